/*
 * wtz_lib_pwtext.h — the alignment picture as a batch service (wtz_pwtext_batch: K-pwtext, wtz_pwtext.h).  Included by wtz_lib_batch.h.
 */
struct pwt_plan_t { wtz_pwtprob_t d; uint64_t need; };

/* alignment i from its views, its start and its CIGAR slice, or WTZ_E_ARG: everything the reference leaves unchecked (kswx.h:1150-1194 reads the sequences as far
 * as the CIGAR says and exits on an unknown op) */
static int pwt_plan(const wtz_ctx *c, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t &p, const wtz_pwtext_in_t &in, uint32_t i, const uint32_t *cigar, uint64_t n_ops, pwt_plan_t *P){
	memset(&P->d, 0, sizeof P->d);
	wtz_seq_packed q, t;
	CHK(dp_problem_views(c, h_off, p, i, true, WTZ_PWT_MAXLEN, &q, &t));
	if(in.qb < 0 || in.qb > p.q_len || in.tb < 0 || in.tb > p.t_len) return wtz_fail(WTZ_E_ARG, "alignment %u: start (%d, %d) outside its %d x %d views", i, in.qb, in.tb, p.q_len, p.t_len);
	if(in.cigar_off > n_ops || (uint64_t)in.cigar_len > n_ops - in.cigar_off) return wtz_fail(WTZ_E_ARG, "alignment %u: CIGAR slice [%llu, +%u) outside the %llu words given", i, (unsigned long long)in.cigar_off, in.cigar_len, (unsigned long long)n_ops);
	wtz_dp_problem_t e = p;
	e.q_from = p.q_from + p.q_strand * in.qb; e.q_len = p.q_len - in.qb; e.t_from = p.t_from + p.t_strand * in.tb; e.t_len = p.t_len - in.tb;
	CHK(dp_problem_views(c, h_off, e, i, true, WTZ_PWT_MAXLEN, &P->d.q, &P->d.t));
	uint64_t nq = 0, nt = 0;
	for(uint32_t k = 0; k < in.cigar_len; k++){
		const uint32_t w = cigar[in.cigar_off + k], op = w & 0xFu; const uint64_t len = w >> 4;
		if(op > 2u) return wtz_fail(WTZ_E_ARG, "alignment %u: operation %u of its CIGAR has op %u (0, 1 and 2 are defined)", i, k, op);
		if(op != 2u) nq += len;
		if(op != 1u) nt += len;
		if(nq > (uint64_t)e.q_len || nt > (uint64_t)e.t_len) return wtz_fail(WTZ_E_ARG, "alignment %u: its CIGAR walks past the end of a view at operation %u (%d query and %d target bases from the start)", i, k, e.q_len, e.t_len);
	}
	uint64_t cols = 0;
	for(uint32_t k = 0; k < in.cigar_len; k++) cols += cigar[in.cigar_off + k] >> 4;
	P->d.qlen = e.q_len; P->d.tlen = e.t_len; P->d.n_ops = in.cigar_len; P->d.cols = (uint32_t)cols;
	P->need = 12ull * in.cigar_len + 3ull * (cols + 1ull);      /* table entry + CIGAR word per operation, the picture */
	return WTZ_OK;
}

/* kswx_cigar2pairwise (kswx.h:1150-1194) + the marker line of pairaln.c:115-125 for n alignments on views of the uploaded reads */
extern "C" int wtz_pwtext_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, const wtz_pwtext_in_t *in, uint32_t n, const uint32_t *cigar, uint64_t n_ops,
		wtz_pwtext_result_t *out, char *text, uint64_t text_cap){
	BATCH_ARGS(c, n, pr && in && out && (cigar || !n_ops) && (text || !text_cap), "wtz_pwtext_batch", "alignments");
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	c->main_used_call = 0;
	std::vector<pwt_plan_t> plan(n);
	std::vector<uint64_t> toff((size_t)n + 1);
	uint64_t tot = 0;
	for(uint32_t i = 0; i < n; i++){ CHK(pwt_plan(c, h_off, pr[i], in[i], i, cigar, n_ops, &plan[i])); toff[i] = tot; tot += 3ull * ((uint64_t)plan[i].d.cols + 1ull); }
	toff[n] = tot;
	if(text && tot > text_cap) return wtz_fail(WTZ_E_ARG, "wtz_pwtext_batch: text buffer too small (%llu bytes needed)", (unsigned long long)tot);
	const uint64_t slack = 4096, budget = c->main_bytes > (1ull << 16) + slack ? c->main_bytes - (1ull << 16) - slack : 0;      /* the pool's own rounding, the blocks' alignment */
	for(uint32_t i = 0; i < n; i++){
		wtz_pwtext_result_t o; memset(&o, 0, sizeof o); o.text_off = toff[i]; o.cols = plan[i].d.cols; out[i] = o;
		if(text && plan[i].need > budget) return pool_fail(c, 1, "wtz_pwtext_batch: alignment %u (%u operations, %u columns) needs %llu bytes in a main pool of %llu; use a larger pool",
			i, plan[i].d.n_ops, plan[i].d.cols, (unsigned long long)plan[i].need, (unsigned long long)c->main_bytes);
	}
	if(!text) return WTZ_OK;      /* the sizing call */
	for(uint32_t g0 = 0, g1; g0 < n; g0 = g1){
		uint64_t sum = 0, ops = 0, tiles = 0;
		for(g1 = g0; g1 < n && sum + plan[g1].need <= budget; g1++){ sum += plan[g1].need; ops += plan[g1].d.n_ops; tiles += (uint64_t)plan[g1].d.cols / WTZ_PWT_TILE + 1ull; }
		const uint32_t m = g1 - g0;
		if(tiles > 0x7FFFFFFFull) return wtz_fail(WTZ_E_ARG, "wtz_pwtext_batch: more than 2^31 - 1 tiles in one launch group");
		wtz_arena_scope launch_scope(&c->arena);      /* the buffers of this launch group go back when it ends (scopes nest) */
		CHK(pool_reset(c));
		const uint64_t tbytes = toff[g1] - toff[g0];
		std::vector<wtz_pwtprob_t> gp(m); std::vector<wtz_pwttile_t> gt((size_t)tiles); std::vector<uint32_t> gc((size_t)ops);
		uint64_t at = 0, nt = 0;
		for(uint32_t k = 0; k < m; k++){
			wtz_pwtprob_t d = plan[g0 + k].d;
			d.cig_off = d.tab_off = at; d.text_off = toff[g0 + k] - toff[g0];
			if(d.n_ops) memcpy(gc.data() + at, cigar + in[g0 + k].cigar_off, (size_t)d.n_ops * 4);
			at += d.n_ops;
			for(uint32_t t = 0; t <= d.cols / WTZ_PWT_TILE; t++){ gt[(size_t)nt].prob = k; gt[(size_t)nt].tile = t; nt++; }
			gp[k] = d;
		}
		/* one block of the main pool: the table, the CIGAR words, the picture */
		const uint64_t tab_bytes = (8ull * ops + 255ull) & ~255ull, cig_bytes = (4ull * ops + 255ull) & ~255ull;
		uint8_t *blk = NULL;
		if(pool_alloc_host(c, 0, (size_t)(tab_bytes + cig_bytes + tbytes + 256ull), (void**)&blk) != WTZ_OK) return pool_fail(c, 1, "wtz_pwtext_batch: no room for %llu bytes in the main pool", (unsigned long long)(tab_bytes + cig_bytes + tbytes));
		unsigned long long *d_tab = (unsigned long long*)blk; uint32_t *d_cig = (uint32_t*)(blk + tab_bytes); char *d_text = (char*)(blk + tab_bytes + cig_bytes);
		wtz_pwtprob_t *d_pr = NULL; wtz_pwttile_t *d_tiles = NULL; uint32_t *d_nent = NULL;
		CHK(dev_alloc((void**)&d_pr, (size_t)m * sizeof(wtz_pwtprob_t))); CHK(dev_h2d(d_pr, gp.data(), (size_t)m * sizeof(wtz_pwtprob_t)));
		CHK(dev_alloc((void**)&d_tiles, (size_t)tiles * sizeof(wtz_pwttile_t))); CHK(dev_h2d(d_tiles, gt.data(), (size_t)tiles * sizeof(wtz_pwttile_t)));
		CHK(dev_alloc((void**)&d_nent, (size_t)m * 4));
		CHK(dev_h2d(d_cig, gc.data(), (size_t)ops * 4));
		wtz_timer tm; tm.start();
#ifndef WTZ_EMUL
		WTZ_LAUNCH(wtz_kernel_pwscan, m, 64, 0, g_stream, (const wtz_pwtprob_t*)d_pr, m, (const uint32_t*)d_cig, d_tab, d_nent);
		WTZ_LAUNCH(wtz_kernel_pwtext, (uint32_t)tiles, 64, 0, g_stream, (const wtz_pwtprob_t*)d_pr, (const wtz_pwttile_t*)d_tiles, (uint32_t)tiles, (const unsigned long long*)d_tab, (const uint32_t*)d_nent, d_text);
#else
		for(uint32_t k = 0; k < m; k++) d_nent[k] = wtz_pwtext_scan(d_cig + d_pr[k].cig_off, d_pr[k].n_ops, d_tab + d_pr[k].tab_off);
		{
			std::vector<unsigned long long> ent(WTZ_PWT_TILE); std::vector<uint32_t> pic(3 * WTZ_PWT_LINE_WORDS);
			for(uint64_t b = 0; b < tiles; b++){ const wtz_pwtprob_t &p = d_pr[d_tiles[b].prob]; wtz_pwtext_tile(p, d_tiles[b].tile, d_tab + p.tab_off, d_nent[d_tiles[b].prob], ent.data(), pic.data(), d_text); }
		}
#endif
		CHK(dev_sync());
		c->cnt.ms_pwtext += tm.stop();
		CHK(dev_d2h(text + toff[g0], d_text, (size_t)tbytes));
		CHK(pool_check(c, "wtz_pwtext_batch"));
		c->cnt.n_pwtext += m; c->cnt.bytes_pwtext += tbytes;
	}
	return batch_leave(c);
}
