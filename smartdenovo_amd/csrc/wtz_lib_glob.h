/*
 * wtz_lib_glob.h — ksw_global2 as a batch service (wtz_global_batch: K-glob, wtz_sw_kglob.h, and the library's wide forms beyond 2 047 band slots) and
 * kswx_align / kswx_align_with_cigar on top of it and of the three stages of wtz_align_batch (wtz_alignx_batch).  Included by wtz_lib_batch.h.
 */
#define WTZ_GLOB_FORM_RING 33
#define WTZ_GLOB_FORM_SCALAR 255

/* the arguments every problem of a call shares, or WTZ_E_ARG */
static int glob_scores(const wtz_ctx *c, const char *who, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, wtz_kglobsc_t *S){
	CHK(batch_scores(c, who, o_del, e_del, o_ins, e_ins, 0));
	S->M = c->P.M; S->X = c->P.X; S->o_del = o_del; S->e_del = e_del; S->o_ins = o_ins; S->e_ins = e_ins;
	return WTZ_OK;
}
/* problem i from its two views, or WTZ_E_ARG (the LIMITS of include/wtzmo_hip.h) */
static int glob_plan(const wtz_ctx *c, const std::vector<uint64_t> &h_off, const wtz_dp_problem_t &p, uint32_t i, const wtz_kglobsc_t &S, wtz_kglobprob_t *d){
	memset(d, 0, sizeof *d);
	CHK(dp_problem_views(c, h_off, p, i, false, WTZ_LOC_MAXLEN, &d->q, &d->t));
	if(p.W < 0) return wtz_fail(WTZ_E_ARG, "problem %u: band width %d is negative", i, p.W);
	const int32_t diff = p.q_len > p.t_len ? p.q_len - p.t_len : p.t_len - p.q_len;
	if(diff > p.W) return wtz_fail(WTZ_E_ARG, "problem %u: |q_len - t_len| = %d is outside the band %d (the corner cell is not computed)", i, diff, p.W);
	/* every finite DP value lies above minus this: far above the sentinel, whatever path it came by */
	const int64_t o = S.o_del > S.o_ins ? S.o_del : S.o_ins, e = S.e_del > S.e_ins ? S.e_del : S.e_ins, x = S.M > -S.X ? S.M : -S.X, len = p.q_len > p.t_len ? p.q_len : p.t_len;
	if(2 * o + e * ((int64_t)p.q_len + p.t_len + 2) + x * (len + 1) > (1 << 28)) return wtz_fail(WTZ_E_ARG, "problem %u: gap costs x lengths beyond 2^28", i);
	d->qlen = p.q_len; d->tlen = p.t_len; d->w = p.W; d->dlo = p.W < p.t_len - 1 ? p.W : p.t_len - 1;
	return WTZ_OK;
}
/* the form of a problem: slots per lane of the K-glob instantiation, or one of the wide forms (the envelope of wtz_global_wave with the 72 KB slice: wtz_gap_problem_wave) */
static uint32_t glob_form(const wtz_kglobprob_t &d){
	const int32_t slots = wtz_kglob_slots(d.qlen, d.tlen, d.w);
	if(slots <= WTZ_KGLOB_MAXSLOTS) return (uint32_t)wtz_kext_form(slots);
#ifdef WTZ_EMUL
	return WTZ_GLOB_FORM_SCALAR;
#else
	const int32_t n_col = d.qlen < 2 * d.w + 1 ? d.qlen : 2 * d.w + 1, qwords = (d.qlen + 63) / 32 + 1;
	return (n_col + 2 <= 8192 && qwords <= 1024 && (d.tlen + 63) / 64 <= WTZ_TRACE_MAXCHUNK) ? WTZ_GLOB_FORM_RING : WTZ_GLOB_FORM_SCALAR;
#endif
}
/* bytes of the main pool a problem takes while its launch group runs.  K-glob: trace + run buffer, carved by the host.  Wide forms: what their bodies request
 * from the pool on the device (ring: one trace byte per column of a row rounded up to 256 per 4 lanes' columns, chunk tables; scalar: three rows of ints and
 * one byte per cell, each doubling to the next power of two), as an upper estimate: a wrong estimate ends in WTZ_E_POOL, not in a wrong result */
static uint64_t glob_need(const wtz_kglobprob_t &d, uint32_t form, uint32_t *run_cap){
	*run_cap = ((uint32_t)(d.qlen + d.tlen) + 2u + 63u) & ~63u;
	if(form <= 32) return ((wtz_kglob_trace_words((int32_t)form, d.tlen) + 63ull) & ~63ull) * 4ull + (uint64_t)*run_cap * 4ull;
	const uint64_t n_col = (uint64_t)(d.qlen < 2 * d.w + 1 ? d.qlen : 2 * d.w + 1);
	if(form == WTZ_GLOB_FORM_RING) return (n_col + 1024ull) * (uint64_t)(d.tlen + 64) + 8ull * (uint64_t)(d.qlen + d.tlen) + (1ull << 16);
	return 2ull * n_col * (uint64_t)d.tlen + 32ull * (uint64_t)(d.qlen + d.tlen) + (1ull << 16);
}

/* matches and mismatches of a CIGAR's op-0 runs, base by base (the wide forms: lane 0) */
WTZ_HD void wtz_glob_fold(const wtz_kglobprob_t &p, const uint32_t *a, uint32_t n, int32_t &mat, int32_t &mis){
	int32_t x1 = 0, x2 = 0; mat = mis = 0;
	for(uint32_t k = 0; k < n; k++){
		const uint32_t op = a[k] & 0xFu; const int32_t len = (int32_t)(a[k] >> 4);
		if(op == 0){ for(int32_t j = 0; j < len; j++){ if(p.q.at(x1 + j) == p.t.at(x2 + j)) mat++; else mis++; } x1 += len; x2 += len; }
		else if(op == 1) x1 += len;
		else x2 += len;
	}
}
/* form 255: wtz_global_banded on one lane, its rows, trace and CIGAR from the pool */
WTZ_HD void wtz_task_glob_scalar(uint32_t t, const wtz_kglobprob_t *pr, const wtz_kglobsc_t &S, wtz_pool_t *pool, wtz_kglobres_t *res){
	const wtz_kglobprob_t p = pr[t];
	wtz_kglobres_t r; memset(&r, 0, sizeof r);
	wtz_swmem_t mem; wtz_swmem_init(mem, pool);
	wtz_cigar_t tmp; tmp.init(pool, 32);
	r.score = wtz_global_banded(p.qlen, p.q, p.tlen, p.t, S.M, S.X, S.o_del, S.e_del, S.o_ins, S.e_ins, p.w, mem, tmp);
	if(mem.bad || tmp.bad) r.bad = 1;
	else { r.runs = tmp.a; r.n_runs = tmp.n; wtz_glob_fold(p, tmp.a, tmp.n, r.mat, r.mis); }
	res[t] = r;
}
#ifndef WTZ_EMUL
/* form 33: wtz_global_wave with the slice of the wide K-sw2 launch (1 024 query words, two rings of 8 192 columns: wtz_gap_problem_wave) */
static __device__ void wtz_task_glob_ring(uint32_t t, const wtz_kglobprob_t *pr, const wtz_kglobsc_t &S, wtz_pool_t *pool, wtz_kglobres_t *res){
#if defined(__HIP_DEVICE_COMPILE__)
	const wtz_kglobprob_t p = pr[t];
	int32_t *lds = wtz_wave_scratch();
	wtz_wave_lds_t LW; LW.tb = (uint64_t*)lds; LW.Hs = lds + 2048; LW.Es = lds + 2048 + 8192; LW.PM = 8191; LW.tw = 1024; LW.qw = NULL;
	wtz_trace_t tr; tr.chunk = NULL; tr.zb = NULL; tr.n_chunk = 0; tr.zrow = 0; tr.cap_rows = 0;
	wtz_cigar_t tmp; tmp.init(pool, WTZ_LANE == 0 ? 32 : 0);
	bool ok = true;
	const int32_t score = __shfl(wtz_global_wave(p.qlen, p.q, p.tlen, p.t, S.M, S.X, S.o_del, S.e_del, S.o_ins, S.e_ins, p.w, LW, tr, pool, tmp, &ok), 0, 64);
	if(WTZ_LANE != 0) return;
	wtz_kglobres_t r; memset(&r, 0, sizeof r);
	r.score = score;
	if(!ok || tmp.bad) r.bad = 1;
	else { r.runs = tmp.a; r.n_runs = tmp.n; wtz_glob_fold(p, tmp.a, tmp.n, r.mat, r.mis); }
	res[t] = r;
#endif
}
#endif

template<int C> static int kglob_launch(const wtz_kglobprob_t *pr, const uint32_t *order, uint32_t n, const wtz_kglobsc_t &S, uint32_t *blk, wtz_kglobres_t *res){
#ifdef WTZ_EMUL
	std::vector<uint32_t> stg(WTZ_KGLOB_STAGE_WORDS);
	for(uint32_t b = 0; b < n; b++){ const wtz_kglobprob_t &p = pr[order[b]]; wtz_kglob_problem<C>(p, S, blk + p.tr_off, blk + p.run_off, stg.data(), res[order[b]]); }
#else
	WTZ_LAUNCH(wtz_kernel_kglob<C>, n, 64, 0, g_stream, pr, order, n, S, blk, blk, res);
#endif
	return WTZ_OK;
}
/* THE launch path of the banded global: the problems of one score setting.  They are ordered by form (wide forms first, then the widest K-glob instantiation)
 * and inside a form largest first, and cut into launch groups whose traces fit the main pool together; a group is one launch per form present, one wavefront
 * per problem.  hr[i], form[i]: result and form of problem i (hr[i].runs is meaningless on return); the run list of problem i is flat[pos[i], pos[i] + hr[i].n_runs).
 * Counts into ms_kglob / n_kglob / cells_kglob.  Leaves the main pool reset. */
static int glob_run(wtz_ctx *c, const char *who, std::vector<wtz_kglobprob_t> &hp, const wtz_kglobsc_t &S, std::vector<wtz_kglobres_t> &hr, std::vector<uint32_t> &form,
		std::vector<uint32_t> &flat, std::vector<uint64_t> &pos){
	const uint32_t n = (uint32_t)hp.size();
	hr.resize(n); form.resize(n); pos.assign(n, 0); flat.clear();
	if(n == 0) return WTZ_OK;
	const uint64_t budget = c->main_bytes > (1ull << 16) ? c->main_bytes - (1ull << 16) : 0;      /* the pool's own rounding */
	std::vector<uint64_t> need(n);
	for(uint32_t i = 0; i < n; i++){
		form[i] = glob_form(hp[i]); need[i] = glob_need(hp[i], form[i], &hp[i].run_cap);
		if(need[i] > budget) return pool_fail(c, 1, "%s: problem %u (%d x %d, band %d) needs %llu bytes of trace in a main pool of %llu; use a larger pool",
			who, i, hp[i].tlen, hp[i].qlen, hp[i].w, (unsigned long long)need[i], (unsigned long long)c->main_bytes);
	}
	const std::vector<uint32_t> order = batch_order(n, form.data(), need);
	for(uint32_t g0 = 0, g1; g0 < n; g0 = g1){
		const bool wide = form[order[g0]] > 32;      /* a wide form is a launch of its own kind: never mixed with another form */
		uint64_t sum = 0;
		for(g1 = g0; g1 < n && (form[order[g1]] > 32 ? form[order[g1]] == form[order[g0]] : !wide) && sum + need[order[g1]] <= budget; g1++) sum += need[order[g1]];
		const uint32_t m = g1 - g0;
		wtz_arena_scope launch_scope(&c->arena);      /* the buffers of this launch group go back when it ends (scopes nest) */
		CHK(pool_reset(c));
		std::vector<wtz_kglobprob_t> gp(m); std::vector<uint32_t> gorder(m), gform(m);
		uint64_t words = 0;
		for(uint32_t k = 0; k < m; k++){
			wtz_kglobprob_t d = hp[order[g0 + k]];
			gform[k] = form[order[g0 + k]];
			if(!wide){ d.tr_off = words; words += (wtz_kglob_trace_words((int32_t)gform[k], d.tlen) + 63ull) & ~63ull; d.run_off = words; words += d.run_cap; }
			gp[k] = d; gorder[k] = k;
		}
		uint32_t *blk = NULL;
		if(!wide && pool_alloc_host(c, 0, (size_t)words * 4, (void**)&blk) != WTZ_OK) return pool_fail(c, 1, "%s: no room for %llu bytes of trace in the main pool", who, (unsigned long long)words * 4ull);
		wtz_kglobprob_t *d_pr = NULL; uint32_t *d_order = NULL; wtz_kglobres_t *d_res = NULL;
		CHK(batch_upload(gp, gorder, &d_pr, &d_order, &d_res));
		wtz_timer tm; tm.start();
		if(wide){
			wtz_pool_t *pool = c->dpool; const wtz_kglobprob_t *pp = d_pr;
			if(gform[0] == WTZ_GLOB_FORM_SCALAR) CHK(wtz_launch_wave<K_glob_scalar>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_glob_scalar((uint32_t)t, pp, S, pool, d_res); }));
#ifndef WTZ_EMUL
			else CHK(wtz_launch_coop<K_glob_ring>(m, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_glob_ring((uint32_t)t, pp, S, pool, d_res); }, WTZ_GAP_WIDE_LDS_BYTES));
#endif
		} else CHK(for_each_form(m, [&](uint32_t b){ return gform[b]; }, [&](auto K, uint32_t b0, uint32_t b1){ return kglob_launch<decltype(K)::value>(d_pr, d_order + b0, b1 - b0, S, blk, d_res); }));
		std::vector<wtz_kglobres_t> gr;
		CHK(batch_fetch(tm, c->cnt.ms_kglob, m, d_res, gr));
		CHK(pool_check(c, who));
		/* the run lists of the group, packed on the device, behind those of the groups before */
		std::vector<uint64_t> off((size_t)m + 1, 0);
		for(uint32_t k = 0; k < m; k++){
			if(gr[k].bad) return pool_fail(c, 1, "%s: problem %u ran out of scratch", who, order[g0 + k]);
			off[k + 1] = off[k] + gr[k].n_runs;
		}
		const size_t at = flat.size();
		flat.resize(at + (size_t)off[m]);
		const wtz_kglobres_t *rs = d_res;
		CHK(pack_runs<K_globcopy>(off, [=] WTZ_LAMBDA (uint64_t t) -> const uint32_t* { return rs[t].runs; }, flat.data() + at));
		for(uint32_t k = 0; k < m; k++){
			const uint32_t i = order[g0 + k];
			hr[i] = gr[k]; hr[i].runs = NULL; pos[i] = at + off[k];
			if(wide){      /* sum of end - beg over the rows, as the reference's loops execute them */
				unsigned long long cells = 0;
				for(int32_t r = 0; r < hp[i].tlen; r++){ const int32_t beg = r > hp[i].w ? r - hp[i].w : 0, end = r + hp[i].w + 1 < hp[i].qlen ? r + hp[i].w + 1 : hp[i].qlen; if(end > beg) cells += (unsigned long long)(end - beg); }
				hr[i].cells = cells;
			}
			c->cnt.cells_kglob += hr[i].cells;
			if(!wide){ c->cnt.ticks_kglob_dp += hr[i].ticks_dp; c->cnt.ticks_kglob_tb += hr[i].ticks_tb; }
		}
		c->cnt.n_kglob += m;
	}
	return batch_leave(c);
}

/* the fold of kswx.h:1468-1477 over a run list: op 1 (query only) counts as del, op 2 (target only) as ins - the convention of kswx_gen_cigar_core2, not the one
 * of the gap task's fold behind wtz_test_dp */
static void glob_fold_kswx(const uint32_t *a, uint32_t n, int32_t *aln, int32_t *ins, int32_t *del){
	*aln = *ins = *del = 0;
	for(uint32_t k = 0; k < n; k++){ const uint32_t op = a[k] & 0xFu; const int32_t len = (int32_t)(a[k] >> 4); *aln += len; if(op == 1) *del += len; else if(op == 2) *ins += len; }
}
/* the CIGARs of a glob_run to the caller: result_of(k) is where problem k's result goes (it fills what is its own and returns it); aln / ins / del are folded from
 * the run list and, where the caller gave a buffer, the lists are laid one behind the other into it */
template<typename F> static int glob_hand_out(const char *who, const std::vector<wtz_kglobres_t> &hr, const std::vector<uint32_t> &flat, const std::vector<uint64_t> &pos,
		uint32_t *cigar, uint64_t cigar_cap, F result_of){
	uint64_t tot = 0, at = 0;
	for(size_t k = 0; k < hr.size(); k++) tot += hr[k].n_runs;
	if(cigar && tot > cigar_cap) return wtz_fail(WTZ_E_ARG, "%s: CIGAR buffer too small (%llu words needed)", who, (unsigned long long)tot);
	for(size_t k = 0; k < hr.size(); k++){
		auto &o = result_of(k);
		glob_fold_kswx(flat.data() + pos[k], hr[k].n_runs, &o.aln, &o.ins, &o.del);
		if(cigar){ o.cigar_off = at; o.cigar_len = hr[k].n_runs; if(hr[k].n_runs) memcpy(cigar + at, flat.data() + pos[k], (size_t)hr[k].n_runs * 4); at += hr[k].n_runs; }
	}
	return WTZ_OK;
}

/* ksw_global2 (ksw.c:503-586) for n independent problems on views of the uploaded reads */
extern "C" int wtz_global_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins,
		wtz_global_result_t *out, uint32_t *cigar, uint64_t cigar_cap){
	BATCH_ARGS(c, n, pr && out && (cigar || !cigar_cap), "wtz_global_batch", "problems");
	wtz_kglobsc_t S; CHK(glob_scores(c, "wtz_global_batch", o_del, e_del, o_ins, e_ins, &S));
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	std::vector<wtz_kglobprob_t> hp(n);
	for(uint32_t i = 0; i < n; i++) CHK(glob_plan(c, h_off, pr[i], i, S, &hp[i]));
	std::vector<wtz_kglobres_t> hr; std::vector<uint32_t> form, flat; std::vector<uint64_t> pos;
	CHK(glob_run(c, "wtz_global_batch", hp, S, hr, form, flat, pos));
	return glob_hand_out("wtz_global_batch", hr, flat, pos, cigar, cigar_cap, [&](size_t i) -> wtz_global_result_t& {
		wtz_global_result_t &o = out[i]; memset(&o, 0, sizeof o);
		o.score = hr[i].score; o.mat = hr[i].mat; o.mis = hr[i].mis; o.form_used = form[i]; o.cells = hr[i].cells;
		return o;
	});
}

/* the band of kswx_gen_cigar_core2 (kswx.h:1452-1461) for the rectangle [tb, te) x [qb, qe) of score `score`: double arithmetic truncated to int where the reference
 * has it, matrix[0] = M, integer division by -E; a negative w is the exact band -w */
static int32_t alignx_band(int32_t w, int32_t tb, int32_t te, int32_t qb, int32_t qe, int32_t score, int32_t M, int32_t E){
	if(w < 0) return -w;
	int32_t x1 = (te - tb) - (qe - qb);
	if(x1 < 0) x1 = -x1;
	if(w < x1 * 1.5) w = (int32_t)(x1 * 1.5);
	int32_t w2 = (((te - tb < qe - qb) ? te - tb : qe - qb) * M - score) / (-E) + 1;
	if(w2 < (w / 4) + 1) w2 = (w / 4) + 1;
	if(w > w2) w = w2;
	return w;
}

/* kswx_align / kswx_align_with_cigar (kswx.h:1495-1502, 1513-1520) for n independent problems: the three stages of wtz_align_batch, the band rule, one
 * wtz_global_batch stage over the extended rectangles with (-D, -E, -I, -E) */
extern "C" int wtz_alignx_batch(wtz_ctx_t *c, const wtz_dp_problem_t *pr, uint32_t n, int32_t w, int32_t I, int32_t D, int32_t E, int32_t T,
		wtz_alignx_result_t *out, uint32_t *cigar, uint64_t cigar_cap){
	if(w < 0 && w >= -WTZ_KEXT_MAXW && T < 0) return wtz_fail(WTZ_E_ARG, "wtz_alignx_batch: an exact band (w = %d) needs T >= 0: the reference's extensions are not defined for a negative band", w);
	wtz_kextsc_t SR[2];
	CHK(align_args(c, "wtz_alignx_batch", pr, n, out, (w < 0 && w >= -WTZ_KEXT_MAXW) ? 0 : w, I, D, E, T, SR));
	if(n == 0) return WTZ_OK;
	if(!cigar && cigar_cap) return wtz_fail(WTZ_E_ARG, "null argument");
	wtz_kglobsc_t S; CHK(glob_scores(c, "wtz_alignx_batch", -D, -E, -I, -E, &S));
	CHK(batch_count(n, "wtz_local_batch", "problems"));      /* stage 1's limit, under its name */
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	std::vector<wtz_align_result_t> ar(n);
	CHK(align_stages(c, "wtz_alignx_batch", h_off, pr, n, w < 0 ? 0 : w, I, D, E, T, SR, ar.data()));
	std::vector<wtz_kglobprob_t> hp; std::vector<uint32_t> who;
	for(uint32_t i = 0; i < n; i++){
		wtz_alignx_result_t o; memset(&o, 0, sizeof o);
		const wtz_align_result_t &a = ar[i];
		if(a.found){
			o.found = 1; o.score = a.score; o.tb = a.tb; o.te = a.te; o.qb = a.qb; o.qe = a.qe;
			o.band = alignx_band(w, a.tb, a.te, a.qb, a.qe, a.score, c->P.M, E);
			const int32_t dt = a.te - a.tb, dq = a.qe - a.qb, diff = dt > dq ? dt - dq : dq - dt;
			if(dt < 1 || dq < 1 || o.band < diff)
				return wtz_fail(WTZ_E_STATE, "wtz_alignx_batch: problem %u: the band rule gives %d for the %d x %d rectangle of score %d: the corner is outside the band, the DP is not run", i, o.band, dt, dq, a.score);
			const wtz_dp_problem_t &p = pr[i];
			wtz_dp_problem_t e = p;
			e.q_from = p.q_from + p.q_strand * a.qb; e.q_len = dq; e.t_from = p.t_from + p.t_strand * a.tb; e.t_len = dt; e.W = o.band; e.init_score = 0;
			wtz_kglobprob_t d; CHK(glob_plan(c, h_off, e, i, S, &d));
			hp.push_back(d); who.push_back(i);
		}
		out[i] = o;
	}
	std::vector<wtz_kglobres_t> hr; std::vector<uint32_t> form, flat; std::vector<uint64_t> pos;
	CHK(glob_run(c, "wtz_alignx_batch", hp, S, hr, form, flat, pos));
	return glob_hand_out("wtz_alignx_batch", hr, flat, pos, cigar, cigar_cap, [&](size_t k) -> wtz_alignx_result_t& {
		wtz_alignx_result_t &o = out[who[k]];
		o.score = hr[k].score; o.mat = hr[k].mat; o.mis = hr[k].mis; o.form_used = form[k];
		return o;
	});
}
