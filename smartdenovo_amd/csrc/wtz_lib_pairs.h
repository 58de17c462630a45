/*
 * wtz_lib_pairs.h — the per-batch pair stages in front of the alignment: wtz_batch_begin, wtz_pairs_seed (K_pair and the launches that finish what it
 * leaves), wtz_pairs_seed_region (the same with one interval of the indexed read per pair: K_pair_region), wtz_set_window_chaining (both through K_pair_chain)
 * and wtz_pairs_windows.  Included by wtz_lib.cpp.
 */
#ifndef WTZ_PAIR_DM_LDS_TIER2
#define WTZ_PAIR_DM_LDS_TIER2 49152u
#endif
/* the last two launches keep only the band work arrays in LDS (the per-match image of a strand goes to the pool when it does not fit):
 * what a heavy pair needs is resident waves, not LDS - a 159 KB slice meant ONE wave per CU, and the repeat-rich 40 Mbp set spent 14 of
 * its 15 s there (159 KB: 13.8 s, 76: 7.1, 50: 5.0, 36: 4.1).  Tier 3 = eight waves per CU with room for ~2 000 linear groups per
 * strand, tier 4 = four waves per CU with 8 191. */
#ifndef WTZ_PAIR_DM_LDS_TIER3
#define WTZ_PAIR_DM_LDS_TIER3 20480u
#endif
#ifndef WTZ_PAIR_DM_LDS_TIER4
#define WTZ_PAIR_DM_LDS_TIER4 36864u
#endif
/* ------------------------------------------------------------------------------------------------ */
/* per-batch pair stages                                                                             */
/* ------------------------------------------------------------------------------------------------ */
extern "C" int wtz_batch_begin(wtz_ctx_t *c){
	if(!c) return wtz_fail(WTZ_E_ARG, "null context");
	CTX_ENTER(c);
	free_batch(c);
	return pool_reset(c);
}

/* The heavy-first list of wtz_pair_order (wtz_tasks.h): the n / 32 pairs with the largest len(q) * len(c), largest first, then the others in the plan order, as a
 * device array; *nh = how many head it.  Fewer than 8 of them, or the switch off: no list (*d_ord = NULL, *nh = 0).  WTZ_PAIR_HEAVY_FIRST=0 / 1 overrides the
 * engine default (dmo on; zmo off: its launches were measured full to the end).  The host emulation runs its pairs in the caller's order. */
static int pairs_heavy_first(wtz_ctx_t *c, const uint32_t *qid, const uint32_t *cid, uint32_t n, const uint32_t **d_ord, uint32_t *nh){
	*d_ord = NULL; *nh = 0;
#ifndef WTZ_EMUL
	if(!(c->sw.heavy_first >= 0 ? c->sw.heavy_first != 0 : c->P.dot_matrix != 0) || n / 32u < 8u) return WTZ_OK;
	const uint32_t k = n / 32u;
	std::vector<uint64_t> key(n); std::vector<uint32_t> ord(n), hv(n);
	for(uint32_t i = 0; i < n; i++){ key[i] = (uint64_t)c->h_rdlen[qid[i]] * c->h_rdlen[cid[i]]; hv[i] = i; }
	const auto heavier = [&](uint32_t a, uint32_t b){ return key[a] != key[b] ? key[a] > key[b] : a < b; };
	std::nth_element(hv.begin(), hv.begin() + k, hv.end(), heavier);
	std::sort(hv.begin(), hv.begin() + k, heavier);
	std::vector<uint8_t> heavy(n, 0);
	for(uint32_t i = 0; i < k; i++){ ord[i] = hv[i]; heavy[hv[i]] = 1; }
	uint32_t w = k; for(uint32_t i = 0; i < n; i++) if(!heavy[i]) ord[w++] = i;
	uint32_t *dd = NULL; CHK(dev_alloc((void**)&dd, (size_t)n * 4)); CHK(dev_h2d(dd, ord.data(), (size_t)n * 4));
	*d_ord = dd; *nh = k;
#else
	(void)c; (void)qid; (void)cid; (void)n;
#endif
	return WTZ_OK;
}

/* wtz_pairs_seed (beg == NULL) and wtz_pairs_seed_region (one interval [beg[i], end[i]) of read qid[i] per pair, defaults applied by the caller): the
 * two differ in the first launch only, K_pair or K_pair_region.  After wtz_set_window_chaining(ctx, 0) that launch is K_pair_chain for both: the whole form is
 * the interval [0, length of the indexed read), which cuts nothing (hzm_aln.h:1690-1691) */
static int pairs_seed_run(wtz_ctx_t *c, const char *who, const uint32_t *qid, const uint32_t *cid, const int32_t *beg, const int32_t *end, uint32_t n, wtz_pair_summary_t *out){
	if(!c || !c->zs[0].have || (n && (!qid || !cid || !out))) return wtz_fail(WTZ_E_ARG, "z-index not built / null argument");
	CTX_ENTER(c);
	free_batch(c);
	CHK(pool_reset(c));
	if(n == 0){ c->n_pairs = 0; c->h_pairres.clear(); c->have_pairs = true; return WTZ_OK; }
	for(uint32_t i = 0; i < n; i++) if(qid[i] >= c->n_reads || cid[i] >= c->n_reads) return wtz_fail(WTZ_E_ARG, "pair %u: read id out of range", i);
	CHK(reserve_pairs(c, n));
	CHK(dev_h2d(c->d_qid, qid, (size_t)n * 4)); CHK(dev_h2d(c->d_cid, cid, (size_t)n * 4));
	int32_t *d_beg = NULL, *d_end = NULL;
	const bool chain = c->window_chaining == 0;
	if(beg || chain){
		/* the defaults of hzm_aln.h:1690-1691: beg < 0 -> 0, end <= 0 -> the length of the indexed read; an end behind the read stays as it is (it excludes nothing) */
		std::vector<int32_t> b(n), e(n);
		for(uint32_t i = 0; i < n; i++){ b[i] = (!beg || beg[i] < 0) ? 0 : beg[i]; e[i] = (!beg || end[i] <= 0) ? (int32_t)c->h_rdlen[qid[i]] : end[i]; }
		CHK(dev_alloc((void**)&d_beg, (size_t)n * 4)); CHK(dev_h2d(d_beg, b.data(), (size_t)n * 4));
		CHK(dev_alloc((void**)&d_end, (size_t)n * 4)); CHK(dev_h2d(d_end, e.data(), (size_t)n * 4));
	}
	const wtz_env_t V = ctx_env(c); const uint32_t *dq = c->d_qid, *dc = c->d_cid; wtz_pairres_t *dr = c->d_pairres;
	wtz_timer tm; tm.start();
	wtz_timer t1; t1.start();
	const char *kname = chain ? "K_pair_chain" : beg ? "K_pair_region" : "K_pair";
	STAGE(c, kname);
	uint32_t nh = 0; const uint32_t *d_ord = NULL;
	CHK(pairs_heavy_first(c, qid, cid, n, &d_ord, &nh));
	const wtz_pair_order order = { nh, n - nh, c->sw.xcd_group, d_ord };
	/* ---- the first launch: every pair ---- */
#ifdef WTZ_EMUL
	/* the host emulation: one loop over the pairs in the caller's order, engine and form chosen per call (ENGINE = -1) */
	(void)order;
	CHK(wtz_launch_coop<K_pair>(n, [=] WTZ_LAMBDA (uint64_t b){
		if(chain) wtz_task_pair<-1, true, true>((uint32_t)b, V, dq, dc, dr, d_beg, d_end);
		else if(d_beg) wtz_task_pair<-1, true>((uint32_t)b, V, dq, dc, dr, d_beg, d_end);
		else wtz_task_pair<-1>((uint32_t)b, V, dq, dc, dr); }, c->P.dot_matrix ? WTZ_PAIR_DM_LDS_BYTES : WTZ_PAIR_LDS_BYTES));
#else
	/* K_pair_chain and K_pair_region take the pairs in the caller's order: the pairs of a layout share ONE query table, the backbone's, so there is nothing for the XCD mapping to keep together */
	if(chain)                 CHK(wtz_launch_coop<K_pair_chain>(n, [=] WTZ_LAMBDA (uint64_t b){ wtz_task_pair<0, true, true>((uint32_t)b, V, dq, dc, dr, d_beg, d_end); }, WTZ_PAIR_LDS_BYTES));
	else if(beg)              CHK(wtz_launch_coop<K_pair_region>(n, [=] WTZ_LAMBDA (uint64_t b){ wtz_task_pair<0, true>((uint32_t)b, V, dq, dc, dr, d_beg, d_end); }, WTZ_PAIR_LDS_BYTES));
	else if(c->P.dot_matrix)  CHK(wtz_launch_coop<K_pair_dm>(n, [=] WTZ_LAMBDA (uint64_t b){ wtz_task_pair<1>(order(b), V, dq, dc, dr); }, WTZ_PAIR_DM_LDS_BYTES));
	else                      CHK(wtz_launch_coop<K_pair>(n, [=] WTZ_LAMBDA (uint64_t b){ wtz_task_pair<0>(order(b), V, dq, dc, dr); }, WTZ_PAIR_LDS_BYTES));
#endif
	CHK(dev_sync());
	{ const double ms1 = t1.stop(); if(c->sw.profile) fprintf(stderr, "[pair-profile] %s first launch: %u pairs, %.1f ms\n", kname, n, ms1); }
	c->n_pairs = n; c->h_pairres.resize(n); c->have_pairs = true;
	CHK(dev_d2h(c->h_pairres.data(), c->d_pairres, (size_t)n * sizeof(wtz_pairres_t)));
	/* ---- the finishers: a launch over the pairs of h_pairres that `want` picks (a device list of their indexes), the results read back; *n_list = how many ---- */
	auto finish = [&](const char *stage, const char *what, auto want, auto launch, size_t *n_list) -> int {
		std::vector<uint32_t> list;
		for(uint32_t i = 0; i < n; i++) if(want(c->h_pairres[i])) list.push_back(i);
		*n_list = list.size();
		if(list.empty()) return WTZ_OK;
		uint32_t *d_list = NULL; CHK(dev_alloc((void**)&d_list, list.size() * 4)); CHK(dev_h2d(d_list, list.data(), list.size() * 4));
		wtz_timer tt; tt.start();
		STAGE(c, stage);
		CHK(launch(d_list, list.size()));
		CHK(dev_sync());
		const double ms_t = tt.stop();
		CHK(dev_d2h(c->h_pairres.data(), c->d_pairres, (size_t)n * sizeof(wtz_pairres_t)));
		if(c->sw.profile) fprintf(stderr, "[pair-profile] %s: %zu pairs, %.1f ms\n", what, list.size(), ms_t);
		return WTZ_OK;
	};
	if(c->P.dot_matrix){
		/* pairs whose strand images exceed the LDS slice of K_pair_dm are finished by launches with larger slices: few pairs,
		 * but they are the long ones that would otherwise bound the batch from a single lane */
		uint32_t tiers[3] = { WTZ_PAIR_DM_LDS_TIER2, WTZ_PAIR_DM_LDS_TIER3, WTZ_PAIR_DM_LDS_TIER4 };
		if(getenv("WTZ_DM_TIER3_KB")) tiers[1] = (uint32_t)atoi(getenv("WTZ_DM_TIER3_KB")) << 10;
		if(getenv("WTZ_DM_TIER4_KB")) tiers[2] = (uint32_t)atoi(getenv("WTZ_DM_TIER4_KB")) << 10;
		/* with the pool image allowed in the first launch only what overflowed its group table or band list is left: the last launch's */
		for(int tier = c->sw.dm_first_big ? 2 : 0; tier < 3; tier++){
			const uint32_t lb = tiers[tier]; const bool last = (tier == 2), big = (tier >= 1);
			char what[64]; snprintf(what, sizeof what, "dmo tier %d (%u KB LDS)", tier + 2, lb >> 10);
			size_t left = 0;
			CHK(finish("K_pair_big", what, [](const wtz_pairres_t &r){ return r.gate && r.dm_dir == -2 && !r.bad; }, [=](const uint32_t *d_list, size_t k){
				return wtz_launch_coop<K_pair_big>(k, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_pair_dm_big((uint32_t)t, V, d_list, dq, dc, dr, lb, last, big); }, lb); }, &left));
			if(left == 0) break;
		}
	}
	/* ---- counters, profile, summaries ---- */
	c->cnt.ms_pairs += tm.stop(); c->cnt.n_pairs += n;
	for(uint32_t i = 0; i < n; i++) c->cnt.bytes_zmer_algo += (uint64_t)c->h_rdlen[cid[i]] / 4 + 16ull * c->h_pairres[i].n_hits;
	CHK(pool_check(c, who));
	if(c->sw.profile){
		uint64_t sum[4] = {0, 0, 0, 0}; uint32_t mx[4] = {0, 0, 0, 0}, arg = 0;
		for(uint32_t i = 0; i < n; i++){ for(int k = 0; k < 4; k++){ sum[k] += c->h_pairres[i].tick[k]; if(c->h_pairres[i].tick[k] > mx[k]){ mx[k] = c->h_pairres[i].tick[k]; if(k == 3) arg = i; } } }
		fprintf(stderr, "[pair-profile] n=%u kticks sum match/sort/win/total %llu/%llu/%llu/%llu max %u/%u/%u/%u; slowest pair: hits %u (its match/sort/win %u/%u/%u)\n", n,
			(unsigned long long)sum[0], (unsigned long long)sum[1], (unsigned long long)sum[2], (unsigned long long)sum[3], mx[0], mx[1], mx[2], mx[3],
			c->h_pairres[arg].n_hits, c->h_pairres[arg].tick[0], c->h_pairres[arg].tick[1], c->h_pairres[arg].tick[2]);
	}
	for(uint32_t i = 0; i < n; i++){
		const wtz_pairres_t &r = c->h_pairres[i];
		if(r.bad) return wtz_fail(WTZ_E_POOL, "%s: pair %u ran out of scratch", who, i);
		wtz_pair_summary_t s; memset(&s, 0, sizeof s);
		s.n_hits = r.n_hits; s.gate = r.gate; s.ovl[0] = r.ovl[0]; s.ovl[1] = r.ovl[1]; s.nwin[0] = r.nwin[0]; s.nwin[1] = r.nwin[1];
		s.dm_score = r.dm_score; s.dm_qb = r.dm_qb; s.dm_qe = r.dm_qe; s.dm_tb = r.dm_tb; s.dm_te = r.dm_te; s.dm_dir = r.dm_dir;
		out[i] = s;
	}
	return WTZ_OK;
}
extern "C" int wtz_pairs_seed(wtz_ctx_t *c, const uint32_t *qid, const uint32_t *cid, uint32_t n, wtz_pair_summary_t *out){
	return pairs_seed_run(c, "wtz_pairs_seed", qid, cid, NULL, NULL, n, out);
}
/* align_hzmaux's form of the pair stages wants params.aux_strand = 1 and the zmo engine */
static int region_args(const wtz_ctx *c, const char *who){
	if(c && (c->P.aux_strand == 0 || c->P.dot_matrix != 0)) return wtz_fail(WTZ_E_ARG, "%s: needs params.aux_strand = 1 and the zmo engine (align_hzmaux, hzm_aln.h:1684-1775)", who);
	return WTZ_OK;
}
extern "C" int wtz_pairs_seed_region(wtz_ctx_t *c, const uint32_t *qid, const uint32_t *cid, const int32_t *beg, const int32_t *end, uint32_t n, wtz_pair_summary_t *out){
	CHK(region_args(c, "wtz_pairs_seed_region"));
	if(n && (!beg || !end)) return wtz_fail(WTZ_E_ARG, "null argument");
	return pairs_seed_run(c, "wtz_pairs_seed_region", qid, cid, beg, end, n, out);
}

/* HZM_FAST_WINDOW_KMER_CHAINING of the reference (hzm_aln.h:36), per context: 1 = the median-diagonal filter of hzm_aln.h:488-543, 0 = chaining_hzmps, hzm_aln.h:544-561 */
extern "C" int wtz_set_window_chaining(wtz_ctx_t *c, int fast){
	if(!c) return wtz_fail(WTZ_E_ARG, "null context");
	if(!fast) CHK(region_args(c, "wtz_set_window_chaining(0)"));
	c->window_chaining = fast ? 1 : 0;
	return WTZ_OK;
}

extern "C" int wtz_pairs_windows(wtz_ctx_t *c, wtz_winbox_t *wins, uint64_t n_wins){
	if(!c || !c->have_pairs) return wtz_fail(WTZ_E_STATE, "wtz_pairs_windows before wtz_pairs_seed");
	CTX_ENTER(c);
	uint64_t tot = 0; for(uint32_t i = 0; i < c->n_pairs; i++) tot += c->h_pairres[i].nwin[0] + c->h_pairres[i].nwin[1];
	if(tot != n_wins) return wtz_fail(WTZ_E_ARG, "wtz_pairs_windows: expected room for %llu windows, got %llu", (unsigned long long)tot, (unsigned long long)n_wins);
	if(tot == 0) return WTZ_OK;
	if(!wins) return wtz_fail(WTZ_E_ARG, "null output");
	std::vector<uint64_t> off((size_t)c->n_pairs * 2 + 1);
	uint64_t o = 0; for(uint32_t i = 0; i < c->n_pairs; i++) for(int d = 0; d < 2; d++){ off[(size_t)i * 2 + d] = o; o += c->h_pairres[i].nwin[d]; }
	off[(size_t)c->n_pairs * 2] = o;
	uint64_t *d_off = NULL; wtz_winbox_t *d_w = NULL;
	CHK(dev_alloc((void**)&d_off, off.size() * 8)); CHK(dev_h2d(d_off, off.data(), off.size() * 8));
	CHK(dev_alloc((void**)&d_w, (size_t)tot * sizeof(wtz_winbox_t)));
	const wtz_pairres_t *dr = c->d_pairres;
	CHK(wtz_launch<K_pack_windows>((uint64_t)c->n_pairs * 2, [=] WTZ_LAMBDA (uint64_t t){
		const wtz_pairres_t &r = dr[t >> 1]; const uint32_t d = (uint32_t)(t & 1);
		for(uint32_t k = 0; k < r.nwin[d]; k++){ wtz_winbox_t b; b.beg[0] = r.win[d][k].beg[0]; b.beg[1] = r.win[d][k].beg[1]; b.end[0] = r.win[d][k].end[0]; b.end[1] = r.win[d][k].end[1]; d_w[d_off[t] + k] = b; }
	}));
	CHK(dev_sync());
	CHK(dev_d2h(wins, d_w, (size_t)tot * sizeof(wtz_winbox_t)));
	return WTZ_OK;
}
