/*
 * wtz_testdp.h — wtz_test_dp(): the TEST-ONLY entry of the C ABI (include/wtzmo_hip.h).  It runs single banded-DP problems through a
 * chosen device form of K-sw1 / K-sw2 / K-sw3 so that every form can be compared, function by function, with vectors dumped from the
 * reference's own kswx_extend_align_core (kswx.h:234), kswx_extend_align_shift_core (kswx.h:101) and ksw_global2 (ksw.c:503).
 * The forms are selected by the very functions the product kernels call (wtz_fixed_problem_wave, wtz_gap_problem_wave, run_extjobs and
 * the extension-job kernels); this file only wraps problems into their inputs and collects the results.  Included by wtz_lib_batch.h.
 */
#ifndef WTZ_TESTDP_H
#define WTZ_TESTDP_H

struct K_test_fixed;
struct K_test_global;
struct K_test_global_wide;
struct K_test_lane;

typedef struct { wtz_seq_packed q, t; int32_t qlen, tlen, init_score, W; } wtz_dpprob_dev_t;
typedef struct { wtz_aln_t x; uint32_t *cigar; uint32_t cigar_len; int32_t form, bad; unsigned long long cells; } wtz_dpres_dev_t;

/*
 * Form 65: the lane bodies of wtz_sw_lane.h the way the product runs them - WTZ_NLANES problems per wavefront in the CALLER's order (problems 64k .. 64k+63 share
 * wavefront k; nothing is sorted, the last wavefront may be partial), K-sw1 in the relative mode, and two launches: the forward DP writes the wave's lane-interleaved
 * trace block into the transient pool (K_ldp / K_gdp), the second launch walks it back, lane l the rows lane l wrote (K_ltb / K_gtb).  The instantiation NC of a
 * wavefront is the class of its widest live problem.  The task bodies below restate the wrappers wtz_task_ldp / _ltb / _gdp / _gtb around the SAME lane bodies, with
 * a test problem in the place of a window's slot; the host emulation runs them with one lane, one problem per "wavefront".
 */
WTZ_HD int32_t wtz_test_l65_band(const wtz_dpprob_dev_t &p, const wtz_params_t *P){ return p.W > 0 ? p.W : P->w; }      /* WTZ_DP_FIXED: W > 0 names the -w of this problem, 0 = params.w */
/* what wtz_task_lplan leaves to the chained kernel (and an empty side): false = form 65 declines the problem */
WTZ_HD bool wtz_test_l65_fixed_geo(const wtz_dpprob_dev_t &p, const wtz_params_t *P, int32_t &W, int32_t &ql, int32_t &tl, int32_t &n_col){
	W = wtz_test_l65_band(p, P); ql = tl = n_col = 0;
	if(p.qlen <= 0 || p.tlen <= 0) return false;
	int32_t W1 = W, ql1, tl1, nc1;
	wtz_ext_geometry(p.qlen, p.tlen, 0, W, P->M, P->I, P->D, P->E, P->T, ql, tl, n_col);
	wtz_ext_geometry(p.qlen, p.tlen, 1 << 24, W1, P->M, P->I, P->D, P->E, P->T, ql1, tl1, nc1);
	return !(W != W1 || n_col > WTZ_LN_MAXCOLS || ql > WTZ_LN_MAXROWS || ql + tl > WTZ_LN_MAXSPAN);
}
/* form 64's envelope of the lane K-sw2 */
WTZ_HD bool wtz_test_l65_global_geo(const wtz_dpprob_dev_t &p, int32_t &n_col){
	n_col = p.qlen < 2 * p.W + 1 ? p.qlen : 2 * p.W + 1;
	return !(p.qlen <= 0 || p.tlen <= 0 || p.W <= 0 || WTZ_ABSDIFF(p.qlen, p.tlen) > p.W || n_col > WTZ_LN_MAXCOLS || p.tlen > WTZ_LG_MAXROWS);
}
/* first launch, wavefront wv: wtr[wv] = the wave's trace block, wrs[wv] = its trace dwords per row; res[i].flags stays 0 for a problem that was declined */
template<bool GLOBAL>
WTZ_HD void wtz_task_test_ldp(uint32_t wv, const wtz_dpprob_dev_t *pr, uint32_t n, const wtz_env_t &V, wtz_lres_t *res, uint64_t *wtr, uint32_t *wrs){
	const wtz_params_t *P = V.P;
	const uint32_t idx = wv * WTZ_NLANES + WTZ_LANE;
	wtz_dpprob_dev_t p; memset(&p, 0, sizeof p);
	p.q.bits = p.t.bits = V.R.bits; p.q.strand = p.t.strand = 1;
	bool live = idx < n;
	if(live) p = pr[idx];
	const int32_t M = P->M, X = P->X, I = P->I, D = P->D, E = P->E, T = P->T;
	int32_t W = P->w, ql = 0, tl = 0, n_col = 0;
	if(live) live = GLOBAL ? wtz_test_l65_global_geo(p, n_col) : wtz_test_l65_fixed_geo(p, P, W, ql, tl, n_col);
	if(!live){ ql = tl = n_col = 0; p.qlen = p.tlen = 0; }
	const int32_t rows = GLOBAL ? p.tlen : ql;
	const int32_t ncmax = wtz_lane_wmax(n_col);
	const uint32_t RS = wtz_lane_rs(ncmax);
	const uint32_t rows_max = (uint32_t)wtz_lane_wmax(rows);
	uint64_t pa = 0;
	if(WTZ_LANE == 0){
		pa = (uint64_t)(uintptr_t)wtz_pool_alloc(V.pool + 1, (size_t)WTZ_NLANES * rows_max * RS * 4 + 16);      /* as wtz_task_ldp / wtz_task_gdp: the transient pool */
		wtr[wv] = pa; wrs[wv] = RS;
	}
	pa = wtz_coop_bcast64(pa);
	if(pa == 0) return;                       /* the host reports the pool */
	uint32_t *tr = (uint32_t*)(uintptr_t)pa;
	wtz_lres_t R; memset(&R, 0, sizeof R);
	if(GLOBAL){
		if(ncmax <= 16)      wtz_lane_global<16>(live, p.qlen, p.q, p.tlen, p.t, p.W, M, X, -I, -E, -D, -E, tr, R);
		else if(ncmax <= 32) wtz_lane_global<32>(live, p.qlen, p.q, p.tlen, p.t, p.W, M, X, -I, -E, -D, -E, tr, R);
		else if(ncmax <= 64) wtz_lane_global<64>(live, p.qlen, p.q, p.tlen, p.t, p.W, M, X, -I, -E, -D, -E, tr, R);
		else                 wtz_lane_global<104>(live, p.qlen, p.q, p.tlen, p.t, p.W, M, X, -I, -E, -D, -E, tr, R);
	} else {
		if(ncmax <= 16)      wtz_lane_fixed<16, false>(live, p.qlen, p.q, p.tlen, p.t, 0, W, ql, tl, M, X, I, D, E, T, tr, R);
		else if(ncmax <= 32) wtz_lane_fixed<32, false>(live, p.qlen, p.q, p.tlen, p.t, 0, W, ql, tl, M, X, I, D, E, T, tr, R);
		else if(ncmax <= 64) wtz_lane_fixed<64, false>(live, p.qlen, p.q, p.tlen, p.t, 0, W, ql, tl, M, X, I, D, E, T, tr, R);
		else                 wtz_lane_fixed<104, false>(live, p.qlen, p.q, p.tlen, p.t, 0, W, ql, tl, M, X, I, D, E, T, tr, R);
	}
	if(live) res[idx] = R;
}
/* second launch: lane l walks the rows lane l wrote; the runs stay in traceback order (the host reverses them) */
template<bool GLOBAL>
WTZ_HD void wtz_task_test_ltb(uint32_t wv, const wtz_dpprob_dev_t *pr, uint32_t n, const wtz_env_t &V, const uint64_t *runoff, uint32_t *runs, wtz_lres_t *res, const uint64_t *wtr, const uint32_t *wrs){
	const uint32_t idx = wv * WTZ_NLANES + WTZ_LANE;
	const uint64_t pa = wtr[wv];
	if(idx >= n || pa == 0) return;
	wtz_lres_t R = res[idx];
	if(!(R.flags & WTZ_LR_DONE)) return;
	const wtz_dpprob_dev_t p = pr[idx];
	const uint32_t *tr = (const uint32_t*)(uintptr_t)pa;      /* lane-interleaved, as the first launch wrote it */
	if(GLOBAL){
		const int32_t r0 = p.tlen - 1, c0 = (r0 + p.W + 1 < p.qlen ? r0 + p.W + 1 : p.qlen) - 1;
		wtz_lane_traceback<true>(true, r0, c0, p.W, wrs[wv], p.t, p.tlen, p.q, p.qlen, tr, runs + runoff[idx], R);
	} else {
		int32_t W, ql, tl, n_col;
		(void)wtz_test_l65_fixed_geo(p, V.P, W, ql, tl, n_col);
		wtz_lane_traceback<false>(true, R.qe - 1, R.te - 1, W, wrs[wv], p.q, p.qlen, p.t, p.tlen, tr, runs + runoff[idx], R);
	}
	res[idx] = R;
}

#ifndef WTZ_EMUL
static __device__ void wtz_testdp_store(wtz_dpres_dev_t *res, const wtz_aln_t &x, bool from_runs, const uint32_t *runs, uint32_t n_runs, const wtz_cigar_t &tmp,
		wtz_pool_t *pool, int form, int bad, unsigned long long cells){
	/* lane 0 only */
	wtz_dpres_dev_t r; memset(&r, 0, sizeof r);
	r.x = x; r.form = form; r.bad = bad; r.cells = cells;
	if(from_runs){
		wtz_cigar_t cg; cg.init(pool, n_runs ? n_runs : 1);
		for(uint32_t k = n_runs; k-- > 0;) cg.push(runs[k]);         /* runs are in traceback order */
		r.cigar = cg.a; r.cigar_len = cg.n; if(cg.bad) r.bad = 1;
	} else { r.cigar = tmp.a; r.cigar_len = tmp.n; if(tmp.bad) r.bad = 1; }
	*res = r;
}

static __device__ void wtz_task_test_fixed(uint32_t t, const wtz_dpprob_dev_t *pr, const wtz_params_t *P, wtz_pool_t *pool, int force, wtz_dpres_dev_t *res){
	const wtz_dpprob_dev_t p = pr[t];
	int32_t *lds = wtz_wave_scratch();
	wtz_wave_lds_t L; L.tb = (uint64_t*)lds; L.Hs = lds + 256; L.Es = lds + 768; L.PM = 511; L.tw = 128; L.qw = (uint32_t*)(lds + WTZ_WINALIGN_LDS_BYTES / 4);        /* the slice of wtz_align_window_wave */
	uint8_t *ztr = (uint8_t*)(lds + 256); const int32_t ztr_bytes = WTZ_WINALIGN_LDS_BYTES - 1024;
	wtz_swmem_t mem; wtz_swmem_init(mem, pool);
	wtz_cigar_t tmp; tmp.init(pool, WTZ_LANE == 0 ? 64 : 0);
	unsigned long long cells = 0;
	wtz_fixres_t R;
	wtz_fixed_problem_wave<true, true>(p.qlen, p.q, p.tlen, p.t, p.init_score, P, L, ztr, ztr_bytes, tmp, mem, pool, &cells, force, R);
	if(WTZ_LANE != 0) return;
	if(R.form < 0){ wtz_dpres_dev_t r; memset(&r, 0, sizeof r); r.form = 0; res[t] = r; return; }
	/* an empty problem is answered in place by every form (score = init, empty CIGAR): report it under the requested name */
	wtz_testdp_store(&res[t], R.y, R.lds_runs, R.runs, R.n_runs, tmp, pool, R.form ? R.form : (force ? force : 1), !R.ok, cells);
}

/* form 64: the lane-per-problem K-sw1 (wtz_sw_lane.h) in ABSOLUTE mode - the reference's function for a known init_score; lane 0 of the wave
 * carries the problem, the other lanes are idle (the product packs 64 problems of one shape class into a wave and runs the relative mode) */
static __device__ void wtz_task_test_lane(uint32_t t, const wtz_dpprob_dev_t *pr, const wtz_params_t *P, wtz_pool_t *pool, wtz_dpres_dev_t *res){
	const wtz_dpprob_dev_t p = pr[t];
	const int32_t M = P->M, X = P->X, I = P->I, D = P->D, E = P->E, T = P->T;
	const int32_t init = p.init_score < 0 ? 0 : p.init_score;
	wtz_dpres_dev_t r; memset(&r, 0, sizeof r);
	if(p.qlen <= 0 || p.tlen <= 0){ r.x.score = init; r.form = 64; if(WTZ_LANE == 0) res[t] = r; return; }
	int32_t W = P->w, ql, tl, n_col;
	wtz_ext_geometry(p.qlen, p.tlen, init, W, M, I, D, E, T, ql, tl, n_col);
	if(n_col > WTZ_LN_MAXCOLS || ql > WTZ_LN_MAXROWS || ql + tl > WTZ_LN_MAXSPAN || init > (1 << 20)){ if(WTZ_LANE == 0) res[t] = r; return; }      /* outside the envelope: declined */
	const uint32_t RS = wtz_lane_rs(n_col);
	unsigned long long pa = 0;
	if(WTZ_LANE == 0) pa = (unsigned long long)(uintptr_t)wtz_pool_alloc(pool, (size_t)ql * RS * 4 * WTZ_NLANES + (size_t)(ql + tl + 4) * 4 + 32);      /* the wave's lane-interleaved trace block (wtz_ltr_at), although only lane 0 has a problem here */
	pa = __shfl(pa, 0, 64);
	if(pa == 0){ r.bad = 1; r.form = 64; if(WTZ_LANE == 0) res[t] = r; return; }
	uint32_t *tr = (uint32_t*)(uintptr_t)pa, *runs = tr + (size_t)ql * RS * WTZ_NLANES + 4;
	const bool live = WTZ_LANE == 0;
	wtz_lres_t R; memset(&R, 0, sizeof R);
	if(n_col <= 16)      wtz_lane_fixed<16, true>(live, p.qlen, p.q, p.tlen, p.t, init, W, ql, tl, M, X, I, D, E, T, tr, R);
	else if(n_col <= 32) wtz_lane_fixed<32, true>(live, p.qlen, p.q, p.tlen, p.t, init, W, ql, tl, M, X, I, D, E, T, tr, R);
	else if(n_col <= 64) wtz_lane_fixed<64, true>(live, p.qlen, p.q, p.tlen, p.t, init, W, ql, tl, M, X, I, D, E, T, tr, R);
	else                 wtz_lane_fixed<104, true>(live, p.qlen, p.q, p.tlen, p.t, init, W, ql, tl, M, X, I, D, E, T, tr, R);
	if(!live) return;
	wtz_lane_traceback<false>(true, R.qe - 1, R.te - 1, W, RS, p.q, p.qlen, p.t, p.tlen, tr, runs, R);
	wtz_aln_t x; memset(&x, 0, sizeof x);
	x.score = R.score; x.qe = R.qe; x.te = R.te; x.mat = R.mat; x.mis = R.mis; x.ins = R.ins; x.del = R.del; x.aln = R.mat + R.mis + R.ins + R.del;
	wtz_cigar_t none; none.a = NULL; none.n = none.cap = 0; none.pool = pool; none.bad = 0;
	wtz_testdp_store(&res[t], x, true, runs, R.n_runs, none, pool, 64, 0, R.cells);
}

/* form 64 of WTZ_DP_GLOBAL: the lane-per-gap K-sw2 (wtz_lane_global) at the band width the problem names */
static __device__ void wtz_task_test_lane_global(uint32_t t, const wtz_dpprob_dev_t *pr, const wtz_params_t *P, wtz_pool_t *pool, wtz_dpres_dev_t *res){
	const wtz_dpprob_dev_t p = pr[t];
	const int32_t M = P->M, X = P->X, I = P->I, D = P->D, E = P->E;
	wtz_dpres_dev_t r; memset(&r, 0, sizeof r);
	const int32_t w = p.W, n_col = p.qlen < 2 * w + 1 ? p.qlen : 2 * w + 1;
	if(p.qlen <= 0 || p.tlen <= 0 || WTZ_ABSDIFF(p.qlen, p.tlen) > w || n_col > WTZ_LN_MAXCOLS || p.tlen > WTZ_LG_MAXROWS){ if(WTZ_LANE == 0) res[t] = r; return; }     /* declined */
	const uint32_t RS = wtz_lane_rs(n_col);
	unsigned long long pa = 0;
	if(WTZ_LANE == 0) pa = (unsigned long long)(uintptr_t)wtz_pool_alloc(pool, (size_t)p.tlen * RS * 4 * WTZ_NLANES + (size_t)(p.qlen + p.tlen + 4) * 4 + 32);
	pa = __shfl(pa, 0, 64);
	if(pa == 0){ r.bad = 1; r.form = 64; if(WTZ_LANE == 0) res[t] = r; return; }
	uint32_t *tr = (uint32_t*)(uintptr_t)pa, *runs = tr + (size_t)p.tlen * RS * WTZ_NLANES + 4;
	const bool live = WTZ_LANE == 0;
	wtz_lres_t R; memset(&R, 0, sizeof R);
	if(n_col <= 16)      wtz_lane_global<16>(live, p.qlen, p.q, p.tlen, p.t, w, M, X, -I, -E, -D, -E, tr, R);
	else if(n_col <= 32) wtz_lane_global<32>(live, p.qlen, p.q, p.tlen, p.t, w, M, X, -I, -E, -D, -E, tr, R);
	else if(n_col <= 64) wtz_lane_global<64>(live, p.qlen, p.q, p.tlen, p.t, w, M, X, -I, -E, -D, -E, tr, R);
	else                 wtz_lane_global<104>(live, p.qlen, p.q, p.tlen, p.t, w, M, X, -I, -E, -D, -E, tr, R);
	if(!live) return;
	{ const int32_t r0 = p.tlen - 1, c0 = (r0 + w + 1 < p.qlen ? r0 + w + 1 : p.qlen) - 1; wtz_lane_traceback<true>(true, r0, c0, w, RS, p.t, p.tlen, p.q, p.qlen, tr, runs, R); }
	wtz_aln_t x; memset(&x, 0, sizeof x);
	x.score = R.score; x.mat = R.mat; x.mis = R.mis; x.ins = R.ins; x.del = R.del; x.aln = R.mat + R.mis + R.ins + R.del;
	wtz_cigar_t none; none.a = NULL; none.n = none.cap = 0; none.pool = pool; none.bad = 0;
	wtz_testdp_store(&res[t], x, true, runs, R.n_runs, none, pool, 64, 0, R.cells);
}

static __device__ void wtz_task_test_global(uint32_t t, const wtz_dpprob_dev_t *pr, const wtz_params_t *P, wtz_pool_t *pool, int force, uint32_t wide_lds, wtz_dpres_dev_t *res){
#if defined(__HIP_DEVICE_COMPILE__)
	const wtz_dpprob_dev_t p = pr[t];
	int32_t *lds = wtz_wave_scratch();
	wtz_trace_t tr; tr.chunk = NULL; tr.zb = NULL; tr.n_chunk = 0; tr.zrow = 0; tr.cap_rows = 0;
	wtz_swmem_t mem; wtz_swmem_init(mem, pool);
	wtz_cigar_t tmp; tmp.init(pool, WTZ_LANE == 0 ? 32 : 0);
	wtz_gapdp_t G;
	wtz_gap_problem_wave<true>(p.qlen, p.q, p.tlen, p.t, P, p.W, lds, wide_lds, false, pool, tmp, tr, mem, force == 33 ? WTZ_FORM_RING : force, G);
	if(WTZ_LANE != 0) return;
	if(G.form < 0){ wtz_dpres_dev_t r; memset(&r, 0, sizeof r); r.form = 0; res[t] = r; return; }
	wtz_aln_t x; memset(&x, 0, sizeof x); x.score = G.score;
	if(G.from_reg){
		x.mat = G.r_mat; x.mis = G.r_mis;
		for(uint32_t k = 0; k < G.n_runs; k++){ const uint32_t r = G.runs[k], op = r & 0xFu; const int32_t len = (int32_t)(r >> 4); x.aln += len; if(op == 1) x.ins += len; else if(op == 2) x.del += len; }
	} else {        /* the fold of wtz_task_gap over a CIGAR that came without counts */
		int32_t x1 = 0, x2 = 0;
		for(uint32_t idx = 0; idx < tmp.n; idx++){
			const int32_t op = (int32_t)(tmp.a[idx] & 0xF), len = (int32_t)(tmp.a[idx] >> 4);
			x.aln += len;
			if(op == 0){ for(int32_t j = 0; j < len; j++){ if(p.q.at(x1 + j) == p.t.at(x2 + j)) x.mat++; else x.mis++; } x1 += len; x2 += len; }
			else if(op == 1){ x1 += len; x.ins += len; }
			else if(op == 2){ x2 += len; x.del += len; }
		}
	}
	wtz_testdp_store(&res[t], x, G.from_reg, G.runs, G.n_runs, tmp, pool, (G.form == WTZ_FORM_RING && force == 33) ? 33 : G.form, G.bad, 0);
#endif
}
#endif

/* form 65 of WTZ_DP_FIXED / WTZ_DP_GLOBAL, both back ends: the two launches, then the fold's rule per K-sw1 problem */
static int test_dp_lanes(wtz_ctx_t *c, int32_t kind, const wtz_dp_problem_t *pr, uint32_t n, wtz_dp_result_t *out, uint32_t *cigar, uint64_t cigar_cap){
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	std::vector<wtz_dpprob_dev_t> hp(n);
	std::vector<uint64_t> h_ro((size_t)n + 1, 0);      /* room for the runs of problem i: at most one per row and column, as the planners size it */
	for(uint32_t i = 0; i < n; i++){
		const wtz_dp_problem_t &p = pr[i];
		wtz_dpprob_dev_t d; CHK(dp_problem_views(c, h_off, p, i, true, 0, &d.q, &d.t)); d.qlen = p.q_len; d.tlen = p.t_len; d.init_score = p.init_score; d.W = p.W;
		hp[i] = d; h_ro[i + 1] = h_ro[i] + (uint64_t)(p.q_len > 0 ? p.q_len : 0) + (uint64_t)(p.t_len > 0 ? p.t_len : 0) + 4u;
	}
	const wtz_env_t V = ctx_env(c);
	const uint32_t nw = (uint32_t)(((uint64_t)n + WTZ_NLANES - 1) / WTZ_NLANES);
	wtz_dpprob_dev_t *d_pr = NULL; wtz_lres_t *d_res = NULL; uint64_t *d_ro = NULL, *d_wtr = NULL; uint32_t *d_runs = NULL, *d_wrs = NULL;
	CHK(batch_upload(hp, std::vector<uint32_t>(), &d_pr, (uint32_t**)NULL, &d_res));
	CHK(dev_alloc((void**)&d_ro, ((size_t)n + 1) * 8)); CHK(dev_h2d(d_ro, h_ro.data(), ((size_t)n + 1) * 8));
	CHK(dev_alloc((void**)&d_runs, (size_t)h_ro[n] * 4));
	CHK(dev_alloc((void**)&d_wtr, (size_t)nw * 8)); CHK(dev_set(d_wtr, 0, (size_t)nw * 8));
	CHK(dev_alloc((void**)&d_wrs, (size_t)nw * 4)); CHK(dev_set(d_wrs, 0, (size_t)nw * 4));
	if(kind == WTZ_DP_FIXED){
		CHK(wtz_launch_coop<K_test_ldp>(nw, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_ldp<false>((uint32_t)t, d_pr, n, V, d_res, d_wtr, d_wrs); }, 0));
		CHK(wtz_launch_coop<K_test_ltb>(nw, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_ltb<false>((uint32_t)t, d_pr, n, V, d_ro, d_runs, d_res, d_wtr, d_wrs); }, 0));
	} else {
		CHK(wtz_launch_coop<K_test_ldp>(nw, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_ldp<true>((uint32_t)t, d_pr, n, V, d_res, d_wtr, d_wrs); }, 0));
		CHK(wtz_launch_coop<K_test_ltb>(nw, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_ltb<true>((uint32_t)t, d_pr, n, V, d_ro, d_runs, d_res, d_wtr, d_wrs); }, 0));
	}
	CHK(dev_sync());
	CHK(tpool_check(c, "wtz_test_dp"));
	CHK(pool_check(c, "wtz_test_dp"));
	std::vector<wtz_lres_t> hr(n); std::vector<uint32_t> h_runs((size_t)h_ro[n]);
	CHK(dev_d2h(hr.data(), d_res, (size_t)n * sizeof(wtz_lres_t)));
	CHK(dev_d2h(h_runs.data(), d_runs, (size_t)h_ro[n] * 4));
	uint64_t off = 0;
	for(uint32_t i = 0; i < n; i++){
		const wtz_lres_t &r = hr[i];
		wtz_dp_result_t o; memset(&o, 0, sizeof o);
		const int32_t a = pr[i].init_score < 0 ? 0 : pr[i].init_score;                 /* kswx.h:241 */
		const bool answered = (r.flags & WTZ_LR_DONE) && (kind == WTZ_DP_GLOBAL || !wtz_lres_declined(a, r));
		if(answered){
			if(r.n_runs > h_ro[i + 1] - h_ro[i]) return wtz_fail(WTZ_E_STATE, "wtz_test_dp: problem %u wrote %u runs into room for %llu", i, r.n_runs, (unsigned long long)(h_ro[i + 1] - h_ro[i]));
			o.score = kind == WTZ_DP_GLOBAL ? r.score : a + r.score;
			if(kind == WTZ_DP_FIXED){ o.qe = r.qe; o.te = r.te; }
			o.mat = r.mat; o.mis = r.mis; o.ins = r.ins; o.del = r.del; o.aln = r.mat + r.mis + r.ins + r.del;
			o.form_used = 65; o.cigar_len = r.n_runs; o.cigar_off = off; o.cells = r.cells;
			if(off + r.n_runs > cigar_cap) return wtz_fail(WTZ_E_ARG, "wtz_test_dp: CIGAR buffer too small");
			for(uint32_t k = 0; k < r.n_runs; k++) cigar[off + k] = h_runs[(size_t)h_ro[i] + r.n_runs - 1 - k];      /* traceback order -> CIGAR order */
			off += r.n_runs;
		}
		out[i] = o;
	}
	return WTZ_OK;
}

extern "C" int wtz_test_dp(wtz_ctx_t *c, int32_t kind, int32_t form, const wtz_dp_problem_t *pr, uint32_t n, wtz_dp_result_t *out, uint32_t *cigar, uint64_t cigar_cap){
	BATCH_ARGS(c, n, pr && out && (cigar || !cigar_cap), NULL, NULL);
	if((kind == WTZ_DP_FIXED || kind == WTZ_DP_GLOBAL) && form == 65) return test_dp_lanes(c, kind, pr, n, out, cigar, cigar_cap);
#ifdef WTZ_EMUL
	/* beside form 65 (above) the host emulation has the scalar bodies only -WTZ_DP_SHIFT 4, WTZ_DP_FIXED / WTZ_DP_GLOBAL 255 -, called as the device's scalar forms call them */
	if(!((kind == WTZ_DP_SHIFT && form == 4) || ((kind == WTZ_DP_FIXED || kind == WTZ_DP_GLOBAL) && form == 255)))
		return wtz_fail(WTZ_E_STATE, "wtz_test_dp drives the DEVICE forms of the banded DPs: it needs the HIP build");
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	const wtz_params_t *P = c->dP; wtz_pool_t *pool = c->dpool;
	uint64_t off = 0;
	for(uint32_t i = 0; i < n; i++){
		const wtz_dp_problem_t &p = pr[i];
		wtz_seq_packed q, t; CHK(dp_problem_views(c, h_off, p, i, true, 0, &q, &t));
		wtz_swmem_t mem; wtz_swmem_init(mem, pool);
		wtz_cigar_t cg; cg.init(pool, 64);
		wtz_aln_t x; memset(&x, 0, sizeof x);
		unsigned long long cells = 0;
		if(kind == WTZ_DP_SHIFT) x = wtz_extend_shift(p.q_len, q, p.t_len, t, p.init_score, p.W, P->M, P->X, P->I, P->D, P->E, P->T, mem, cg, &cells);
		else if(kind == WTZ_DP_FIXED) x = wtz_extend_fixed(p.q_len, q, p.t_len, t, p.init_score, P->w, P->M, P->X, P->I, P->D, P->E, P->T, mem, cg);
		else {
			x.score = wtz_global_banded(p.q_len, q, p.t_len, t, P->M, P->X, -P->I, -P->E, -P->D, -P->E, p.W, mem, cg);      /* hzm_aln.h:1407 */
			int32_t x1 = 0, x2 = 0;
			for(uint32_t k = 0; k < cg.n; k++){      /* the fold of wtz_task_gap */
				const int32_t op = (int32_t)(cg.a[k] & 0xF), len = (int32_t)(cg.a[k] >> 4);
				x.aln += len;
				if(op == 0){ for(int32_t j = 0; j < len; j++){ if(q.at(x1 + j) == t.at(x2 + j)) x.mat++; else x.mis++; } x1 += len; x2 += len; }
				else if(op == 1){ x1 += len; x.ins += len; }
				else { x2 += len; x.del += len; }
			}
		}
		if(mem.bad || cg.bad) return wtz_fail(WTZ_E_POOL, "wtz_test_dp: problem %u ran out of scratch", i);
		wtz_dp_result_t o; memset(&o, 0, sizeof o);
		o.score = x.score; o.tb = x.tb; o.te = x.te; o.qb = x.qb; o.qe = x.qe; o.aln = x.aln; o.mat = x.mat; o.mis = x.mis; o.ins = x.ins; o.del = x.del;
		o.form_used = (uint32_t)form; o.cigar_len = cg.n; o.cigar_off = off; o.cells = cells;
		if(off + cg.n > cigar_cap) return wtz_fail(WTZ_E_ARG, "wtz_test_dp: CIGAR buffer too small");
		if(cg.n) memcpy(cigar + off, cg.a, (size_t)cg.n * 4);
		off += cg.n;
		out[i] = o;
		CHK(pool_reset(c));      /* one problem at a time: its scratch goes back */
	}
	return WTZ_OK;
#else
	CTX_ENTER(c);
	std::vector<uint64_t> h_off; CHK(batch_begin(c, h_off));
	std::vector<wtz_dpprob_dev_t> hp(n);
	for(uint32_t i = 0; i < n; i++){
		const wtz_dp_problem_t &p = pr[i];
		wtz_dpprob_dev_t d; CHK(dp_problem_views(c, h_off, p, i, true, 0, &d.q, &d.t)); d.qlen = p.q_len; d.tlen = p.t_len; d.init_score = p.init_score; d.W = p.W;
		hp[i] = d;
	}
	const wtz_env_t V = ctx_env(c);
	std::vector<wtz_dpres_dev_t> hr(n);
	if(kind == WTZ_DP_SHIFT){
		std::vector<wtz_extjob_t> jobs(n);
		for(uint32_t i = 0; i < n; i++){ wtz_extjob_t j; memset(&j, 0, sizeof j); j.q = hp[i].q; j.t = hp[i].t; j.qlen = hp[i].qlen; j.tlen = hp[i].tlen; j.init_score = hp[i].init_score; j.W = hp[i].W; j.item = i; j.valid = 1; jobs[i] = j; }
		wtz_extjob_t *d_jobs = NULL; CHK(dev_alloc((void**)&d_jobs, (size_t)n * sizeof(wtz_extjob_t))); CHK(dev_h2d(d_jobs, jobs.data(), (size_t)n * sizeof(wtz_extjob_t)));
		wtz_timer tform; tform.start();      /* the forced forms report their launch time through counters.ms_ext too (tools/ubench/ksw3_bench.py) */
		if(form == 0){ CHK(run_extjobs(c, V, d_jobs, n)); }
		else if(form == 3){ WTZ_LAUNCH((wtz_kernel_extjobs<2048, 1032>), n, 64, 0, g_stream, d_jobs, (const uint32_t*)NULL, n, V.P, V.pool, V.pool + 1); }
		else if(form == 4){ CHK(wtz_launch_wave<K_extjob_scalar>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_extjob_scalar((uint32_t)t, V, d_jobs); })); }
		else if(form == 5){ WTZ_LAUNCH_SP(c, wtz_kernel_extjobs_fr, 1032, n, 64, 0, g_stream, d_jobs, (const uint32_t*)NULL, n, V.P, V.pool, V.pool + 1); }
		else if(form == 7){ WTZ_LAUNCH_SP(c, wtz_kernel_extjobs_pk, 1032, n, 64, 0, g_stream, d_jobs, (const uint32_t*)NULL, n, V.P, V.pool, V.pool + 1); }      /* frame form, two 16-bit cells per register (round 6) */
		else return wtz_fail(WTZ_E_ARG, "WTZ_DP_SHIFT: unknown form %d", form);      /* 1, 2 and 6 were kernels that have been removed: their numbers are not reused */
		CHK(dev_sync());
		if(form != 0){ c->cnt.ms_ext += tform.stop(); c->cnt.n_extjobs += n; }
		CHK(tpool_check(c, "wtz_test_dp"));
		CHK(dev_d2h(jobs.data(), d_jobs, (size_t)n * sizeof(wtz_extjob_t)));
		for(uint32_t i = 0; i < n; i++){
			wtz_dpres_dev_t r; memset(&r, 0, sizeof r);
			const int done = form == 4 ? 4 : (int)jobs[i].done;
			const bool empty = jobs[i].qlen <= 0 || jobs[i].tlen <= 0;
			/* the register kernels leave empty problems (and what is outside their envelope) to the general kernel */
			if(done || (form == 0) || (form == 3 && empty)){ r.x = jobs[i].x; r.cigar = jobs[i].cigar; r.cigar_len = jobs[i].cigar_len; r.form = done ? done : 3; r.bad = jobs[i].bad; r.cells = jobs[i].cells; }
			hr[i] = r;
		}
	} else if(kind == WTZ_DP_FIXED || kind == WTZ_DP_GLOBAL){
		wtz_dpprob_dev_t *d_pr = NULL; wtz_dpres_dev_t *d_res = NULL;
		CHK(batch_upload(hp, std::vector<uint32_t>(), &d_pr, (uint32_t**)NULL, &d_res));
		const wtz_params_t *dP = c->dP; wtz_pool_t *pool = c->dpool;
		if(kind == WTZ_DP_FIXED && form == 64){
			CHK(wtz_launch_coop<K_test_lane>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_lane((uint32_t)t, d_pr, dP, pool, d_res); }, 0));
		} else if(kind == WTZ_DP_FIXED){
			CHK(wtz_launch_coop<K_test_fixed>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_fixed((uint32_t)t, d_pr, dP, pool, form, d_res); }, WTZ_WINALIGN_LDS_BYTES + WTZ_WINALIGN_QW_BYTES));
		} else if(form == 64){
			CHK(wtz_launch_coop<K_test_lane>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_lane_global((uint32_t)t, d_pr, dP, pool, d_res); }, 0));
		} else if(form == 33){
			CHK(wtz_launch_coop<K_test_global_wide>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_global((uint32_t)t, d_pr, dP, pool, form, (uint32_t)WTZ_GAP_WIDE_LDS_BYTES, d_res); }, WTZ_GAP_WIDE_LDS_BYTES));
		} else {
			CHK(wtz_launch_coop<K_test_global>(n, [=] WTZ_LAMBDA (uint64_t t){ wtz_task_test_global((uint32_t)t, d_pr, dP, pool, form, 0u, d_res); }, WTZ_GAP_LDS_BYTES));
		}
		CHK(dev_sync());
		CHK(dev_d2h(hr.data(), d_res, (size_t)n * sizeof(wtz_dpres_dev_t)));
	} else return wtz_fail(WTZ_E_ARG, "unknown DP kind %d", kind);
	CHK(pool_check(c, "wtz_test_dp"));
	uint64_t off = 0;
	for(uint32_t i = 0; i < n; i++){
		const wtz_dpres_dev_t &r = hr[i];
		if(r.bad) return wtz_fail(WTZ_E_POOL, "wtz_test_dp: problem %u ran out of scratch", i);
		wtz_dp_result_t o; memset(&o, 0, sizeof o);
		o.form_used = (uint32_t)r.form;
		if(r.form){
			o.score = r.x.score; o.tb = r.x.tb; o.te = r.x.te; o.qb = r.x.qb; o.qe = r.x.qe; o.aln = r.x.aln; o.mat = r.x.mat; o.mis = r.x.mis; o.ins = r.x.ins; o.del = r.x.del;
			o.cigar_len = r.cigar_len; o.cigar_off = off; o.cells = r.cells;
			if(off + r.cigar_len > cigar_cap) return wtz_fail(WTZ_E_ARG, "wtz_test_dp: CIGAR buffer too small");
			if(r.cigar_len) CHK(dev_d2h(cigar + off, r.cigar, (size_t)r.cigar_len * 4));
			off += r.cigar_len;
		}
		out[i] = o;
	}
	return WTZ_OK;
#endif
}
#endif
