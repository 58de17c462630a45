/*
 * wtz_sw_fixed.h — K-sw1, kswx_extend_align_core (kswx.h:234-335: fixed band around the diagonal), and the window alignment built on it,
 * one 64-lane wavefront per problem:
 *     wtz_walk_step / wtz_walk_finish   the branch-free traceback step of lane 0 (kswx.h:309-333);
 *     wtz_extend_fixed_reg<C, ZG>       the register form: C band columns per lane, 4-bit trace in LDS or (ZG) in the pool;
 *     wtz_align_zmer_w                  hz_align_hzmo (hzm_aln.h:278-314) over register-resident sequences;
 *     wtz_fixed_problem_wave            picks the form of one problem from its shape (or the form a test forces);
 *     wtz_align_window_wave             the anchor loop of a window (hzm_aln.h:1247-1302) with its K-sw1 gaps on the wave.
 * Semantics reproduced exactly: -10000 sentinels outside the band, H(i,-1)/H(-1,j) boundary values, the LAST arg-max of a row
 * (kswx.h:288-289), gmax/max end rule with T, early exit when a row maximum is <= 0.
 */
#ifndef WTZ_SW_FIXED_H
#define WTZ_SW_FIXED_H

#include "wtz_wave.h"

#ifndef WTZ_WINALIGN_LDS_BYTES
#define WTZ_WINALIGN_LDS_BYTES 12288     /* LDS slice of a window-alignment wave (measured best with 3 waves/SIMD) */
#endif
#ifndef WTZ_WINALIGN_QW_BYTES
#define WTZ_WINALIGN_QW_BYTES 512       /* behind the slice: the query of the current K-sw1 problem as 2-bit words, for its traceback */
#endif

#ifdef __HIPCC__

/*
 * K-sw1 for the small problems between two anchors of a window (80 % have a band of <= 64 columns, 96 % <= 128 rows):
 * the whole DP state lives in registers.  Lane l owns the C band-relative columns l*C .. l*C+C-1; the fixed band moves
 * right by exactly one column per row once i > W, so the hand-over between rows is a register rotation plus one
 * wave_shl DPP per array (no LDS rings).  The query is staged as 32-base words in VGPRs (the row's base comes from a
 * v_readlane), the target as 32-base words in LDS; the trace is kept in LDS at 4 bits per cell (two rows per byte), so
 * the traceback of lane 0 never leaves the CU.  Results are those of kswx_extend_align_core (the scalar body wtz_extend_fixed states them on the device).
 * Requirements (checked by the caller): n_col <= 64*C, ((ql+1)/2)*64*C <= ztr_bytes, (tl+63)/32+1 <= tb words, ql <= 2048.
 */

/* one step of the K-sw1 / kswx traceback on lane 0, written without branches (the branchy form spent its time in exec-mask
 * bookkeeping and taken branches, not in arithmetic): next state from the cell's nibble, base equality from the 2-bit words of
 * both sequences in LDS (read whether the step is diagonal or not), counters and cursor by flag arithmetic; the open run is kept
 * in runs[nr] and simply rewritten every step. */
typedef struct { int32_t i, j; uint32_t d, run_op, run_len, nr; int32_t ndiag, mis, i0, j0; } wtz_walk_t;      /* i0, j0: where the walk started */
WTZ_D void wtz_walk_step(wtz_walk_t &w, uint32_t nib, const uint32_t *qw32, const uint32_t *tb32, uint32_t *runs){
	const uint32_t h3 = nib & 3u, h = h3 > 2u ? 2u : h3;
	const uint32_t d = ((h | (nib & 4u) | ((nib & 8u) << 2)) >> (w.d << 1)) & 3u;      /* bits 1:0 move from H, 3:2 from E (0 / 1), 5:4 from F (0 / 2) */
	const uint32_t qb = (qw32[w.i >> 4] >> ((w.i & 15) * 2)) & 3u, tq = (tb32[w.j >> 4] >> ((w.j & 15) * 2)) & 3u;
	const uint32_t isd = d == 0 ? 1u : 0u, ne = qb != tq ? 1u : 0u;
	w.ndiag += (int32_t)isd; w.mis += (int32_t)(isd & ne);          /* insertions / deletions follow from the distance walked (wtz_walk_finish) */
	w.i -= d != 2 ? 1 : 0; w.j -= d != 1 ? 1 : 0;
	const bool same = d == w.run_op;
	w.nr += (!same && w.run_len) ? 1u : 0u;
	w.run_len = same ? w.run_len + 1u : 1u; w.run_op = d; w.d = d;
	runs[w.nr] = (w.run_len << 4) | d;
}
/* the two leading gaps (kswx.h:321-322) merge with the open run when the operation agrees (kswx_push_cigar); closes the list */
WTZ_D void wtz_walk_finish(wtz_walk_t &w, wtz_aln_t &x, uint32_t *runs, uint32_t *n_runs){
	uint32_t run_op = w.run_op, run_len = w.run_len, nr = w.nr;
	x.mat = w.ndiag - w.mis; x.mis = w.mis; x.ins = (w.i0 - w.i) - w.ndiag; x.del = (w.j0 - w.j) - w.ndiag;      /* every step but a deletion moves up, every step but an insertion moves left */
	if(w.i >= 0){ x.ins += w.i + 1; if(run_len && run_op == 1u) run_len += (uint32_t)(w.i + 1); else { if(run_len) runs[nr++] = (run_len << 4) | run_op; run_op = 1u; run_len = (uint32_t)(w.i + 1); } }
	if(w.j >= 0){ x.del += w.j + 1; if(run_len && run_op == 2u) run_len += (uint32_t)(w.j + 1); else { if(run_len) runs[nr++] = (run_len << 4) | run_op; run_op = 2u; run_len = (uint32_t)(w.j + 1); } }
	if(run_len) runs[nr++] = (run_len << 4) | run_op;
	*n_runs = nr;                              /* in traceback order: the caller replays them backwards */
	x.aln = x.mat + x.mis + x.ins + x.del; x.qe++; x.te++;
}

/* ZG: the trace does not fit LDS and lives in the pool (HBM): the rows store it through a global-address-space pointer (one
 * contiguous zrow-byte piece per row pair), the traceback walks LDS-staged blocks of 64 DP rows x the whole band (`stage`, 4 KB) */
template<int C, bool ZG = false>
WTZ_D wtz_aln_t wtz_extend_fixed_reg(int32_t qlen, const wtz_seq_packed &query, int32_t tlen, const wtz_seq_packed &target, int32_t init_score,
		int32_t ql, int32_t tl, int32_t W, int32_t M, int32_t X, int32_t I, int32_t D, int32_t E, int32_t T,
		uint64_t *tb, uint32_t *qlds, uint8_t *ztr, uint32_t zrow, uint32_t *runs, uint32_t *n_runs, unsigned long long *cells, uint8_t *stage = NULL){
	const int lane = (int)(threadIdx.x & 63);
	constexpr int KB = C <= 2 ? 7 : 9;           /* bits of the band column inside the packed arg-max key (callers check |h| < 2^(31-KB)) */
	wtz_aln_t x; memset(&x, 0, sizeof x);
	*n_runs = 0;
	if(init_score < 0) init_score = 0;
	const unsigned long long pt_stage = WTZ_PROF_T();
	/* ---- stage both sequences ---- */
	{
		const int32_t nw = (tl + 31) / 32 + 1;
		for(int32_t w = lane; w < nw; w += 64) tb[w] = wtz_pack32(target, w * 32, tl);
	}
	const uint64_t qw = wtz_pack32(query, lane * 32, ql);
	const uint32_t qw_lo = (uint32_t)qw, qw_hi = (uint32_t)(qw >> 32);
	((uint64_t*)qlds)[lane] = qw;                    /* for the traceback: base i is bits 2*(i&15) of word i>>4 */
	__threadfence_block();
	WTZ_PROF_ADD(5, pt_stage);
	const unsigned long long pt_rows = WTZ_PROF_T();
	/* The row loop is written for instruction count: every cell update is branch-free (max / compare-select), the row
	 * maximum and its LAST arg-max come out of ONE integer max-reduction over packed keys h*128 + band column (the caller
	 * guarantees |h| < 2^23), the lane's target bases sit in a 16-base register window that is shifted once per row and
	 * refilled from LDS every 16-C rows, and the row's query base is scalar. */
	int32_t hp[C], ep[C]; uint32_t nibp[C];
	#pragma unroll
	for(int k = 0; k < C; k++){ hp[k] = -10000; ep[k] = -10000; nibp[k] = 0; }
	int32_t mx = init_score, mi = -1, mj = -1, gmax = 0, gi = -1, gj = -1;
	int32_t jbp = 0, i, i_done = -1;
	unsigned long long ncell = 0;
	const int32_t CE = C * E, IE = I + E, DE = D + E;
	const uint32_t *tb32 = (const uint32_t*)tb;
	uint32_t tw = 0; int32_t tw_left = 0; uint32_t qcur = 0;
	const int32_t colrel0 = lane * C;
	for(i = 0; i < ql; i++){
		int32_t jb = i - W; if(jb < 0) jb = 0;
		int32_t je = i + W + 1; if(je > tl) je = tl;
		if((i & 15) == 0){
			const int32_t qs = __builtin_amdgcn_readfirstlane(i >> 5);
			qcur = (i & 16) ? (uint32_t)__builtin_amdgcn_readlane((int)qw_hi, qs) : (uint32_t)__builtin_amdgcn_readlane((int)qw_lo, qs);
		}
		const uint32_t qbase = (qcur >> ((i & 15) * 2)) & 3u;
		const int32_t j0 = jb + colrel0;
		const bool moved = (i > 0) && (jb != jbp);
		if(moved){ tw >>= 2; tw_left--; }
		if(i == 0 || tw_left < C){
			const int32_t jj = j0 < tl ? j0 : (tl > 0 ? tl - 1 : 0);
			const uint32_t lo = tb32[jj >> 4], hi = tb32[(jj >> 4) + 1];
			tw = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(jj & 15) * 2u);
			tw_left = 16;
		}
		/* ---- predecessors from the previous row's registers ---- */
		int32_t pred[C], ein[C];
		if(i == 0){
			#pragma unroll
			for(int k = 0; k < C; k++){ const int32_t j = j0 + k; pred[k] = (j == 0) ? init_score : init_score + D + E * j; ein[k] = -10000; }     /* rh[] / re[] initialisation, kswx.h:143-146 */
		} else if(moved){                     /* band moved right by one: H(i-1,j-1) is the lane's own column, E(i-1,j) the next one */
			const int32_t nxt = wtz_dpp_wave_shl1(-10000, ep[0]);
			#pragma unroll
			for(int k = 0; k < C; k++){ pred[k] = hp[k]; ein[k] = (k + 1 < C) ? ep[k + 1] : nxt; }
		} else {                              /* band still starts at column 0 */
			int32_t prv = wtz_dpp_wave_shr1(-10000, hp[C - 1]);
			prv = (lane == 0) ? init_score + I + E * i : prv;           /* H(i-1,-1), kswx.h:262 */
			#pragma unroll
			for(int k = 0; k < C; k++){ pred[k] = k ? hp[k - 1] : prv; ein[k] = ep[k]; }
		}
		/* ---- m and the lane's F aggregate ---- */
		int32_t mv[C]; bool valid[C]; int32_t agg = -0x3FFFFFFF;
		#pragma unroll
		for(int k = 0; k < C; k++){
			const uint32_t tbase = (tw >> (2 * k)) & 3u;
			mv[k] = pred[k] + ((qbase == tbase) ? M : X);
			valid[k] = (j0 + k < je);
			const int32_t cand = mv[k] + DE + (C - 1 - k) * E;
			agg = (valid[k] && cand > agg) ? cand : agg;
		}
		int32_t f = wtz_f_carry(agg, lane, CE, -0x3FFFFFFF, -10000);
		/* ---- H, E', F, trace nibble ---- */
		int32_t key = (int32_t)0x80000000;
		#pragma unroll
		for(int k = 0; k < C; k++){
			const int32_t m = mv[k], e = ein[k];
			const int32_t h0 = m > e ? m : e;
			const int32_t te = m + IE, e2 = e + E, tf = m + DE, f2 = f + E;
			/* the four decisions as sign bits of differences (|values| < 2^23: no overflow), shifted in with v_alignbit instead of four
			 * compare + select pairs: bit 0 m < e, bit 1 max(m,e) < f, bit 2 E extended, bit 3 F extended; the walker reads the move
			 * from H as min(bits 1:0, 2) */
			uint32_t nib = (uint32_t)(tf - f2) >> 31;
			nib = __builtin_amdgcn_alignbit(nib, (uint32_t)(te - e2), 31);
			nib = __builtin_amdgcn_alignbit(nib, (uint32_t)(h0 - f), 31);
			nib = __builtin_amdgcn_alignbit(nib, (uint32_t)(m - e), 31);
			const int32_t h = h0 > f ? h0 : f;
			const int32_t en = e2 > te ? e2 : te;
			f = f2 > tf ? f2 : tf;
			hp[k] = valid[k] ? h : -10000; ep[k] = valid[k] ? en : -10000;
			nib = valid[k] ? nib : 0u;
			const int32_t kk = h * (1 << KB) + (colrel0 + k);
			key = (valid[k] && kk > key) ? kk : key;
			if(i & 1){
				if((uint32_t)(colrel0 + k) < zrow){
					if(ZG) wtz_as_global(ztr)[(size_t)(i >> 1) * zrow + colrel0 + k] = (uint8_t)(nibp[k] | (nib << 4));
					else ztr[(size_t)(i >> 1) * zrow + colrel0 + k] = (uint8_t)(nibp[k] | (nib << 4));
				}
			}
			else nibp[k] = nib;
		}
		i_done = i;
		ncell += (unsigned long long)(je - jb);
		key = wtz_wave_max_i32(key);
		int32_t imax = 0, mj2 = -1;
		if((key >> KB) >= 0){ imax = key >> KB; mj2 = jb + (key & ((1 << KB) - 1)); }           /* last j with h >= running max >= 0, kswx.h:288-289 */
		if(je == tlen){
			const int32_t idx = je - 1 - jb;
			int32_t hsel = hp[0];
			#pragma unroll
			for(int k = 1; k < C; k++) hsel = (idx % C == k) ? hp[k] : hsel;
			const int32_t h1 = __builtin_amdgcn_readlane(hsel, __builtin_amdgcn_readfirstlane(idx / C));      /* H(i, je-1) */
			if(gmax < h1){ gmax = h1; gi = i; gj = je - 1; }
		}
		if(i + 1 == qlen && gmax < imax){ gmax = imax; gi = i; gj = mj2; }
		jbp = jb;
		if(imax > mx){ mx = imax; mi = i; mj = mj2; }
		else if(imax <= 0) break;
	}
	if(i_done >= 0 && !(i_done & 1)){          /* the last row was the first of its byte pair */
		#pragma unroll
		for(int k = 0; k < C; k++) if((uint32_t)(lane * C + k) < zrow) ztr[(size_t)(i_done >> 1) * zrow + lane * C + k] = (uint8_t)nibp[k];
	}
	if(cells && lane == 0) *cells += ncell;
	if(gmax > 0 && gmax >= mx + T){ x.score = gmax; x.qe = gi; x.te = gj; }
	else { x.score = mx; x.qe = mi; x.te = mj; }
	__threadfence_block();
	WTZ_PROF_ADD(2, pt_rows);
	WTZ_PROF_CNT(4, i_done + 1);
	const unsigned long long pt_tb = WTZ_PROF_T();
	wtz_walk_t wk; wk.i = x.qe; wk.j = x.te; wk.d = 0; wk.run_op = 0xFFu; wk.run_len = 0; wk.nr = 0; wk.ndiag = wk.mis = 0; wk.i0 = wk.i; wk.j0 = wk.j;
	if(ZG){
		uint32_t *stage32 = (uint32_t*)stage;
		const int32_t RB = zrow <= 128 ? 32 : (zrow <= 256 ? 16 : 8);         /* packed rows per staged block: RB * zrow <= 4 KB */
		int32_t i_ = wk.i, j_ = wk.j;
		while(i_ >= 0 && j_ >= 0){
			const int32_t p1 = i_ >> 1, p0 = p1 >= RB - 1 ? p1 - (RB - 1) : 0;
			{
				const uint32_t nd = (uint32_t)(p1 - p0 + 1) * (zrow >> 2);
				const uint32_t *src = (const uint32_t*)(ztr + (size_t)p0 * zrow);
				for(uint32_t xw = (uint32_t)lane; xw < nd; xw += 64) stage32[xw] = src[xw];
			}
			__threadfence_block();
			if(lane == 0){
				while((wk.i | wk.j) >= 0 && (wk.i >> 1) >= p0){
					const int32_t col = wk.j - (wk.i > W ? wk.i - W : 0);
					const uint32_t zv = stage[(size_t)((wk.i >> 1) - p0) * zrow + col];
					wtz_walk_step(wk, zv >> ((wk.i & 1) * 4), qlds, tb32, runs);
				}
			}
			i_ = __builtin_amdgcn_readfirstlane(wk.i); j_ = __builtin_amdgcn_readfirstlane(wk.j);
			__threadfence_block();
		}
		if(lane == 0) wtz_walk_finish(wk, x, runs, n_runs);
	} else
	if(lane == 0){
		while((wk.i | wk.j) >= 0){
			const int32_t col = wk.j - (wk.i > W ? wk.i - W : 0);
			const uint32_t zv = ztr[(size_t)(wk.i >> 1) * zrow + col];
			wtz_walk_step(wk, zv >> ((wk.i & 1) * 4), qlds, tb32, runs);
		}
		wtz_walk_finish(wk, x, runs, n_runs);
	}
	WTZ_PROF_ADD(3, pt_tb);
	return wtz_bcast_aln(x);
}

/* up to 64 bases of a view in two registers */
struct wtz_seq_reg2 { uint64_t w0, w1; WTZ_D uint32_t at(int32_t i) const { return (uint32_t)(((i < 32) ? (w0 >> (2 * i)) : (w1 >> (2 * (i - 32)))) & 3u); } };
/* hz_align_hzmo (hzm_aln.h:278-314) over register-resident sequences; W == NULL only scores.  A mismatching z-mer must leave
 * the CIGAR untouched: the caller snapshots the writer (open run + vector length) and restores it when aln == 0 */
template<typename S1, typename S2>
WTZ_D wtz_aln_t wtz_align_zmer_w(const S1 &pb1, uint32_t len1, const S2 &pb2, uint32_t len2, int32_t M, int32_t I, int32_t D, int32_t E, wtz_cigw_t *W){
	wtz_aln_t x, zero; memset(&zero, 0, sizeof zero); x = zero;
	uint32_t s0 = 0, s1 = 0, e0, e1, l0, l1;
	while(s0 < len1 || s1 < len2){
		const uint32_t b0 = pb1.at((int32_t)s0);
		if(b0 != pb2.at((int32_t)s1)) return zero;
		e0 = s0 + 1; while(e0 < len1 && pb1.at((int32_t)e0) == b0) e0++;
		e1 = s1 + 1; while(e1 < len2 && pb2.at((int32_t)e1) == b0) e1++;
		l0 = e0 - s0; l1 = e1 - s1;
		if(l0 < l1){
			x.aln += l1; x.mat += l0; x.ins += l1 - l0; x.score += (int32_t)l0 * M + I + (int32_t)(l1 - l0) * E;
			if(W){ wtz_cigw_push(*W, 0, l0); wtz_cigw_push(*W, 1, l1 - l0); }
		} else if(l0 == l1){
			x.aln += l0; x.mat += l0; x.score += (int32_t)l0 * M;
			if(W) wtz_cigw_push(*W, 0, l0);
		} else {
			x.aln += l0; x.mat += l1; x.del += l0 - l1; x.score += (int32_t)l1 * M + D + (int32_t)(l0 - l1) * E;
			if(W){ wtz_cigw_push(*W, 0, l1); wtz_cigw_push(*W, 2, l0 - l1); }
		}
		s0 = e0; s1 = e1;
	}
	x.te = x.mat + x.del; x.qe = x.mat + x.ins;
	return x;
}

/* ---- one K-sw1 problem on the wavefront: picks the device form from the problem's shape (register DP with 1 / 2 / 4 / 8 band columns
 *      per lane, 4-bit trace in the LDS slice or in the pool; the scalar body for what is outside every envelope) and runs it.
 *      TEST = true is the form of wtz_test_dp (function-level parity vectors): `force` then names the form instead
 *      (C | 16 = trace in the pool, 255 = scalar body) and R.form = -1 reports a problem outside the forced form's envelope.
 *      LDS slice: 128 target words (1 KB) at L.tb, then the 4-bit trace with its run list at the top end (ztr, ztr_bytes). ---- */
typedef struct { wtz_aln_t y; uint32_t *runs; uint32_t n_runs; bool lds_runs, ok, defer; int form; } wtz_fixres_t;
#define WTZ_FORM_SCALAR 255
template<bool FULL, bool TEST>
WTZ_D void wtz_fixed_problem_wave(int32_t qlen, const wtz_seq_packed &q, int32_t tlen, const wtz_seq_packed &t, int32_t score_in, const wtz_params_t *P,
		const wtz_wave_lds_t &L, uint8_t *ztr, int32_t ztr_bytes, wtz_cigar_t &tmp, wtz_swmem_t &mem, wtz_pool_t *pool, unsigned long long *cells, int force, wtz_fixres_t &R){
	const int lane = (int)(threadIdx.x & 63);
	const int32_t M = P->M, X = P->X, I = P->I, D = P->D, E = P->E, T = P->T;
	wtz_aln_t y; memset(&y, 0, sizeof y);
	R.runs = NULL; R.n_runs = 0; R.lds_runs = false; R.ok = true; R.defer = false; R.form = 0;
	const unsigned long long pt0 = WTZ_PROF_T(); (void)pt0;
	int32_t init = score_in < 0 ? 0 : score_in, W = P->w, ql = 0, tl = 0, n_col = 0; bool okk = true;
	if(qlen > 0 && tlen > 0) wtz_ext_geometry(qlen, tlen, init, W, M, I, D, E, T, ql, tl, n_col);
	const int32_t run_bytes = 4 * (ql + tl + 4);
	const int32_t zrow = (n_col + 3) & ~3;                 /* trace bytes per row pair: one nibble pair per band column */
	const int32_t hmax = init + M * (ql < tl ? ql : tl);                 /* bound of |h|: the register DP packs h and the band column into one int32 key */
	const bool shape = (qlen > 0 && tlen > 0 && ql <= 2048 && (tl + 63) / 32 + 1 <= L.tw);
	bool lds_fit = shape && n_col <= 128 && hmax < (1 << 23) && ((ql + 1) / 2) * zrow + run_bytes <= ztr_bytes;
	bool pool_fit = shape && !lds_fit && n_col <= 512 && hmax < (n_col <= 128 ? (1 << 23) : (1 << 21)) && 4096 + run_bytes <= ztr_bytes;
	int32_t cmin = n_col <= 64 ? 1 : (n_col <= 128 ? 2 : (n_col <= 256 ? 4 : 8));       /* band columns per lane */
	bool scalar = false;
	if constexpr(TEST){
		if(force == WTZ_FORM_SCALAR){ lds_fit = pool_fit = false; scalar = true; }
		else if(force){
			const int32_t fc = force & 15; const bool zg = (force & 16) != 0;
			const bool key_ok = hmax < (fc <= 2 ? (1 << 23) : (1 << 21));
			const bool can = shape && (fc == 1 || fc == 2 || fc == 4 || fc == 8) && fc >= cmin && n_col <= 64 * fc && key_ok && (FULL || fc <= 2)
				&& (zg ? (4096 + run_bytes <= ztr_bytes) : (((ql + 1) / 2) * zrow + run_bytes <= ztr_bytes && fc <= 2));
			if(!can && !(qlen <= 0 || tlen <= 0)){ R.form = -1; R.y = y; return; }
			lds_fit = can && !zg; pool_fit = can && zg; cmin = fc;
		}
	}
	if(!FULL && !(qlen <= 0 || tlen <= 0) && !(lds_fit || (pool_fit && n_col <= 128))){ R.defer = true; R.y = y; return; }
	if(lds_fit){
		R.runs = (uint32_t*)(ztr + ztr_bytes - run_bytes); R.lds_runs = true; R.form = cmin;
		if(cmin == 1) y = wtz_extend_fixed_reg<1>(qlen, q, tlen, t, score_in, ql, tl, W, M, X, I, D, E, T, L.tb, L.qw, ztr, (uint32_t)zrow, R.runs, &R.n_runs, cells);
		else          y = wtz_extend_fixed_reg<2>(qlen, q, tlen, t, score_in, ql, tl, W, M, X, I, D, E, T, L.tb, L.qw, ztr, (uint32_t)zrow, R.runs, &R.n_runs, cells);
	} else if(pool_fit){
		/* the 4-bit trace does not fit the LDS slice (or the band is wider than 128 columns): trace in the pool, traceback through a
		 * 4 KB LDS stage, run list in LDS above the stage */
		unsigned long long za = 0;
		if(lane == 0) za = (unsigned long long)(uintptr_t)wtz_pool_alloc(pool, (size_t)((ql + 1) / 2) * zrow);
		za = __shfl(za, 0, 64);
		if(za == 0){ R.ok = false; R.y = y; return; }
		uint8_t *zg = (uint8_t*)(uintptr_t)za;
		R.runs = (uint32_t*)(ztr + ztr_bytes - run_bytes); R.lds_runs = true; R.form = cmin | 16;
		if(cmin == 1)      y = wtz_extend_fixed_reg<1, true>(qlen, q, tlen, t, score_in, ql, tl, W, M, X, I, D, E, T, L.tb, L.qw, zg, (uint32_t)zrow, R.runs, &R.n_runs, cells, ztr);
		else if(cmin == 2) y = wtz_extend_fixed_reg<2, true>(qlen, q, tlen, t, score_in, ql, tl, W, M, X, I, D, E, T, L.tb, L.qw, zg, (uint32_t)zrow, R.runs, &R.n_runs, cells, ztr);
		else if constexpr(FULL){
			if(cmin == 4) y = wtz_extend_fixed_reg<4, true>(qlen, q, tlen, t, score_in, ql, tl, W, M, X, I, D, E, T, L.tb, L.qw, zg, (uint32_t)zrow, R.runs, &R.n_runs, cells, ztr);
			else          y = wtz_extend_fixed_reg<8, true>(qlen, q, tlen, t, score_in, ql, tl, W, M, X, I, D, E, T, L.tb, L.qw, zg, (uint32_t)zrow, R.runs, &R.n_runs, cells, ztr);
		}
		WTZ_PROF_ADD(55, pt0); WTZ_PROF_CNT(7, 1); WTZ_PROF_CNT(13, ql); WTZ_PROF_CNT(14, n_col);
	} else if(qlen <= 0 || tlen <= 0){
		/* empty problem (wtz_extend_fixed: score = init, nothing aligned, empty CIGAR) */
		memset(&y, 0, sizeof y); y.score = init; if(lane == 0) tmp.n = 0;
	} else if constexpr(FULL){
		/* whatever is outside the register DP's envelope (rows > 2048, band > 512 columns, huge scores): the scalar body */
		(void)scalar;
		const unsigned long long ptw = WTZ_PROF_T(); (void)ptw;
		R.form = WTZ_FORM_SCALAR;
		if(lane == 0){ tmp.n = 0; y = wtz_extend_fixed(qlen, q, tlen, t, score_in, P->w, M, X, I, D, E, T, mem, tmp); if(mem.bad) okk = false; }
		y = wtz_bcast_aln(y);
		okk = __shfl((int)okk, 0, 64) != 0;
		WTZ_PROF_ADD(10, ptw); WTZ_PROF_CNT(8, 1);
	}
	if(R.lds_runs) WTZ_PROF_CNT(6, 1);
	if(!okk) R.ok = false;
	R.y = y;
}

/* ---- A9 with the K-sw1 gaps run by the whole wave (hzm_aln.h:1247-1302).  Every lane follows the anchor loop with
 *      the same x; CIGAR bookkeeping and the run-by-run z-mer alignment stay on lane 0.  lds: >= 8 KB. ---- */
/* FULL = false is the form of the first launch: only the one / two-columns-per-lane register DP (and the empty problem) are compiled
 * in; a window with a problem that needs anything else sets *defer and is redone from scratch by a FULL launch. */
template<bool FULL = true>
WTZ_D wtz_aln_t wtz_align_window_wave(const wtz_readview &pb1, const wtz_readview &pb2, const wtz_win_t &win, const wtz_zhit_t *anchors,
		wtz_cigar_t &cigar, wtz_cigar_t &tmp, const wtz_params_t *P, wtz_pool_t *pool, int32_t *lds, unsigned long long *cells, bool *ok, bool *defer = NULL){
	const int lane = (int)(threadIdx.x & 63);
	const int32_t M = P->M, I = P->I, D = P->D, E = P->E;
	/* LDS slice: 128 target words (1 KB), then the 4-bit trace of the register DP with its run list at the top end (7 KB) */
	wtz_wave_lds_t L; L.tb = (uint64_t*)lds; L.Hs = lds + 256; L.Es = lds + 768; L.PM = 511; L.tw = 128; L.qw = (uint32_t*)(lds + WTZ_WINALIGN_LDS_BYTES / 4);
	uint8_t *ztr = (uint8_t*)(lds + 256); const int32_t ztr_bytes = WTZ_WINALIGN_LDS_BYTES - 1024;
	wtz_swmem_t mem; wtz_swmem_init(mem, pool);
	wtz_aln_t x, y; memset(&x, 0, sizeof x);
	wtz_cigw_t Wc; Wc.v = &cigar; Wc.tail = 0;
	*ok = true;
	for(uint32_t i = win.anchors[0]; i < win.anchors[1]; i++){
		const wtz_zhit_t p = anchors[i];
		const int32_t off1 = (int32_t)ZH_OFF1(p), off2 = (int32_t)ZH_OFF2(p);
		if(x.aln == 0){ x.tb = x.te = off1; x.qb = x.qe = off2; }
		if(off1 < x.te) continue;
		if(off2 < x.qe) continue;
		const int32_t qlen = off2 - x.qe, tlen = off1 - x.te;
		const unsigned long long pt0 = WTZ_PROF_T();
		wtz_fixres_t R;
		wtz_fixed_problem_wave<FULL, false>(qlen, pb2.sub(x.qe, 1), tlen, pb1.sub(x.te, 1), x.score, P, L, ztr, ztr_bytes, tmp, mem, pool, cells, 0, R);
		if(!FULL && R.defer){ *defer = true; return x; }
		if(!R.ok){ *ok = false; return x; }
		y = R.y;
		const uint32_t n_runs = R.n_runs; const uint32_t *runs = R.runs; const bool lds_runs = R.lds_runs;
		WTZ_PROF_ADD(0, pt0);
		const unsigned long long pt1 = WTZ_PROF_T();
		int32_t stop = 0;
		if(lane == 0){
			x.score = y.score;
			x.aln += y.aln; x.mat += y.mat; x.mis += y.mis; x.ins += y.ins; x.del += y.del;
			x.te += y.te; x.qe += y.qe;
			if(lds_runs){ for(uint32_t k = n_runs; k-- > 0;){ const uint32_t r = runs[k]; wtz_cigw_push(Wc, r & 0xFu, r >> 4); } }
			else { for(uint32_t k = 0; k < tmp.n; k++){ const uint32_t r = tmp.a[k]; wtz_cigw_push(Wc, r & 0xFu, r >> 4); } }
			if(x.te < off1){ x.del += off1 - x.te; x.aln += off1 - x.te; wtz_cigw_push(Wc, 2, (uint32_t)(off1 - x.te)); x.te = off1; }
			if(x.qe < off2){ x.ins += off2 - x.qe; x.aln += off2 - x.qe; wtz_cigw_push(Wc, 1, (uint32_t)(off2 - x.qe)); x.qe = off2; }
			WTZ_PROF_ADD(48, pt1); WTZ_PROF_CNT(50, 1000); WTZ_PROF_CNT(51, n_runs); WTZ_PROF_CNT(52, (qlen > 0 ? qlen : 0)); WTZ_PROF_CNT(53, (tlen > 0 ? tlen : 0));
			const unsigned long long pt2 = WTZ_PROF_T(); (void)pt2;
			const uint32_t len1 = ZH_LEN1(p), len2 = ZH_LEN2(p);
			const wtz_seq_packed z1 = pb1.sub(off1, 1), z2 = pb2.sub(off2, 1);
			/* one pass that writes its runs; a z-mer pair that turns out not to align (aln == 0) is rolled back: the writer's
			 * state is its open run plus the vector length */
			const uint32_t keep_tail = Wc.tail, keep_n = cigar.n;
			if(len1 <= 64 && len2 <= 64){
				wtz_seq_reg2 r1, r2;
				r1.w0 = wtz_pack32(z1, 0, (int32_t)len1); r1.w1 = wtz_pack32(z1, 32, (int32_t)len1);
				r2.w0 = wtz_pack32(z2, 0, (int32_t)len2); r2.w1 = wtz_pack32(z2, 32, (int32_t)len2);
				if(len1 == len2 && r1.w0 == r2.w0 && r1.w1 == r2.w1){
					/* the two expanded z-mers are the same string (no homopolymer-length difference): every run matches in full, the
					 * runs merge into one M of the whole length (hzm_aln.h:278-314 run by run gives exactly that) */
					memset(&y, 0, sizeof y);
					y.aln = y.mat = (int32_t)len1; y.te = y.qe = (int32_t)len1; y.score = (int32_t)len1 * M;
					wtz_cigw_push(Wc, 0, len1);
				} else
				y = wtz_align_zmer_w(r1, len1, r2, len2, M, I, D, E, &Wc);
			} else {
				y = wtz_align_zmer_w(z1, len1, z2, len2, M, I, D, E, &Wc);
			}
			if(y.aln == 0){ Wc.tail = keep_tail; cigar.n = keep_n; }
			if(y.aln == 0) stop = 1;
			else {
				x.score += y.score;
				x.aln += y.aln; x.mat += y.mat; x.mis += y.mis; x.ins += y.ins; x.del += y.del;
				x.te += y.te; x.qe += y.qe;
			}
			WTZ_PROF_ADD(49, pt2); WTZ_PROF_CNT(54, len1 + len2);
		}
		x = wtz_bcast_aln(x);
		stop = __shfl(stop, 0, 64);
		WTZ_PROF_ADD(1, pt1);
		if(stop) break;
	}
	if(lane == 0) wtz_cigw_finish(Wc);
	return x;
}

#endif /* __HIPCC__ */
#endif
