/*
 * K-glob: ksw_global2 (ksw.c:503-586) at ONE band width w over a whole rectangle - the banded global alignment that kswx_gen_cigar_core2
 * (kswx.h:1443-1482) runs over the extended hit of kswx_align.  One wavefront per problem; the same body runs with ONE lane in the host
 * emulation (tests/emul), where it is the CPU restatement that tests/test_kglob_cpu.py pins against the reference routine itself.
 *
 * What the reference computes (32-bit ints; rows i = target, columns j = query; beg = max(i - w, 0), end = min(i + w + 1, qlen)):
 *     row -1   H(-1, -1) = 0, H(-1, j) = -(o_ins + e_ins * (j + 1)) for j < w, E = MINUS_INF                          (ksw.c:521-524)
 *     row i    H(i, -1) = -(o_del + e_del * (i + 1)) while beg == 0, F = MINUS_INF at j = beg                           (ksw.c:527, 532)
 *              M = H(i-1, j-1) + S(t_i, q_j)         h = M >= E ? M : E  (d = 0 / 1)      h = h >= F ? h : F  (d = 2)     (ksw.c:549-552)
 *              E(i+1, j) = max(E - e_del, M - oe_del), bit 2 of d when E - e_del >  M - oe_del                          (ksw.c:554-557)
 *              F(i, j+1) = max(F - e_ins, M - oe_ins), bit 3 of d when F - e_ins >  M - oe_ins                          (ksw.c:559-562)
 *     score    H(tlen - 1, qlen - 1); the walk of ksw.c:571-579 starts there and reads, per cell, the field of d that the state names.
 * E and F are fed from M, not from h: the CIGAR that ksw.c:541-543 calls impossible stays impossible.  Every in-band M is finite (its diagonal
 * predecessor is in the band of the row before, or on the boundary), so E and F of a live cell are finite from the second cell on and any sentinel far
 * below the finite values gives the reference's direction bits; the host checks that the finite values stay above -2^28 (glob_plan, wtz_lib_glob.h).
 *
 * Device form: K-kext's DIAGONAL FRAME (wtz_sw_kext.h) at a fixed band.  Slot s = j - i + dlo, dlo = min(w, tlen - 1), is fixed to lane s / C, register
 * s % C; H(i-1, j-1) is the slot's own value of the row before, E(i, j) was written by the slot to the right (one wave_shl per row), F is the max-plus
 * prefix over the slots (register chain + one DPP prefix maximum over the lanes' aggregates).  No floor, no band trim, no row reductions.  A slot outside
 * [beg, end) writes H = H(i, -1) (what the cell of column 0 of the next row reads) and E = sentinel.  The query window, its 32-row reload and the
 * target word are K-kext's (wtz_kext_bases).
 *
 * Trace: 4 bits per cell (d & 3, bit 2, bit 3), in slot order.  A lane packs its C cells of a row into C / 8 32-bit words (C >= 8) or gathers 8 / C rows into
 * one word (C < 8: a "row group"); every lane of the wave stores its words of a group with ONE full-width store (dword, dwordx2, dwordx4: 16 bytes per lane
 * and row at C = 32), so that a group of the wave is 64 * max(C / 8, 1) contiguous words: word (group * 64 + lane) * WPL + n.  The stores go through a
 * global-address-space pointer and nothing in the row loop waits for them; the loop's only loads are the sequence words every 32 rows.
 *
 * Traceback, same kernel, same wavefront, after one fence: the walk stages a WINDOW of the trace in LDS - WTZ_KGLOB_WIN_GROUPS (64) row groups x
 * WTZ_KGLOB_WIN_WORDS (32) words of a group, 8 KB: at C >= 8 that is 64 rows x 256 slots - with all 64 lanes (each load instruction fetches two rows' 128
 * contiguous bytes; the compiled loop keeps 8 loads in flight and drains them before the next 8), then walks it with wave-uniform control (the staged word is read with a broadcast).  RESTAGING RULE: when the
 * current cell's word lies outside the window, the window is placed again with the current row group as its LAST group (the walk only goes up) and the
 * current word in the MIDDLE of its 32 words (a vertical run drifts to higher slots, a horizontal run to lower ones), clamped to the trace.  So a diagonal or
 * vertical stretch restages every 64 groups, a horizontal run every 128 slots.  Runs (len << 4 | op, op 1 = query-only, 2 = target-only) are written
 * downwards from the end of the problem's run buffer, so that they read first operation first; both tails of ksw.c:578-579 are merged like push_cigar does.
 * Matches and mismatches of the op-0 runs are counted afterwards by all lanes, 32 bases per lane and step from the packed views (XOR + popcount).
 */
#ifndef WTZ_SW_KGLOB_H
#define WTZ_SW_KGLOB_H

#include "wtz_sw_kext.h"

#define WTZ_KGLOB_MAXSLOTS 2047       /* 64 lanes x 32 registers, as K-kext */
#define WTZ_KGLOB_NEG WTZ_KEXT_NEG
#define WTZ_KGLOB_WIN_GROUPS 64
#define WTZ_KGLOB_WIN_WORDS 32
#define WTZ_KGLOB_STAGE_WORDS (WTZ_KGLOB_WIN_GROUPS * WTZ_KGLOB_WIN_WORDS)

/* tr_off / run_off: first word of the problem's trace / run buffer inside the launch group's block; run_cap: words of the run buffer (>= qlen + tlen) */
typedef struct { wtz_seq_packed q, t; int32_t qlen, tlen, w, dlo; unsigned long long tr_off, run_off; uint32_t run_cap, pad; } wtz_kglobprob_t;
/* runs: first operation first; ticks_dp / ticks_tb: the wave's clock over the DP rows / over traceback and counting (0 in the emulation) */
typedef struct { int32_t score, mat, mis; uint32_t n_runs; const uint32_t *runs; unsigned long long cells, ticks_dp, ticks_tb; int32_t bad, pad; } wtz_kglobres_t;
typedef struct { int32_t M, X, o_del, e_del, o_ins, e_ins; } wtz_kglobsc_t;

/* words of a lane per row group, rows per group, words of the wave per group, and the trace words of a problem of tlen rows */
WTZ_HD int32_t wtz_kglob_wpl(int32_t C){ return C >= 8 ? C / 8 : 1; }
WTZ_HD int32_t wtz_kglob_rpg(int32_t C){ return C >= 8 ? 1 : 8 / C; }
WTZ_HD unsigned long long wtz_kglob_trace_words(int32_t C, int32_t tlen){
	const int32_t rpg = wtz_kglob_rpg(C);
	return (unsigned long long)((tlen + rpg - 1) / rpg) * 64ull * (unsigned long long)wtz_kglob_wpl(C);
}
WTZ_HD int32_t wtz_kglob_slots(int32_t qlen, int32_t tlen, int32_t w){ return (w < tlen - 1 ? w : tlen - 1) + (w < qlen - 1 ? w : qlen - 1) + 1; }

#if defined(__HIP_DEVICE_COMPILE__)
WTZ_D unsigned long long wtz_kglob_clock(){ return (unsigned long long)wall_clock64(); }
WTZ_D uint32_t wtz_kglob_sum(uint32_t v){ uint32_t tot; (void)wtz_coop_excl_scan(v, &tot); return tot; }
#define WTZ_KGLOB_FENCE() __threadfence()
typedef uint32_t wtz_kglob_v2 __attribute__((ext_vector_type(2)));
typedef uint32_t wtz_kglob_v4 __attribute__((ext_vector_type(4)));
#else
WTZ_COOP_HOST unsigned long long wtz_kglob_clock(){ return 0ull; }
WTZ_COOP_HOST uint32_t wtz_kglob_sum(uint32_t v){ return v; }
#define WTZ_KGLOB_FENCE() do {} while(0)
#endif

/* the DP rows: writes the trace, returns H(tlen - 1, qlen - 1) (every lane) */
template<int C>
WTZ_HD int32_t wtz_kglob_dp(const wtz_kglobprob_t &p, const wtz_kglobsc_t &S, uint32_t *tr, unsigned long long &cells_out){
	constexpr int SUB = 64 / WTZ_LOC_LANES, CL = C * SUB, NW = (CL + 31) / 32;
	constexpr int WPL = C >= 8 ? C / 8 : 1, RPG = C >= 8 ? 1 : 8 / C, TW = WPL * SUB;
	const int32_t lane = (int32_t)WTZ_LANE, s0 = lane * CL;
	const int32_t qlen = (int32_t)wtz_coop_bcast32((uint32_t)p.qlen), tlen = (int32_t)wtz_coop_bcast32((uint32_t)p.tlen);
	const int32_t w = (int32_t)wtz_coop_bcast32((uint32_t)p.w), dlo = (int32_t)wtz_coop_bcast32((uint32_t)p.dlo);
	const int32_t Mm = S.M, X = S.X, e_del = S.e_del, e_ins = S.e_ins, oe_del = S.o_del + S.e_del, oe_ins = S.o_ins + S.e_ins;
	int32_t H[CL], E[CL];
	uint64_t qw[NW + 1];
	uint32_t tw[TW];
	/* row -1 as the slots of row 0 see it: slot s = column s - dlo; H(-1, j - 1) = -(o_ins + e_ins * j) */
	#pragma unroll
	for(int k = 0; k < CL; k++){
		const int32_t j = s0 + k - dlo;
		H[k] = j <= 0 ? 0 : -(S.o_ins + e_ins * j);
		E[k] = WTZ_KGLOB_NEG;
	}
	#pragma unroll
	for(int n = 0; n < TW; n++) tw[n] = 0;
	#pragma unroll
	for(int n = 0; n < NW; n++) qw[n] = wtz_kext_bases(p.q, s0 - dlo + 32 * n, qlen);
	qw[NW] = 0;
	uint64_t qpre = wtz_kext_bases(p.q, s0 - dlo + 32 * NW, qlen);
	uint64_t tcur = 0, tnext = wtz_pack32(p.t, 0, tlen);
	unsigned long long cells = 0;
	int32_t score = WTZ_KGLOB_NEG;
#if defined(__HIP_DEVICE_COMPILE__)
	WTZ_GLOBAL_AS uint32_t *trg = wtz_as_global(tr);
#endif
	for(int32_t i = 0; i < tlen; i++){
		if((i & 31) == 0){      /* the next 32 rows' sequence words: loaded and waited for here, once per 32 rows (the wait also drains the trace stores issued so far) */
			tcur = tnext; tnext = wtz_pack32(p.t, i + 32, tlen);
			qw[NW] = qpre; qpre = wtz_kext_bases(p.q, s0 - dlo + i + 32 * NW + 32, qlen);
		}
		const uint32_t tb = (uint32_t)(tcur >> (2 * (i & 31))) & 3u;
		const int32_t beg = i > w ? i - w : 0, end = i + w + 1 < qlen ? i + w + 1 : qlen;
		const int32_t h1 = beg == 0 ? -(S.o_del + e_del * (i + 1)) : WTZ_KGLOB_NEG;
		const int32_t off = i - dlo;                                      /* column of slot s: s + off */
		const int32_t lo = beg - off - s0, hi = end - off - s0;           /* the lane's live slots: lo <= k < hi */
		cells += (unsigned long long)(end > beg ? end - beg : 0);
		/* ---- pass 1: M in place, the lane's F aggregate ---- */
		int32_t agg = WTZ_KGLOB_NEG;
		#pragma unroll
		for(int n = 0; n < NW; n++){
			const uint64_t x = qw[n] ^ (0x5555555555555555ull * tb);
			const uint64_t eq = ~(x | (x >> 1)) & 0x5555555555555555ull;
			#pragma unroll
			for(int kk = 0; kk < 32; kk++){
				const int k = n * 32 + kk;
				if(k < CL){
					const int32_t m = H[k] + (((eq >> (2 * kk)) & 1ull) ? Mm : X);
					H[k] = m;
					int32_t g = m - oe_ins + e_ins * (k + 1);      /* + e_ins * s0, the same for all of the lane's slots: added once below */
					g = g > agg ? g : agg;
					agg = (k >= lo && k < hi) ? g : agg;
				}
			}
		}
		/* ---- F carry from the lanes to the left: F at the lane's first slot, or the sentinel ---- */
		int32_t f;
		{ const int32_t cin = wtz_kext_scan_excl(agg + e_ins * s0, WTZ_KGLOB_NEG) - e_ins * s0; f = cin > WTZ_KGLOB_NEG ? cin : WTZ_KGLOB_NEG; }
		/* ---- pass 2: the cells ---- */
		const int32_t r = i % RPG;
		int32_t e0 = WTZ_KGLOB_NEG;
		#pragma unroll
		for(int k = 0; k < CL; k++){
			const bool live = k >= lo && k < hi;
			const int32_t m = H[k], e = E[k];
			uint32_t d = m >= e ? 0u : 1u;
			int32_t h = m >= e ? m : e;
			d = h >= f ? d : 2u;
			h = h >= f ? h : f;
			const int32_t t = m - oe_del; int32_t en = e - e_del;
			d |= en > t ? 4u : 0u;
			en = en > t ? en : t;
			const int32_t g = m - oe_ins; int32_t fn = f - e_ins;
			d |= fn > g ? 8u : 0u;
			fn = fn > g ? fn : g;
			H[k] = live ? h : h1;
			f = live ? fn : WTZ_KGLOB_NEG;
			en = live ? en : WTZ_KGLOB_NEG;
			d = live ? d : 0u;
			if(k == 0) e0 = en; else E[k - 1] = en;
			const int nib0 = k % C;      /* + r * C inside a group of several rows */
			if constexpr(C >= 8) tw[(k / C) * WPL + nib0 / 8] |= d << (4 * (nib0 % 8));
			else tw[k / C] |= d << (4 * (r * C + nib0));
		}
		E[CL - 1] = wtz_kext_from_right(WTZ_KGLOB_NEG, e0);
		/* ---- the group's words go out ---- */
		if(r == RPG - 1 || i == tlen - 1){
			const size_t base = ((size_t)(i / RPG) * 64u + (size_t)(s0 / C)) * (size_t)WPL;
#if defined(__HIP_DEVICE_COMPILE__)
			if constexpr(WPL == 4){ wtz_kglob_v4 v; v.x = tw[0]; v.y = tw[1]; v.z = tw[2]; v.w = tw[3]; *(WTZ_GLOBAL_AS wtz_kglob_v4*)(trg + base) = v; }
			else if constexpr(WPL == 2){ wtz_kglob_v2 v; v.x = tw[0]; v.y = tw[1]; *(WTZ_GLOBAL_AS wtz_kglob_v2*)(trg + base) = v; }
			else trg[base] = tw[0];
#else
			for(int n = 0; n < TW; n++) tr[base + n] = tw[n];
#endif
			#pragma unroll
			for(int n = 0; n < TW; n++) tw[n] = 0;
		}
		if(i == tlen - 1){      /* the corner: column qlen - 1 */
			const int32_t kc = qlen - 1 - off - s0;
			int32_t sel = WTZ_KGLOB_NEG;
			#pragma unroll
			for(int k = 0; k < CL; k++) sel = (k == kc) ? H[k] : sel;
			score = wtz_kext_max(sel);
		}
		/* the query moves one column to the left in the frame */
		#pragma unroll
		for(int n = 0; n < NW; n++) qw[n] = (qw[n] >> 2) | (qw[n + 1] << 62);
		qw[NW] >>= 2;
	}
	cells_out = cells;
	return score;
}

/* the walk of ksw.c:571-579 over the trace written by wtz_kglob_dp<C>; stg: WTZ_KGLOB_STAGE_WORDS words (LDS on the device).  Runs end at runs[cap]: the list
 * is runs[cap - n_runs, cap).  Every lane returns the same n_runs; -1: the run buffer is too small (cannot happen with cap >= qlen + tlen). */
template<int C>
WTZ_HD int32_t wtz_kglob_walk(const wtz_kglobprob_t &p, const uint32_t *tr, uint32_t *stg, uint32_t *runs, uint32_t cap){
	constexpr int WPL = C >= 8 ? C / 8 : 1, RPG = C >= 8 ? 1 : 8 / C, GW = 64 * WPL, GR = WTZ_KGLOB_WIN_GROUPS, CWN = WTZ_KGLOB_WIN_WORDS;
	const int32_t lane = (int32_t)WTZ_LANE, NL = (int32_t)WTZ_NLANES;
	const int32_t qlen = (int32_t)wtz_coop_bcast32((uint32_t)p.qlen), tlen = (int32_t)wtz_coop_bcast32((uint32_t)p.tlen);
	const int32_t w = (int32_t)wtz_coop_bcast32((uint32_t)p.w), dlo = (int32_t)wtz_coop_bcast32((uint32_t)p.dlo);
	int32_t i = tlen - 1, k = (i + w + 1 < qlen ? i + w + 1 : qlen) - 1;
	int32_t g_lo = 1, g_hi = 0, cw_lo = 0;      /* empty window */
	uint32_t which = 0, cur_op = 0xFu, cur_len = 0, n = 0;
	bool full = false;
	auto push = [&](uint32_t op, uint32_t len){
		if(op == cur_op){ cur_len += len; return; }
		if(cur_len){ if(n < cap){ if(lane == 0) runs[cap - 1 - n] = cur_len << 4 | cur_op; n++; } else full = true; }
		cur_op = op; cur_len = len;
	};
	while(i >= 0 && k >= 0){
		const int32_t s = k - i + dlo, g = i / RPG;
		const int32_t nib = C >= 8 ? s % C : (i % RPG) * C + s % C;
		const int32_t cw = (s / C) * WPL + nib / 8;
		if(g < g_lo || g > g_hi || cw < cw_lo || cw >= cw_lo + CWN){
			g_hi = g; g_lo = g - GR + 1 > 0 ? g - GR + 1 : 0;
			cw_lo = cw - CWN / 2; if(cw_lo > GW - CWN) cw_lo = GW - CWN; if(cw_lo < 0) cw_lo = 0;
			const int32_t nwords = (g_hi - g_lo + 1) * CWN;
			WTZ_WAVE_SYNC();
			for(int32_t idx = lane; idx < nwords; idx += NL) stg[idx] = tr[(size_t)(g_lo + idx / CWN) * GW + (size_t)(cw_lo + idx % CWN)];
			WTZ_WAVE_SYNC();
		}
		const uint32_t word = wtz_coop_bcast32(stg[(g - g_lo) * CWN + (cw - cw_lo)]);
		const uint32_t z = (word >> (4 * (nib % 8))) & 15u;
		which = which == 0 ? (z & 3u) : (which == 1 ? ((z >> 2) & 1u) : ((z >> 3) & 1u) * 2u);
		if(which == 0){ push(0, 1); i--; k--; }
		else if(which == 1){ push(2, 1); i--; }
		else { push(1, 1); k--; }
	}
	if(i >= 0) push(2, (uint32_t)(i + 1));
	if(k >= 0) push(1, (uint32_t)(k + 1));
	push(0xEu, 0);      /* flushes the last run */
	return full ? -1 : (int32_t)n;
}

/* matches and mismatches of the op-0 runs of a run list (first operation first), 32 bases per lane and step */
WTZ_HD void wtz_kglob_count(const wtz_kglobprob_t &p, const uint32_t *runs, uint32_t n_runs, int32_t &mat, int32_t &mis){
	const int32_t lane = (int32_t)WTZ_LANE, NL = (int32_t)WTZ_NLANES;
	const int32_t qlen = (int32_t)wtz_coop_bcast32((uint32_t)p.qlen), tlen = (int32_t)wtz_coop_bcast32((uint32_t)p.tlen);
	int32_t x1 = 0, x2 = 0; uint32_t diff = 0, tot = 0;
	for(uint32_t r = 0; r < n_runs; r++){
		const uint32_t run = wtz_coop_bcast32(runs[r]), op = run & 0xFu; const int32_t len = (int32_t)(run >> 4);
		if(op == 0){
			for(int32_t c = lane * 32; c < len; c += NL * 32){
				const int32_t nb = len - c < 32 ? len - c : 32;
				uint64_t x = wtz_pack32(p.q, x1 + c, qlen) ^ wtz_pack32(p.t, x2 + c, tlen);
				x = (x | (x >> 1)) & 0x5555555555555555ull;
				if(nb < 32) x &= (1ull << (2 * nb)) - 1ull;
				diff += (uint32_t)__builtin_popcountll(x);
			}
			x1 += len; x2 += len; tot += (uint32_t)len;
		} else if(op == 1) x1 += len;
		else x2 += len;
	}
	diff = wtz_kglob_sum(diff);
	mis = (int32_t)diff; mat = (int32_t)(tot - diff);
}

/* one problem: DP, fence, walk, count.  tr / runs: the problem's own trace and run buffer */
template<int C>
WTZ_HD void wtz_kglob_problem(const wtz_kglobprob_t &p, const wtz_kglobsc_t &S, uint32_t *tr, uint32_t *runs, uint32_t *stg, wtz_kglobres_t &r){
	const unsigned long long t0 = wtz_kglob_clock();
	r.score = wtz_kglob_dp<C>(p, S, tr, r.cells);
	WTZ_KGLOB_FENCE();
	const unsigned long long t1 = wtz_kglob_clock();
	const uint32_t cap = wtz_coop_bcast32(p.run_cap);
	const int32_t n = wtz_kglob_walk<C>(p, tr, stg, runs, cap);
	r.bad = n < 0 ? 1 : 0; r.pad = 0;
	r.n_runs = n < 0 ? 0u : (uint32_t)n;
	r.runs = runs + (cap - r.n_runs);
	WTZ_KGLOB_FENCE();
	wtz_kglob_count(p, r.runs, r.n_runs, r.mat, r.mis);
	r.ticks_dp = t1 - t0; r.ticks_tb = wtz_kglob_clock() - t1;
}

#if defined(__HIPCC__) && !defined(WTZ_EMUL)
/* resident waves per SIMD the instantiations are compiled for: K-kext's register budgets from C = 8 on (the row state is the same, the trace words come on
 * top); below that the 8 KB traceback window of every wave decides: 160 KB of LDS per CU hold 20 windows, 5 waves per SIMD */
#ifndef WTZ_KGLOB_OCC
#define WTZ_KGLOB_OCC(C) ((C) <= 4 ? 5 : ((C) <= 8 ? 4 : ((C) <= 16 ? 3 : 2)))
#endif
/* block b = one wavefront = problem order[b] (largest first); every problem of a launch has wtz_kext_form(slots) == C */
template<int C>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WTZ_KGLOB_OCC(C), 8)))
wtz_kernel_kglob(const wtz_kglobprob_t *pr, const uint32_t *order, uint32_t n, wtz_kglobsc_t S, uint32_t *trace, uint32_t *runbuf, wtz_kglobres_t *res){
	__shared__ uint32_t stg[WTZ_KGLOB_STAGE_WORDS];
	if(blockIdx.x >= n) return;
	const uint32_t id = order[blockIdx.x];
	const wtz_kglobprob_t p = pr[id];
	wtz_kglobres_t r;
	wtz_kglob_problem<C>(p, S, trace + p.tr_off, runbuf + p.run_off, stg, r);
	if(WTZ_LANE == 0) res[id] = r;
}
#endif
#endif
