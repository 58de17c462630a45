/*
 * K-kext: ksw_extend2 (ksw.c:381-478) - the banded extension with a clip bonus and a data-dependent, self-trimming band that kswx_extend_core
 * (kswx.h:1386-1441) calls once per end of a local hit.  One wavefront per problem; the same body runs with ONE lane in the host emulation
 * (tests/emul), where it is the CPU restatement that tests/test_kext_cpu.py pins against the reference routine itself.
 *
 * What the reference computes (32-bit ints, no saturation; rows i = target, columns j = query; eh[] = one (h, e) pair per column):
 *     row -1   eh[0].h = h0, eh[j].h = max(h0 - o_ins - e_ins * j, 0), all e = 0                                       (ksw.c:396-398)
 *     row i    beg = max(beg, i - w), end = min(end, i + w + 1, qlen); for j in [beg, end):
 *                  M = H(i-1, j-1) + S(t_i, q_j)        (not floored)         h = max(M, e, f), f = 0 at j = beg
 *                  E(i+1, j) = max(e - e_del, M - oe_del, 0)                  F(i, j+1) = max(f - e_ins, M - oe_ins, 0)   (both fed from M, not from h)
 *              H(i, beg-1) = max(0, h0 - o_del - e_del * (i + 1)) whatever beg is (ksw.c:417); eh[end] = { H(i, end-1), 0 }   (ksw.c:448)
 *     m, mj    the row maximum (>= 0: e and f are) and the LAST column holding it; m == 0 ends the DP (ksw.c:453)
 *     gscore   when the column loop ended at j == qlen: H(i, qlen-1) with >=, the last such row wins (ksw.c:449-452)
 *     band     beg' = one past the nearest j <= mj with eh[j].h == 0, end' = the nearest j >= mj + 2 with eh[j].h == 0, else end + 1 (ksw.c:465-468),
 *              read on eh as the row left it: eh[j].h = H(i, j-1)
 *
 * Device form: the DIAGONAL FRAME.  Slot s = j - i + dlo is fixed to a lane / register (lane s / C, register s % C), dlo = min(w, tlen - 1); the band
 * never leaves [0, dlo + min(w, qlen - 1)], which is what C is chosen from.  In that frame
 *     H(i-1, j-1) is the slot's OWN value of the row before (eh[j].h of the reference = the slot's h, in place);
 *     E(i, j) was written by the slot to the RIGHT (each cell writes its E into its left neighbour's register: no moves; one wave_shl per row);
 *     F is a max-plus prefix over the slots: f(s) = max over live k < s of (max(M_k - oe_ins, 0) + e_ins * (k + 1)) - e_ins * s, floored at 0:
 *     a register chain inside the lane, one DPP prefix-maximum over the lanes' aggregates for the carry.
 * A slot outside [beg, end) writes h = H(i, beg-1) and E = 0: the only such values a later row can read are eh[beg].h (the slot left of the band) and
 * eh[end].e (the slot right of it, read by the band's last slot); end grows by at most one per row and beg never falls, so nothing else is ever read.
 * Per row: four wave reductions (row maximum, last slot holding it, nearest zero left / right of it) and, when the band touches qlen, the pick of
 * H(i, end-1).  The query slides by one column per row: each lane keeps its 32 * ceil(C / 32) bases and the 32 behind them in 64-bit words that shift by
 * one base per row; the next 32 are loaded a block of 32 rows ahead, like the target's.  Nothing of the row state goes to memory.
 */
#ifndef WTZ_SW_KEXT_H
#define WTZ_SW_KEXT_H

#include "wtz_sw_local.h"

/* WTZ_KEXT_MAXW (band half-width: 2 * 1023 + 1 slots = 64 lanes x 32 registers) and WTZ_KEXT_MAXLEN (rows and columns of one problem): include/wtzmo_hip.h */
#define WTZ_KEXT_MAXC 32
#define WTZ_KEXT_NEG (-0x40000000)

typedef struct { wtz_seq_packed q, t; int32_t qlen, tlen, h0, w, dlo; } wtz_kextprob_t;      /* w: after the clamp of ksw.c:403-408; h0 >= 0 */
typedef struct { int32_t score, qle, tle, gtle, gscore, max_off; uint32_t rows; unsigned long long cells; } wtz_kextres_t;
typedef struct { int32_t M, X, o_del, e_del, o_ins, e_ins, zdrop; } wtz_kextsc_t;

/* slots per lane for a band of `slots` live diagonals: the instantiations are 1, 2, 4, 8, 16, 32 */
WTZ_HD int32_t wtz_kext_form(int32_t slots){ int32_t c = 1; while(c < WTZ_KEXT_MAXC && 64 * c < slots) c <<= 1; return c; }

#if defined(__HIP_DEVICE_COMPILE__)
WTZ_D int32_t wtz_kext_scan_excl(int32_t v, int32_t ident){ return wtz_wave_max_scan_excl(v, ident); }
WTZ_D int32_t wtz_kext_max(int32_t v){ return wtz_wave_max_i32(v); }
WTZ_D int32_t wtz_kext_from_right(int32_t last, int32_t v){ return wtz_dpp_wave_shl1(last, v); }      /* lane 63 gets `last` */
#else
WTZ_COOP_HOST int32_t wtz_kext_scan_excl(int32_t, int32_t ident){ return ident; }
WTZ_COOP_HOST int32_t wtz_kext_max(int32_t v){ return v; }
WTZ_COOP_HOST int32_t wtz_kext_from_right(int32_t last, int32_t){ return last; }
#endif

/* 32 bases [b0, b0 + 32) of a view of qlen bases, base b0 + k at bits 2k; b0 may be negative or beyond the end (such bases read as 0) */
WTZ_HD uint64_t wtz_kext_bases(const wtz_seq_packed &s, int32_t b0, int32_t len){
	if(b0 >= 0) return wtz_pack32(s, b0, len);
	if(b0 <= -32) return 0ull;
	return wtz_pack32(s, 0, len) << (2 * (-b0));
}

/* C slots per lane on 64 lanes; the one lane of the emulation holds all 64 * C */
template<int C>
WTZ_HD void wtz_kext_problem(const wtz_kextprob_t &p, const wtz_kextsc_t &S, wtz_kextres_t &r){
	constexpr int CL = C * (64 / WTZ_LOC_LANES), NW = (CL + 31) / 32;
	const int32_t lane = (int32_t)WTZ_LANE, s0 = lane * CL;
	const int32_t qlen = (int32_t)wtz_coop_bcast32((uint32_t)p.qlen), tlen = (int32_t)wtz_coop_bcast32((uint32_t)p.tlen), h0 = (int32_t)wtz_coop_bcast32((uint32_t)p.h0);
	const int32_t w = (int32_t)wtz_coop_bcast32((uint32_t)p.w), dlo = (int32_t)wtz_coop_bcast32((uint32_t)p.dlo);
	const int32_t Mm = S.M, X = S.X, e_del = S.e_del, e_ins = S.e_ins, oe_del = S.o_del + S.e_del, oe_ins = S.o_ins + S.e_ins, zdrop = S.zdrop;
	int32_t H[CL], E[CL];
	uint64_t qw[NW + 1];
	/* row -1 as the slots of row 0 see it: slot s = column s - dlo */
	#pragma unroll
	for(int k = 0; k < CL; k++){
		const int32_t j = s0 + k - dlo;
		const long long v = (long long)h0 - S.o_ins - (long long)e_ins * j;
		H[k] = j <= 0 ? h0 : (v > 0 ? (int32_t)v : 0);
		E[k] = 0;
	}
	#pragma unroll
	for(int n = 0; n < NW; n++) qw[n] = wtz_kext_bases(p.q, s0 - dlo + 32 * n, qlen);
	qw[NW] = 0;
	uint64_t qpre = wtz_kext_bases(p.q, s0 - dlo + 32 * NW, qlen);
	uint64_t tcur = 0, tnext = wtz_pack32(p.t, 0, tlen);
	int32_t beg = 0, end = qlen, mx = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0;
	uint32_t rows = 0; unsigned long long cells = 0;
	for(int32_t i = 0; i < tlen; i++){
		if((i & 31) == 0){      /* the words loaded 32 rows ago come into use, the next are requested */
			tcur = tnext; tnext = wtz_pack32(p.t, i + 32, tlen);
			qw[NW] = qpre; qpre = wtz_kext_bases(p.q, s0 - dlo + i + 32 * NW + 32, qlen);
		}
		const uint32_t tb = (uint32_t)(tcur >> (2 * (i & 31))) & 3u;
		int32_t h1;
		{ const long long v = (long long)h0 - S.o_del - (long long)e_del * (i + 1); h1 = v > 0 ? (int32_t)v : 0; }
		if(beg < i - w) beg = i - w;
		if(end > i + w + 1) end = i + w + 1;
		if(end > qlen) end = qlen;
		const int32_t off = i - dlo;                                      /* column of slot s: s + off */
		const int32_t lo = beg - off - s0, hi = end - off - s0;           /* the lane's live slots: lo <= k < hi */
		rows++; cells += (unsigned long long)(end > beg ? end - beg : 0);
		/* ---- pass 1: M in place, the lane's F aggregate ---- */
		int32_t agg = WTZ_KEXT_NEG;
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
					int32_t g = m - oe_ins; g = g > 0 ? g : 0; g += e_ins * (k + 1);      /* + e_ins * s0, the same for all of the lane's slots: added once below */
					g = g > agg ? g : agg;
					agg = (k >= lo && k < hi) ? g : agg;
				}
			}
		}
		/* ---- F carry from the lanes to the left ---- */
		int32_t f;
		{ const int32_t cin = wtz_kext_scan_excl(agg + e_ins * s0, WTZ_KEXT_NEG) - e_ins * s0; f = cin > 0 ? cin : 0; }
		/* ---- pass 2: the cells ---- */
		int32_t lm = -1, e0 = 0;
		#pragma unroll
		for(int k = 0; k < CL; k++){
			const bool live = k >= lo && k < hi;
			const int32_t m = H[k], e = E[k];
			int32_t h = m > e ? m : e; h = h > f ? h : f;
			int32_t t = m - oe_del; t = t > 0 ? t : 0;
			int32_t en = e - e_del; en = en > t ? en : t;
			int32_t g = m - oe_ins; g = g > 0 ? g : 0;
			int32_t fn = f - e_ins; fn = fn > g ? fn : g;
			H[k] = live ? h : h1;
			f = live ? fn : 0;
			en = live ? en : 0;
			lm = (live && h > lm) ? h : lm;
			if(k == 0) e0 = en; else E[k - 1] = en;
		}
		E[CL - 1] = wtz_kext_from_right(0, e0);
		int32_t m = wtz_kext_max(lm); m = m > 0 ? m : 0;
		/* ---- the column loop ended at j == qlen (an empty band ends at j = beg): gscore from H(i, end-1) ---- */
		if((beg < end ? end : beg) == qlen){
			int32_t h1e = h1;
			if(beg < end){
				int32_t sel = -1;
				#pragma unroll
				for(int k = 0; k < CL; k++) sel = (k == hi - 1) ? H[k] : sel;
				h1e = wtz_kext_max(sel);
			}
			max_ie = gscore > h1e ? max_ie : i;
			gscore = gscore > h1e ? gscore : h1e;
		}
		if(m == 0) break;
		/* ---- last slot holding m, nearest zero on either side of it ---- */
		int32_t la = -1;
		#pragma unroll
		for(int k = 0; k < CL; k++) la = (k >= lo && k < hi && H[k] == m) ? s0 + k : la;
		const int32_t smj = wtz_kext_max(la), mj = smj + off;
		int32_t zl = -1, zr = -1;
		#pragma unroll
		for(int k = 0; k < CL; k++){
			const bool z = k >= lo && k < hi && H[k] == 0;
			zl = (z && s0 + k < smj) ? s0 + k : zl;
			zr = (z && s0 + k > smj && zr < 0) ? 0x7FFFFFFF - (s0 + k) : zr;
		}
		zl = wtz_kext_max(zl); zr = wtz_kext_max(zr);
		if(m > mx){
			mx = m; max_i = i; max_j = mj;
			const int32_t d = mj > i ? mj - i : i - mj;
			max_off = max_off > d ? max_off : d;
		} else if(zdrop > 0){
			if(i - max_i > mj - max_j){ if(mx - m - ((i - max_i) - (mj - max_j)) * e_del > zdrop) break; }
			else { if(mx - m - ((mj - max_j) - (i - max_i)) * e_ins > zdrop) break; }
		}
		const int32_t nbeg = zl >= 0 ? zl + off + 2 : (h1 == 0 ? beg + 1 : beg);
		const int32_t nend = zr >= 0 ? (0x7FFFFFFF - zr) + off + 1 : end + 1;
		beg = nbeg; end = nend;
		/* the query moves one column to the left in the frame */
		#pragma unroll
		for(int n = 0; n < NW; n++) qw[n] = (qw[n] >> 2) | (qw[n + 1] << 62);
		qw[NW] >>= 2;
	}
	r.score = mx; r.qle = max_j + 1; r.tle = max_i + 1; r.gtle = max_ie + 1; r.gscore = gscore; r.max_off = max_off; r.rows = rows; r.cells = cells;
}

#if defined(__HIPCC__) && !defined(WTZ_EMUL)
/* resident waves per SIMD the instantiations are compiled for */
#ifndef WTZ_KEXT_OCC
#define WTZ_KEXT_OCC(C) ((C) <= 2 ? 8 : ((C) <= 4 ? 6 : ((C) <= 8 ? 4 : ((C) <= 16 ? 3 : 2))))
#endif
/* block b = one wavefront = problem order[b] (largest first); every problem of a launch has wtz_kext_form(slots) == C */
template<int C>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WTZ_KEXT_OCC(C), 8)))
wtz_kernel_kext(const wtz_kextprob_t *pr, const uint32_t *order, uint32_t n, wtz_kextsc_t S, wtz_kextres_t *res){
	if(blockIdx.x >= n) return;
	const uint32_t id = order[blockIdx.x];
	const wtz_kextprob_t p = pr[id];
	wtz_kextres_t r;
	wtz_kext_problem<C>(p, S, r);
	if(WTZ_LANE == 0) res[id] = r;
}
#endif
#endif
