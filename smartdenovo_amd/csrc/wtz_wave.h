/*
 * wtz_wave.h — what every one-wavefront-per-problem DP shares (wtz_sw_shift.h, wtz_sw_fixed.h, wtz_sw_global.h, wtz_sw_refine.h,
 * the frame forms, the lane pipelines' reductions):
 *     the DPP lane moves, the exclusive max scan and the max / arg-max reductions (no LDS round trip);
 *     wtz_f_carry, the carry-in of F of a lane's first column from the scanned lane aggregates;
 *     wtz_wave_lds_t, the LDS view of a ring DP, and wtz_wave_fits;
 *     wtz_trace_t / wtz_trace_prepare, the pool-resident trace of the ring forms, carved 64 rows at a time;
 *     wtz_cigw_*, the lane-0 CIGAR writer with its open run in a register;
 *     wtz_static_for and wtz_mad24 for the forms that keep whole rows in registers.
 * Nothing here restates a routine of the reference; the recurrence the scan serves is described in wtz_sw_shift.h.
 */
#ifndef WTZ_WAVE_H
#define WTZ_WAVE_H

#include "wtz_sw.h"

#ifdef __HIPCC__

#define WTZ_TRACE_MAXCHUNK 1024          /* 64-row chunks: up to 65536 rows per problem */

/* reusable trace storage of one task (pointers live in the pool so that lane 0 can chase them during traceback) */
typedef struct { uint8_t **chunk; int32_t *zb; uint32_t n_chunk, zrow, cap_rows; } wtz_trace_t;

/* LDS view handed to the wave DP: rings of PM+1 ints (PM = size-1 mask), target buffer of tw 64-bit words */
typedef struct { int32_t *Hs, *Es; uint64_t *tb; int32_t PM; int32_t tw; uint32_t *qw; } wtz_wave_lds_t;      /* qw: 512 B for the query words of the K-sw1 traceback (only wtz_fixed_problem_wave reads it) */

/* ---- wavefront-wide max scan / arg-max reduction on the DPP data path (no LDS round trip) ----
 * gfx9-family DPP controls: row_shr:n = 0x110+n (inside a row of 16 lanes), row_bcast:15 = 0x142 (lane 15 of each row to
 * the next row), row_bcast:31 = 0x143 (lane 31 to rows 2-3), wave_shr:1 = 0x138.  Lanes without a source keep `old`. */
template<int CTRL, int ROWMASK>
WTZ_D int32_t wtz_dpp_mov(int32_t old, int32_t src){ return __builtin_amdgcn_update_dpp(old, src, CTRL, ROWMASK, 0xF, false); }

/* neighbour lane's value: wave_shl:1 = from lane+1, wave_shr:1 = from lane-1; the edge lane keeps `old` */
WTZ_D int32_t wtz_dpp_wave_shl1(int32_t old, int32_t src){ return __builtin_amdgcn_update_dpp(old, src, 0x130, 0xF, 0xF, false); }
WTZ_D int32_t wtz_dpp_wave_shr1(int32_t old, int32_t src){ return __builtin_amdgcn_update_dpp(old, src, 0x138, 0xF, 0xF, false); }

/* exclusive prefix maximum over the lanes; lane 0 gets `ident`.  The inclusive steps give a lane without a source INT_MIN, the
 * identity of max (every caller's values are >= ident > INT_MIN, so the result is the same as with `ident`): the compiler's DPP
 * combiner then folds each step into ONE v_max_i32_dpp instead of v_mov (ident) + v_mov_dpp + v_max - 12 VALU ops less per DP
 * row of every register DP */
WTZ_D int32_t wtz_wave_max_scan_excl(int32_t v, int32_t ident){
	const int32_t mn = (int32_t)0x80000000;
	int32_t x = v, t;
	t = wtz_dpp_mov<0x111, 0xF>(mn, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x112, 0xF>(mn, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x114, 0xF>(mn, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x118, 0xF>(mn, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x142, 0xA>(mn, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x143, 0xC>(mn, x); x = x > t ? x : t;
	return wtz_dpp_mov<0x138, 0xF>(ident, x);              /* inclusive -> exclusive: shift the whole wave by one lane */
}

/* carry-in of F for the lane's first column: `agg` is the lane's aggregate max_k(m_k + open + (C-k)*e) over its C columns, CE = C*e (e <= 0);
 * the scan runs over agg - lane*CE so that one max serves every distance; F at the band's first column is `sentinel`; `ident` is below every aggregate */
WTZ_D int32_t wtz_f_carry(int32_t agg, int lane, int32_t CE, int32_t ident, int32_t sentinel){
	const int32_t g = agg - lane * CE;
	const int32_t pm = wtz_wave_max_scan_excl(g, ident);
	const int32_t from_prev = (lane == 0) ? ident : pm + (lane - 1) * CE;
	const int32_t from_init = sentinel + lane * CE;
	return from_prev > from_init ? from_prev : from_init;
}

/* all-lanes maximum of an int32, result uniform */
WTZ_D int32_t wtz_wave_max_i32(int32_t v){
	const int32_t ident = (int32_t)0x80000000;
	int32_t x = v, t;
	t = wtz_dpp_mov<0x111, 0xF>(ident, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x112, 0xF>(ident, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x114, 0xF>(ident, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x118, 0xF>(ident, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x142, 0xA>(ident, x); x = x > t ? x : t;
	t = wtz_dpp_mov<0x143, 0xC>(ident, x); x = x > t ? x : t;
	return __builtin_amdgcn_readlane(x, 63);
}

/* all-lanes maximum of a signed 64-bit key (hi:int32 value, lo:uint32 tie-break), result in every lane */
WTZ_D void wtz_wave_max_key(int32_t &hi, uint32_t &lo){
	const int32_t ih = (int32_t)0x80000000; const int32_t il = 0;
#define WTZ_KEYSTEP(CTRL, RM) { const int32_t th = wtz_dpp_mov<CTRL, RM>(ih, hi); const uint32_t tl = (uint32_t)wtz_dpp_mov<CTRL, RM>(il, (int32_t)lo); \
	if(th > hi || (th == hi && tl > lo)){ hi = th; lo = tl; } }
	WTZ_KEYSTEP(0x111, 0xF) WTZ_KEYSTEP(0x112, 0xF) WTZ_KEYSTEP(0x114, 0xF) WTZ_KEYSTEP(0x118, 0xF) WTZ_KEYSTEP(0x142, 0xA) WTZ_KEYSTEP(0x143, 0xC)
#undef WTZ_KEYSTEP
	hi = __builtin_amdgcn_readlane(hi, 63); lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)lo, 63);
}

WTZ_D bool wtz_wave_fits(const wtz_wave_lds_t &L, int32_t n_col, int32_t tl, int32_t ql){
	return n_col + 2 <= L.PM + 1 && n_col <= 64 * 31 && (tl + 63) / 32 + 1 <= L.tw && (ql + 63) / 64 <= WTZ_TRACE_MAXCHUNK;
}

WTZ_D wtz_aln_t wtz_bcast_aln(wtz_aln_t x){
	wtz_aln_t r;
	r.score = __shfl(x.score, 0, 64); r.tb = __shfl(x.tb, 0, 64); r.te = __shfl(x.te, 0, 64); r.qb = __shfl(x.qb, 0, 64); r.qe = __shfl(x.qe, 0, 64);
	r.aln = __shfl(x.aln, 0, 64); r.mat = __shfl(x.mat, 0, 64); r.mis = __shfl(x.mis, 0, 64); r.ins = __shfl(x.ins, 0, 64); r.del = __shfl(x.del, 0, 64);
	return r;
}

/* make sure the trace has chunks for `zrow`-byte rows; lane 0 allocates, everybody learns the table address.
 * returns false on pool exhaustion (uniform) */
WTZ_D bool wtz_trace_prepare(wtz_trace_t &tr, wtz_pool_t *pool, uint32_t zrow, int32_t ql, bool need_zb){
	const int lane = (int)(threadIdx.x & 63);
	if(tr.chunk == NULL || tr.zrow != zrow){
		unsigned long long a = 0;
		if(lane == 0) a = (unsigned long long)(uintptr_t)wtz_pool_alloc(pool, (size_t)WTZ_TRACE_MAXCHUNK * 8);
		a = __shfl(a, 0, 64);
		tr.chunk = (uint8_t**)(uintptr_t)a; tr.n_chunk = 0; tr.zrow = zrow;
		if(tr.chunk == NULL) return false;
	}
	if(need_zb && (tr.zb == NULL || tr.cap_rows < (uint32_t)ql + 2)){
		unsigned long long a = 0;
		if(lane == 0) a = (unsigned long long)(uintptr_t)wtz_pool_alloc(pool, (size_t)(ql + 2) * 4);
		a = __shfl(a, 0, 64);
		tr.zb = (int32_t*)(uintptr_t)a; tr.cap_rows = (uint32_t)ql + 2;
		if(tr.zb == NULL) return false;
	}
	return true;
}

/* lane-0 CIGAR writer: the open run stays in a register, so appending never reads memory back (kswx_push_cigar merges) */
typedef struct { wtz_cigar_t *v; uint32_t tail; } wtz_cigw_t;
WTZ_D void wtz_cigw_push(wtz_cigw_t &w, uint32_t op, uint32_t len){
	if(len == 0) return;
	if(w.tail && (w.tail & 0xFu) == op) w.tail += len << 4;
	else { if(w.tail) w.v->push(w.tail); w.tail = (len << 4) | op; }
}
WTZ_D void wtz_cigw_finish(wtz_cigw_t &w){ if(w.tail){ w.v->push(w.tail); w.tail = 0; } }

/* ---- building blocks of the K-sw3 forms that keep the DP rows entirely in registers (wtz_sw_frame.h, wtz_sw_frame16.h; wtz_extend_shift_wave_rt in wtz_sw_shift.h is
 * their fallback and on-device cross-check) ---- */
template<int V> struct wtz_ic { static constexpr int value = V; };
template<int I, int N, typename F> WTZ_D void wtz_static_for(F &&f){ if constexpr(I < N){ f(wtz_ic<I>{}); wtz_static_for<I + 1, N>(f); } }
/* a*b + c with 24-bit a, b in ONE VALU op; the asm keeps the compiler from turning a 0/1 factor into compare+select or from
 * hoisting the (wave-uniform) product into a scalar register per cell */
WTZ_D int32_t wtz_mad24(int32_t a, int32_t b, int32_t c){ int32_t r; asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

#endif /* __HIPCC__ */
#endif
