/*
 * K-local: ksw_align2(..., KSW_XSTART) with 16-bit lanes (ksw.c:344-366 over ksw_i16, ksw.c:233-335) - the full, unbanded local
 * Smith-Waterman with start coordinates that wtcyc, pairaln (through kswx_align*, kswx.h:1495-1520) and wtcns (wtcns.c:209, 269) start from.
 * One wavefront per problem; the same body runs with ONE lane in the host emulation (tests/emul), where it is the CPU restatement that
 * tests/test_local_cpu.py pins against the reference routine itself.
 *
 * What the reference computes (ksw_i16; `adds` = signed 16-bit saturating addition, ceiling 32767):
 *     H(i,j)   = max{ adds(H(i-1,j-1), S(t_i,q_j)), E(i,j), F(i,j) }
 *     E(i+1,j) = max{ E(i,j) - e_del, H(i,j) - (o_del + e_del), 0 }        (unsigned saturating subtractions: the floor at 0)
 *     F(i,j+1) = max{ F(i,j) - e_ins, H(i,j) - (o_ins + e_ins), 0 }
 * row -1 and column -1 are 0; score = the maximum, te = the smallest row whose maximum reaches it (strict >, ksw.c:308), qe = the smallest column
 * that holds that row's maximum (ksw.c:320-322).  Its striped loop feeds E from H BEFORE the lazy-F correction (ksw.c:277-280): an insertion run
 * followed by a deletion run is never opened from there, but the deletion-then-insertion path through the opposite corner of the same rectangle has
 * the same score and is seen, so H equals the plain recurrence above.  The zero-score cells that pad the query to a multiple of eight lanes
 * (ksw_qinit) hold only values that a real cell of a smaller column or an earlier row holds too: they tie, and never win qe or te.
 * Both points are checked, not assumed: tests/test_local_cpu.py compares this body with live ksw_align2 on 2 000 gap-rich pairs.
 * A score of 0 (no equal base pair) leaves te = -1, qe = 0 and, through the second pass on a one-base query, tb = qb = 0.
 *
 * Second pass (ksw.c:358-364): the same DP on the reversed q[0..qe] and the reversed t[0..te], stopped at the first row whose maximum reaches
 * `score` (KSW_XSTOP, ksw.c:312); (te', qe') = that row and the smallest column holding its maximum; tb = te - te', qb = qe - qe' when that maximum
 * equals `score`, else both stay -1.  The reference hands the whole target to this pass, but the first (te + 1) rows always contain the reversed
 * optimal path, whose prefix scores reach `score` before any cell saturates: the pass is bounded to (te + 1) x (qe + 1) here.
 *
 * Device form: anti-diagonal over LANES, no scan.  The query is cut into strips of 64*C columns; lane l owns C consecutive columns of the strip in
 * registers (H of the previous row, E) and computes row k - l in step k, its C cells one after the other (the F chain is a register chain).  What a
 * row needs from the left - H(i, c-1), F(i, c) and the row's target base - is ONE 32-bit word (15 + 15 + 2 bits) that moves one lane to the right per
 * step with a DPP wave_shr:1; lane 0 takes the word from the strip boundary instead: H / F of the last column of the strip before (written by lane
 * 63, 64 rows per coalesced store, to a per-problem buffer in the scratch pool; two buffers alternate between strips) joined with the base, 64 rows
 * per load, one block ahead of its use.  32-bit arithmetic with an explicit ceiling: all values are in [-128, 32767].
 * Arg-max: a lane keeps the maximum of each row's cells (one v_max per cell) and only when that beats its best so far - a key (value, -row), or
 * (-row, value) for cells >= stop in the second pass - looks for the first column holding it; lanes and strips are merged by (key, smallest column).
 * The second pass lowers its row bound after every strip to the best row found so far (rows beyond cannot win); the result does not depend on it.
 */
#ifndef WTZ_SW_LOCAL_H
#define WTZ_SW_LOCAL_H

#include "wtz_sw.h"

#define WTZ_LOC_MAXLEN 65535          /* rows and columns of one problem: the row index shares a 32-bit key with the 15-bit score */
#define WTZ_LOC_NOSTOP 0x10000        /* ksw.c:250: endsc without KSW_XSTOP */
#define WTZ_LOC_SMALL_COLS 256        /* up to here four columns per lane (one strip on the device), beyond it sixteen */
/* lanes of the wavefront that runs a problem, as a constant the HOST code of the same build can use too (WTZ_NLANES is 1 in hipcc's host pass):
 * 64 in the device library, 1 in the host emulation */
#if defined(__HIPCC__) && !defined(WTZ_EMUL)
#define WTZ_LOC_LANES 64
#else
#define WTZ_LOC_LANES 1
#endif
#if defined(__HIP_DEVICE_COMPILE__)
static_assert(WTZ_NLANES == WTZ_LOC_LANES, "the host plans the strip boundaries for the device's strip width");
#endif

typedef struct { wtz_seq_packed q, t; int32_t qlen, tlen; unsigned long long bnd_off; } wtz_locprob_t;      /* bnd_off: first of the problem's 2 * tlen boundary words */
typedef struct { int32_t score, te, qe, tb, qb; uint32_t form; unsigned long long cells; } wtz_locres_t;
typedef struct { int32_t M, X, oe_del, e_del, oe_ins, e_ins; } wtz_locsc_t;

/* columns per lane / per strip of a pass over qlen columns; a pass of more than one strip needs the 2 * tlen boundary words */
WTZ_HD int32_t wtz_loc_form(int32_t qlen){ return qlen <= WTZ_LOC_SMALL_COLS ? 4 : 16; }
WTZ_HD int32_t wtz_loc_strip_cols(int32_t qlen){ return WTZ_LOC_LANES * wtz_loc_form(qlen); }

#if defined(__HIP_DEVICE_COMPILE__)
/* value of the lane to the left; lane 0 gets `first` (all lanes must be active) */
WTZ_D uint32_t wtz_loc_from_left(uint32_t first, uint32_t v){ return (uint32_t)__builtin_amdgcn_update_dpp((int32_t)first, (int32_t)v, 0x138, 0xF, 0xF, false); }
WTZ_D unsigned long long wtz_loc_max64(unsigned long long v){
	for(int d = 32; d > 0; d >>= 1){
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
		const unsigned long long o = ((unsigned long long)hi << 32) | lo;
		v = o > v ? o : v;
	}
	return wtz_coop_bcast64(v);
}
#else
WTZ_COOP_HOST uint32_t wtz_loc_from_left(uint32_t first, uint32_t){ return first; }
WTZ_COOP_HOST unsigned long long wtz_loc_max64(unsigned long long v){ return v; }
#endif

/* one pass over rows [0, tlen) x columns [0, qlen); stop = WTZ_LOC_NOSTOP: first pass (score, te, qe as ksw_i16 leaves them), else the second pass: the
 * first row holding a value >= stop, that row's maximum and its first column (score = 0: no such row).  bnd: 2 * tlen words, touched only when the
 * query has more than one strip.  Every lane returns the same result. */
template<int C>
WTZ_HD void wtz_local_pass(const wtz_seq_packed &q, const int32_t qlen, const wtz_seq_packed &t, const int32_t tlen, const wtz_locsc_t &S, const int32_t stop,
		uint32_t *bnd, int32_t &score, int32_t &te, int32_t &qe, unsigned long long &cells){
	const int32_t NL = (int32_t)WTZ_NLANES, SW = NL * C, lane = (int32_t)WTZ_LANE;
	const bool stopm = stop < WTZ_LOC_NOSTOP;
	const int32_t M = S.M, X = S.X, oe_del = S.oe_del, e_del = S.e_del, oe_ins = S.oe_ins, e_ins = S.e_ins;
	uint32_t bestkey = stopm ? 0u : 0xFFFFu; int32_t bestcol = 0;      /* first pass: (0, row -1) - a zero cell never beats it */
	int32_t rows = tlen;
	const int32_t nstrip = (qlen + SW - 1) / SW;
	for(int32_t s = 0; s < nstrip; s++){
		const int32_t left = qlen - s * SW;                                /* columns from the strip's first one on */
		const int32_t c0 = s * SW + lane * C;
		const int32_t ncol = qlen - c0 < 0 ? 0 : (qlen - c0 < C ? qlen - c0 : C);
		const int32_t nact = left >= SW ? NL : (left + C - 1) / C;        /* lanes of the strip that own a column */
		const bool more = s + 1 < nstrip;                                 /* then nact = NL and the last lane writes the boundary */
		const uint32_t *bin = bnd + (size_t)(s & 1) * (size_t)tlen; uint32_t *bout = bnd + (size_t)((s + 1) & 1) * (size_t)tlen;
		int32_t qb[C], H[C], E[C];
		{
			const uint64_t qw = ncol > 0 ? wtz_pack32(q, c0, qlen) : 0ull;
			#pragma unroll
			for(int j = 0; j < C; j++){ qb[j] = j < ncol ? (int32_t)((qw >> (2 * j)) & 3u) : 4; H[j] = 0; E[j] = 0; }
		}
		int32_t dsave = 0; uint32_t msg_out = 0, outblk = 0;
		const int32_t nsteps = rows + nact - 1;
		auto load_in = [&](const int32_t r) -> uint32_t { return r < rows ? ((s > 0 ? bin[r] : 0u) | (t.at(r) << 30)) : 0u; };
		uint32_t nxt = load_in(lane);
		for(int32_t k0 = 0; k0 < nsteps; k0 += NL){
			const uint32_t cur = nxt;
			nxt = load_in(k0 + NL + lane);                                 /* a block ahead: its latency hides behind NL steps */
			const int32_t kend = nsteps - k0 < NL ? nsteps - k0 : NL;
			for(int32_t kk = 0; kk < kend; kk++){
				const int32_t k = k0 + kk, i = k - lane;
				const uint32_t msg = wtz_loc_from_left(wtz_coop_lane32(cur, (uint32_t)kk), msg_out);
				if(i >= 0 && i < rows && ncol > 0){
					const int32_t tb = (int32_t)(msg >> 30);
					int32_t f = (int32_t)((msg >> 15) & 0x7FFFu), diag = dsave, m = 0;
					dsave = (int32_t)(msg & 0x7FFFu);
					#pragma unroll
					for(int j = 0; j < C; j++){
						const int32_t d = diag + (qb[j] == tb ? M : X);
						diag = H[j];
						int32_t h = d > E[j] ? d : E[j]; h = h > f ? h : f; h = h < 32767 ? h : 32767;
						H[j] = h; m = m > h ? m : h;
						int32_t e = E[j] - e_del, e2 = h - oe_del; e = e > e2 ? e : e2; E[j] = e > 0 ? e : 0;
						int32_t g = f - e_ins, g2 = h - oe_ins; g = g > g2 ? g : g2; f = g > 0 ? g : 0;
					}
					msg_out = (uint32_t)H[C - 1] | ((uint32_t)f << 15) | ((uint32_t)tb << 30);
					const uint32_t rc = 0xFFFEu - (uint32_t)i;
					const uint32_t key = stopm ? (m >= stop ? ((rc << 16) | (uint32_t)m) : 0u) : (((uint32_t)m << 16) | rc);
					if(key > bestkey){
						int32_t col = 0;
						#pragma unroll
						for(int j = C - 1; j >= 0; j--) col = H[j] == m ? j : col;
						bestkey = key; bestcol = c0 + col;
					}
				}
				if(more){
					const int32_t il = k - (NL - 1);                          /* the row the last lane has just finished */
					if(il >= 0){
						const uint32_t v = wtz_coop_lane32(msg_out, (uint32_t)(NL - 1));
						if(lane == (il & (NL - 1))) outblk = v & 0x3FFFFFFFu;
						if((il & (NL - 1)) == NL - 1 || il == rows - 1){
							const int32_t r = (il & ~(NL - 1)) + lane;
							if(r <= il) bout[r] = outblk;
						}
					}
				}
			}
		}
		cells += (unsigned long long)rows * (unsigned long long)(left < SW ? left : SW);
		WTZ_WAVE_SYNC();                                                   /* the boundary words are read by other lanes in the next strip */
		if(stopm && more){
			const uint32_t bk = (uint32_t)(wtz_loc_max64((unsigned long long)bestkey));
			if(bk){ const int32_t r1 = (int32_t)(0xFFFEu - (bk >> 16)) + 1; rows = r1 < rows ? r1 : rows; }
		}
	}
	const unsigned long long fin = wtz_loc_max64(((unsigned long long)bestkey << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)bestcol));
	const uint32_t fk = (uint32_t)(fin >> 32);
	qe = (int32_t)(0xFFFFFFFFu - (uint32_t)fin);
	if(stopm){ score = (int32_t)(fk & 0xFFFFu); te = fk ? (int32_t)(0xFFFEu - (fk >> 16)) : -1; }
	else { score = (int32_t)(fk >> 16); te = (int32_t)0xFFFE - (int32_t)(fk & 0xFFFFu); }
}

/* the last n bases of a view's first n, walked backwards */
WTZ_HD wtz_seq_packed wtz_loc_reversed(const wtz_seq_packed &s, int32_t n){
	wtz_seq_packed r; r.bits = s.bits; r.start = s.start + (int64_t)(n - 1) * s.strand; r.strand = -s.strand; r.comp = s.comp; return r;
}

/* ksw_align2(qlen, q, tlen, t, ..., KSW_XSTART) of one problem (1 <= qlen, tlen <= WTZ_LOC_MAXLEN).  form = columns per lane of the first pass. */
WTZ_HD void wtz_local_problem(const wtz_locprob_t &p, const wtz_locsc_t &S, uint32_t *bnd_base, wtz_locres_t &r){
	uint32_t *bnd = bnd_base + p.bnd_off;
	r.cells = 0; r.tb = -1; r.qb = -1;
	if(p.qlen <= WTZ_LOC_SMALL_COLS){ r.form = 4; wtz_local_pass<4>(p.q, p.qlen, p.t, p.tlen, S, WTZ_LOC_NOSTOP, bnd, r.score, r.te, r.qe, r.cells); }
	else { r.form = 16; wtz_local_pass<16>(p.q, p.qlen, p.t, p.tlen, S, WTZ_LOC_NOSTOP, bnd, r.score, r.te, r.qe, r.cells); }
	if(r.score <= 0){ r.tb = 0; r.qb = 0; return; }      /* te = -1, qe = 0: the second pass sees one query base, no target row and a stop score of 0 (ksw.c:358-364) */
	const wtz_seq_packed rq = wtz_loc_reversed(p.q, r.qe + 1), rt = wtz_loc_reversed(p.t, r.te + 1);
	int32_t sc2 = 0, te2 = -1, qe2 = 0;
	if(r.qe + 1 <= WTZ_LOC_SMALL_COLS) wtz_local_pass<4>(rq, r.qe + 1, rt, r.te + 1, S, r.score, bnd, sc2, te2, qe2, r.cells);
	else wtz_local_pass<16>(rq, r.qe + 1, rt, r.te + 1, S, r.score, bnd, sc2, te2, qe2, r.cells);
	if(sc2 == r.score){ r.tb = r.te - te2; r.qb = r.qe - qe2; }
}

#if defined(__HIPCC__) && !defined(WTZ_EMUL)
#ifndef WTZ_OCC_LOCAL
#define WTZ_OCC_LOCAL 4
#endif
/* block b = one wavefront = problem order[b] (largest first) */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WTZ_OCC_LOCAL, 8)))
wtz_kernel_local(const wtz_locprob_t *pr, const uint32_t *order, uint32_t n, wtz_locsc_t S, uint32_t *bnd_base, wtz_locres_t *res){
	if(blockIdx.x >= n) return;
	const uint32_t id = order[blockIdx.x];
	const wtz_locprob_t p = pr[id];
	wtz_locres_t r;
	wtz_local_problem(p, S, bnd_base, r);
	if(WTZ_LANE == 0) res[id] = r;
}
#endif
#endif
