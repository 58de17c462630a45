/*
 * wtz_sw_shift.h — K-sw3, kswx_extend_align_shift_core (kswx.h:101-232: the band follows the row arg-max), one 64-lane wavefront per problem:
 *     wtz_extend_shift_wave_rt   the ring form: rows handed over through LDS rings, a lane's block of the row in registers;
 *     wtz_shift_traceback        the walker of the frame forms' trace (wtz_sw_frame.h, wtz_sw_frame16.h) with wtz_tb_solve;
 *     wtz_kernel_extjobs         one wave per extension job: the ring form, or the scalar body for what does not fit the rings;
 *     wtz_extjob_t               the job record (host and device).
 *
 * Why row-wise and not anti-diagonal: in K-sw3 the band centre of row i+1 depends on the arg-max of row i
 * (kswx.h:186-199), so rows are inherently sequential; inside a row, however, the reference's recurrence opens
 * gaps from m (the diagonal value), not from H:
 *        m_j = H(i-1,j-1) + S          E'_j = max(E_j + e, m_j + I + e)        F_{j+1} = max(F_j + e, m_j + D + e)
 * so F along the row is a max-plus prefix scan of values that depend on the previous row only, exact in int32.
 * A row is therefore: (1) every lane computes m for its C consecutive columns and a local scan aggregate,
 * (2) one 6-step cross-lane max-scan over the 64 lane aggregates gives each lane its carry-in (wtz_f_carry), (3) every lane
 * finishes H / E' / F / trace bits for its columns, (4) a 6-step (value, column) reduction yields the row maximum
 * and its arg-max (FIRST for K-sw3, LAST for K-sw1: kswx.h:172 vs 288-289), which moves the K-sw3 band.
 * The ring forms of K-sw2 (wtz_global_wave) and of the refinement (wtz_refine_wave) run the same row.
 *
 * Data layout (per wave, LDS): Hs[P], Es[P] int32 rings indexed by absolute column & (P-1) (P >= band+2); lanes own
 * column blocks of odd width C so the stride-C ds_read/ds_write are bank-conflict free; the target segment is staged
 * once as 2-bit codes in logical order (strand / complement resolved) so that a lane fetches its <= 31 bases with two
 * ds_read_b64.  Trace bytes go to HBM in a lane-transposed layout (row, kk/4, lane, kk%4): each of the ceil(C/4)
 * stores per row writes 256 contiguous bytes; rows are carved from the pool 64 at a time (most extensions stop long
 * before ql rows).
 * Semantics reproduced exactly: -10000 sentinels outside the band, H(i,-1)/H(-1,j) boundary values, the FIRST arg-max of a
 * row, gmax/max end rule with T, early exit when a row maximum is <= 0, the per-row band start.
 */
#ifndef WTZ_SW_SHIFT_H
#define WTZ_SW_SHIFT_H

#include "wtz_wave.h"

typedef struct {
	wtz_seq_packed q, t;        /* logical views: index 0 is the base next to the seed, walking outwards */
	int32_t qlen, tlen, init_score, W;      /* W as passed to kswx_extend_align_shift_core (negative = exact band) */
	uint32_t item;              /* owner (stitch item) */
	uint32_t valid;             /* 0: nothing to do */
	uint32_t done;              /* set by the register-DP kernel; the general kernel then skips the job */
	/* results */
	wtz_aln_t x; uint32_t *cigar; uint32_t cigar_len; int32_t bad; unsigned long long cells;
} wtz_extjob_t;

#ifdef __HIPCC__

/*
 * K-sw3, register-tiled rows.  The row of the file header; a lane keeps its block of the
 * previous row (H and E of <= CMAX columns) in VGPRs: per row it issues all its LDS reads back to back (one
 * latency), computes m / F-scan / H / E' / trace entirely in registers, and issues all LDS writes back to back.
 * The LDS rings are only the hand-over medium between rows (the band moves, so column ownership changes).
 * This cuts the row latency - which is what bounds the longest extension of a batch - by the C dependent
 * ds_read -> ds_write round trips of the loop form.
 */
template<int CMAX, typename SQ, typename ST>
WTZ_D wtz_aln_t wtz_extend_shift_wave_rt(int32_t qlen, const SQ &query, int32_t tlen, const ST &target, int32_t init_score, int32_t W,
		int32_t M, int32_t X, int32_t I, int32_t D, int32_t E, int32_t T, const wtz_wave_lds_t &L, wtz_trace_t &tr, wtz_pool_t *pool,
		wtz_cigar_t &cigars, unsigned long long *cells, bool *ok){
	const int lane = (int)(threadIdx.x & 63);
	const int32_t PM = L.PM;
	wtz_aln_t x; memset(&x, 0, sizeof x);
	*ok = true;
	if(lane == 0) cigars.n = 0;
	if(init_score < 0) init_score = 0;
	if(qlen <= 0 || tlen <= 0){ x.score = init_score; return x; }
	int32_t ql, tl, n_col;
	wtz_ext_geometry(qlen, tlen, init_score, W, M, I, D, E, T, ql, tl, n_col);
	const int32_t C0 = (n_col + 63) / 64, C = (C0 | 1);
	const int32_t C4 = (C + 3) / 4;
	const uint32_t zrow = (uint32_t)C4 * 256u;
	if(!wtz_trace_prepare(tr, pool, zrow, ql, true)){ *ok = false; return x; }
	uint8_t **zchunk = tr.chunk; int32_t *zb = tr.zb;
	uint8_t *z = NULL;
	{
		const int32_t nw = (tl + 31) / 32 + 1;
		for(int32_t w = lane; w < nw; w += 64){
			uint64_t v = 0; const int32_t b0 = w * 32;
			for(int32_t k = 0; k < 32 && b0 + k < tl; k++) v |= ((uint64_t)target.at(b0 + k)) << (2 * k);
			L.tb[w] = v;
		}
	}
	int32_t mx = init_score, mi = -1, mj = -1, gmax = 0, gi = -1, gj = -1;
	int32_t jbp = 0, jep = 0, c = 0, i;
	unsigned long long ncell = 0;
	const int32_t CE = C * E;
	for(i = 0; i < ql; i++){
		if((i & 63) == 0){
			const uint32_t ci = (uint32_t)i >> 6;
			unsigned long long za = 0;
			if(ci < tr.n_chunk){ z = zchunk[ci]; }
			else {
				if(lane == 0){ uint8_t *p = (uint8_t*)wtz_pool_alloc(pool, (size_t)zrow * 64); zchunk[ci] = p; za = (unsigned long long)(uintptr_t)p; }
				za = __shfl(za, 0, 64);
				z = (uint8_t*)(uintptr_t)za;
				if(z == NULL){ *ok = false; break; }
				tr.n_chunk = ci + 1;
			}
		}
		int32_t jb = 0, je = tl;
		if(jb < c - W) jb = c - W;
		if(je > c + W + 1) je = c + W + 1;
		if(je > tl) je = tl;
		const uint32_t qbase = query.at(i);
		const int32_t j0 = jb + lane * C;
		uint64_t tbits;
		{
			const int32_t jj = j0 < tl ? j0 : (tl > 0 ? tl - 1 : 0);
			const int32_t w = jj >> 5, sh = (jj & 31) * 2;
			const uint64_t w0 = L.tb[w], w1 = L.tb[w + 1];
			tbits = sh ? ((w0 >> sh) | (w1 << (64 - sh))) : w0;
		}
		/* ---- load phase: previous-row H and E of the lane's columns, plus H(i-1, j0-1) ---- */
		int32_t hv[CMAX], ev[CMAX];
		int32_t pred0;
		if(i == 0) pred0 = (j0 == 0) ? init_score : init_score + D + E * j0;
		else if(j0 - 1 >= jbp && j0 - 1 < jep) pred0 = L.Hs[(j0 - 1) & PM];
		else pred0 = (j0 == 0) ? init_score + I + E * i : -10000;
		#pragma unroll
		for(int k = 0; k < CMAX; k++){
			const int32_t j = j0 + k;
			const bool live = (k < C) && (i > 0) && (j >= jbp) && (j < jep);
			hv[k] = live ? L.Hs[j & PM] : -10000;
			ev[k] = live ? L.Es[j & PM] : -10000;
		}
		/* ---- m in place (descending k: m_k needs the OLD H of column k-1) and the local F aggregate ---- */
		int32_t agg = -0x3FFFFFFF;
		#pragma unroll
		for(int k = CMAX - 1; k >= 0; k--){
			const int32_t j = j0 + k;
			int32_t pred;
			if(k == 0) pred = pred0;
			else pred = (i == 0) ? init_score + D + E * j : hv[k - 1];
			const uint32_t tbase = (uint32_t)(tbits >> (2 * k)) & 3u;
			const int32_t m = pred + ((qbase == tbase) ? M : X);
			hv[k] = m;
			if(k < C && j < je){ const int32_t cand = m + D + E + (C - 1 - k) * E; agg = agg > cand ? agg : cand; }
		}
		int32_t f = wtz_f_carry(agg, lane, CE, -0x3FFFFFFF, -10000);
		/* ---- H, E', F, trace in registers ---- */
		int32_t best = -0x7FFFFFFF, bestj = 0x7FFFFFFF, h_last = 0;
		uint32_t zw[(CMAX + 3) / 4];
		#pragma unroll
		for(int q4 = 0; q4 < (CMAX + 3) / 4; q4++) zw[q4] = 0;
		#pragma unroll
		for(int k = 0; k < CMAX; k++){
			const int32_t j = j0 + k;
			if(k < C && j < je){
				const int32_t m = hv[k];
				int32_t e = ev[k];
				uint32_t d; int32_t h;
				if(m >= e){ d = 0; h = m; } else { d = 1; h = e; }
				if(h < f){ d = 2; h = f; }
				if(h > best){ best = h; bestj = j; }
				h_last = h;
				int32_t t = m + I + E; e = e + E; if(e > t) d |= 1u << 2; else e = t;
				t = m + D + E; f = f + E; if(f > t) d |= 2u << 4; else f = t;
				hv[k] = h; ev[k] = e;
				if(qbase == ((uint32_t)(tbits >> (2 * k)) & 3u)) d |= 0x80u;       /* bit 7: bases equal (saves two sequence loads per traceback step) */
				zw[k >> 2] |= d << (8 * (k & 3));
			}
		}
		/* ---- store phase ---- */
		#pragma unroll
		for(int k = 0; k < CMAX; k++){
			const int32_t j = j0 + k;
			if(k < C && j < je){ L.Hs[j & PM] = hv[k]; L.Es[j & PM] = ev[k]; }
		}
		{
			uint32_t *zr = (uint32_t*)(z + (size_t)(i & 63) * zrow) + lane;
			#pragma unroll
			for(int q4 = 0; q4 < (CMAX + 3) / 4; q4++) if(q4 < C4) zr[(size_t)q4 * 64] = zw[q4];
		}
		ncell += (unsigned long long)(je - jb);
		{ uint32_t lo = 0x7FFFFFFFu - (uint32_t)bestj; wtz_wave_max_key(best, lo); bestj = (int32_t)(0x7FFFFFFFu - lo); }     /* max value, then smallest column */
		int32_t imax = 0, mj2 = -1;
		if(best > 0){ imax = best; mj2 = bestj; }
		const int32_t lastlane = (je - 1 - jb) / C;
		const int32_t h1 = __builtin_amdgcn_readlane(h_last, __builtin_amdgcn_readfirstlane(lastlane));
		if(lane == 0) zb[i] = jb;
		if(je == tlen && gmax < h1){ gmax = h1; gi = i; gj = je - 1; }
		if(i + 1 == qlen && gmax < imax){ gmax = imax; gi = i; gj = mj2; }
		jbp = jb; jep = je;
		if(imax > mx){ mx = imax; mi = i; mj = mj2; }
		else if(imax <= 0) break;
		c++; if(c < mj2) c++; else if(c > mj2) c--;
	}
	if(cells && lane == 0) *cells += ncell;
	if(!*ok) return x;
	if(gmax > 0 && gmax >= mx + T){ x.score = gmax; x.qe = gi; x.te = gj; }
	else { x.score = mx; x.qe = mi; x.te = mj; }
	__threadfence_block();     /* the trace was written by lanes of THIS wave: ordering inside the wave is enough (an agent-scope fence would write back the whole L2) */
	if(lane == 0){
		/* traceback: one dependent trace-byte load per step; the band start of the previous row is fetched alongside, the chunk
		 * base only every 64 rows, match/mismatch comes from bit 7 of the byte, the CIGAR run is kept in registers */
		int32_t i_ = x.qe, j_ = x.te; uint32_t d_ = 0;
		int32_t chunk_i = -1; const uint8_t *cbase = NULL;
		int32_t zbi = (i_ >= 0) ? zb[i_] : 0;
		uint32_t run_op = 0xFFu, run_len = 0;
		while(i_ >= 0 && j_ >= 0){
			if((i_ >> 6) != chunk_i){ chunk_i = i_ >> 6; cbase = zchunk[chunk_i]; }
			const int32_t col = j_ - zbi;
			const int32_t ln = col / C, kk = col - ln * C;
			const uint8_t zv = cbase[(size_t)(i_ & 63) * zrow + (size_t)(kk >> 2) * 256 + (size_t)ln * 4 + (kk & 3)];
			const int32_t zb_prev = (i_ > 0) ? zb[i_ - 1] : 0;
			d_ = (zv >> (d_ << 1)) & 0x03;
			if(d_ == 0){ if(zv & 0x80u) x.mat++; else x.mis++; i_--; j_--; zbi = zb_prev; }
			else if(d_ == 1){ i_--; x.ins++; zbi = zb_prev; }
			else { j_--; x.del++; }
			if(d_ == run_op) run_len++;
			else { if(run_len) wtz_cigar_push(cigars, run_op, run_len); run_op = d_; run_len = 1; }
		}
		if(run_len) wtz_cigar_push(cigars, run_op, run_len);
		if(i_ >= 0){ x.ins += i_ + 1; wtz_cigar_push(cigars, 1, (uint32_t)(i_ + 1)); }
		if(j_ >= 0){ x.del += j_ + 1; wtz_cigar_push(cigars, 2, (uint32_t)(j_ + 1)); }
		wtz_cigar_reverse(cigars.a, cigars.n);
		x.aln = x.mat + x.mis + x.ins + x.del; x.qe++; x.te++;
	}
	return wtz_bcast_aln(x);
}

/* ---- traceback of the K-sw3 register forms (one wavefront; NL = lanes of a trace row: 64).
 * The trace lives in the pool in the lane-transposed layout (row, k/4, lane, k%4).  Lane 0 walks, but never against HBM latency:
 * for the 64 rows below the current cell the wave copies the dwords of the NLW lanes around the current band-relative column
 * into LDS - one row per step, lane x takes dword (x / C4, x % C4) of the row, so a step is a few contiguous pieces and the loads
 * of eight rows are in flight together (the first version fetched byte by byte, each byte waiting for its own round trip: a 64-row
 * block cost more than the 64 DP rows it traces) - decoded four cells at a time into the walker's bytes, 128 bytes per row in
 * band-relative column order.  The walker tracks the band-relative column itself (a row's band start moves by 0..2 against the
 * row above: 64 deltas in LDS), leaves the block after 64 rows or through either edge of the window, and the next block is
 * staged around the cell it stands on.  Runs go through the register-tail writer and are reversed once at the end.
 * LDS: 8192 + 64 bytes at `tb` (the target words are dead by now).
 * The trace byte holds the four decisions only (bit 3 m<e, bit 2 max(m,e)<f, bit 1 E extended, bit 0 F extended; the "bases equal" bit of the round-4 register kernel
 * went with that kernel); the walk counts diagonal steps and gap runs, and matches / mismatches follow from the score: every gap run of the path was opened once (a run ends in the diagonal step
 * of the cell it was opened from - kswx.h:175-183 opens from m, not from H - so two runs never touch), hence
 *     score - init = M*mat + X*mis + runs*O + E*(ins + del),   mat + mis = diagonal steps.
 * With two opening costs (SP = true, wtz_set_gap_open with I != D) the argument is the same - every run, the two tails of the walk included, was opened once from m:
 * a run of query-only steps (op 1; the leftover rows at the end of the walk are one, kswx.h:220-223, opened by column -1: kswx.h:152) with I, a run of target-only
 * steps (op 2; the leftover columns, kswx.h:224-227, opened by row -1: kswx.h:143) with D - so the walk counts the two kinds apart and solves
 *     score - init = M*mat + X*mis + I*runs_ins + D*runs_del + E*(ins + del).
 * `sc` = {M, X, I, D, E, init_score (clamped)} (SP = false reads I for both); returns false when the identity does not come out in integers (never observed; the caller then leaves the job to the general kernel).
 * wtz_shift_traceback_pk (wtz_sw_frame16.h) is this function with the nibble trace's staging step. ---- */
struct wtz_tb_score { int32_t M, X, I, D, E, init; };
/* the identity above solved for mat: false = it does not come out in integers */
template<bool SP>
WTZ_D bool wtz_tb_solve(wtz_aln_t &x, const wtz_tb_score *sc, int32_t n_gap_runs, int32_t n_del_runs){
	/* n_gap_runs: all runs; n_del_runs: those of op 2 (counted with SP = true only) */
	const int32_t nd = x.mat, MXd = sc->M - sc->X;
	long long S = (long long)x.score - sc->init - (long long)n_gap_runs * sc->I - (long long)sc->E * (x.ins + x.del) - (long long)sc->X * nd;
	if constexpr(SP) S -= (long long)n_del_runs * ((long long)sc->D - sc->I);
	if(MXd == 0 || S % MXd != 0 || S / MXd < 0 || S / MXd > nd) return false;
	x.mat = (int32_t)(S / MXd); x.mis = nd - x.mat;
	return true;
}
template<int C, int NL, bool SP = false>
WTZ_D bool wtz_shift_traceback(wtz_aln_t &x, uint8_t **zchunk, const int32_t *zb, uint32_t zrow, uint64_t *tb, wtz_cigar_t &cigars, const wtz_tb_score *sc){
	const int lane = (int)(threadIdx.x & 63);
	constexpr int C4 = (C + 3) / 4;
	constexpr int NLW = (128 / C) < NL ? (128 / C) : NL;     /* lanes of a row inside the window */
	constexpr int NDW = NLW * C4, ROWB = NLW * C;
	static_assert(NDW <= 64 && ROWB <= 128, "window geometry");
	uint32_t *S32 = (uint32_t*)tb; uint8_t *S8 = (uint8_t*)tb; uint8_t *Sd = S8 + 8192;
	int32_t i_ = x.qe, j_ = x.te; uint32_t d_ = 0;
	uint32_t run_op = 0xFFu, run_len = 0;
	int32_t n_gap_runs = 0, n_del_runs = 0; bool consistent = true;
	wtz_cigw_t Wr; Wr.v = &cigars; Wr.tail = 0;
	int32_t cc = 0;
	if(i_ >= 0) cc = j_ - wtz_as_global(zb)[i_];
	const int ln_off = lane / C4, q4 = lane % C4;
	while(i_ >= 0 && j_ >= 0){
		const int32_t i0 = i_;
		int32_t L0 = (cc < 0 ? 0 : (cc > NL * C - 1 ? NL * C - 1 : cc)) / C - NLW / 2;
		if(L0 > NL - NLW) L0 = NL - NLW;
		if(L0 < 0) L0 = 0;
		const int32_t CC0 = L0 * C;
		{
			const int32_t r = i0 - lane;
			Sd[lane] = (r >= 1) ? (uint8_t)(wtz_as_global(zb)[r] - wtz_as_global(zb)[r - 1]) : (uint8_t)0;
		}
		const int32_t cA = i0 >> 6;
		const uint8_t *chA = wtz_as_global(zchunk)[cA];
		const uint8_t *chB = cA > 0 ? wtz_as_global(zchunk)[cA - 1] : chA;
		const bool act = lane < NDW && (L0 + ln_off) < NL;
		const uint32_t doff = act ? ((uint32_t)q4 * (uint32_t)NL + (uint32_t)(L0 + ln_off)) * 4u : 0u;
		const uint32_t pos0 = (uint32_t)ln_off * (uint32_t)C + (uint32_t)q4 * 4u;
		for(int r8 = 0; r8 < 64; r8 += 8){
			/* eight rows' loads are issued before the first is used; rows above row 0 re-read row 0 (never walked), idle lanes dword 0 (never stored) */
			uint32_t w8[8];
			#pragma unroll
			for(int u = 0; u < 8; u++){
				int32_t r = i0 - (r8 + u); if(r < 0) r = 0;
				const uint8_t *rowp = ((r >> 6) == cA ? chA : chB) + (size_t)(r & 63) * zrow;
				w8[u] = *wtz_as_global((const uint32_t*)(rowp + doff));
			}
			if(act){
				#pragma unroll
				for(int u = 0; u < 8; u++){
					/* the kernel's 4 decision bits -> the walker's byte: bits 1:0 move from H, bits 3:2 from E, bits 5:4 from F */
					const uint32_t w = w8[u];
					const uint32_t a = (w >> 2) & 0x01010101u, b = (w >> 3) & 0x01010101u;
					const uint32_t v = (a << 1) | (b & (a ^ 0x01010101u)) | ((w & 0x02020202u) << 1) | ((w & 0x01010101u) << 5);
					const uint32_t pos = (uint32_t)(r8 + u) * 128u + pos0;
					if constexpr((C & 3) == 0) S32[pos >> 2] = v;
					else {
						#pragma unroll
						for(int k = 0; k < 4; k++) if(q4 * 4 + k < C) S8[pos + k] = (uint8_t)(v >> (8 * k));
					}
				}
			}
		}
		__threadfence_block();
		if(lane == 0){
			while(i_ >= 0 && j_ >= 0){
				const int32_t rr = i0 - i_;
				if(rr >= 64) break;
				uint32_t zv = 0;
				if((uint32_t)cc < (uint32_t)(NL * C)){          /* outside the band the kernel stored nothing: a zero byte, as the byte-wise staging had it */
					const int32_t t = cc - CC0;
					if((uint32_t)t >= (uint32_t)ROWB) break;
					zv = S8[rr * 128 + t];
				}
				const int32_t sft = (int32_t)Sd[rr];
				d_ = (zv >> (d_ << 1)) & 0x03;
				if(d_ == 0){ x.mat++; i_--; j_--; cc += sft - 1; }      /* x.mat counts the diagonal steps until the end */
				else if(d_ == 1){ i_--; x.ins++; cc += sft; }
				else { j_--; x.del++; cc--; }
				if(d_ == run_op) run_len++;
				else { if(run_len) wtz_cigw_push(Wr, run_op, run_len); run_op = d_; run_len = 1; if(d_) n_gap_runs++; if constexpr(SP){ if(d_ == 2) n_del_runs++; } }
			}
		}
		i_ = __builtin_amdgcn_readfirstlane(i_); j_ = __builtin_amdgcn_readfirstlane(j_); cc = __builtin_amdgcn_readfirstlane(cc);
		__threadfence_block();
	}
	if(lane == 0){
		if(run_len) wtz_cigw_push(Wr, run_op, run_len);
		if(i_ >= 0){ x.ins += i_ + 1; wtz_cigw_push(Wr, 1, (uint32_t)(i_ + 1)); n_gap_runs++; }
		if(j_ >= 0){ x.del += j_ + 1; wtz_cigw_push(Wr, 2, (uint32_t)(j_ + 1)); n_gap_runs++; n_del_runs++; }
		wtz_cigw_finish(Wr);
		wtz_cigar_reverse(cigars.a, cigars.n);
		consistent = wtz_tb_solve<SP>(x, sc, n_gap_runs, n_del_runs);
		x.aln = x.mat + x.mis + x.ins + x.del; x.qe++; x.te++;
	}
	return __builtin_amdgcn_readfirstlane((int)consistent) != 0;
}

/* ---- K-sw3 jobs: one wave (64 threads) per job; jobs that do not fit the LDS rings run the scalar body on lane 0 ---- */
template<int P, int TW>
__global__ void __launch_bounds__(64) wtz_kernel_extjobs(wtz_extjob_t *jobs, const uint32_t *order, uint32_t n, const wtz_params_t *Pm, wtz_pool_t *pool, wtz_pool_t *tpool){
	__shared__ int32_t sHs[P]; __shared__ int32_t sEs[P]; __shared__ uint64_t stb[TW];
	const uint32_t b = blockIdx.x;
	if(b >= n) return;
	wtz_extjob_t *job = &jobs[order ? order[b] : b];
	if(!job->valid || job->done) return;
	const int lane = (int)(threadIdx.x & 63);
	int32_t init_score = job->init_score < 0 ? 0 : job->init_score;
	if(job->qlen <= 0 || job->tlen <= 0){
		if(lane == 0){ wtz_aln_t x; memset(&x, 0, sizeof x); x.score = init_score; job->x = x; job->cigar = NULL; job->cigar_len = 0; job->bad = 0; job->cells = 0; }
		return;
	}
	wtz_wave_lds_t L; L.Hs = sHs; L.Es = sEs; L.tb = stb; L.PM = P - 1; L.tw = TW;
	int32_t W = job->W, ql, tl, n_col;
	wtz_ext_geometry(job->qlen, job->tlen, init_score, W, Pm->M, Pm->I, Pm->D, Pm->E, Pm->T, ql, tl, n_col);
	if(wtz_wave_fits(L, n_col, tl, ql)){
		wtz_trace_t tr; tr.chunk = NULL; tr.zb = NULL; tr.n_chunk = 0; tr.zrow = 0; tr.cap_rows = 0;
		wtz_cigar_t cg; if(lane == 0) cg.init(pool, 64);
		unsigned long long cells = 0; bool ok = true;
		const int32_t Cw = (((n_col + 63) / 64) | 1);
		wtz_aln_t x;
		if(Cw <= 8)       x = wtz_extend_shift_wave_rt<8>(job->qlen, job->q, job->tlen, job->t, job->init_score, job->W, Pm->M, Pm->X, Pm->I, Pm->D, Pm->E, Pm->T, L, tr, tpool, cg, &cells, &ok);
		else if(Cw <= 16) x = wtz_extend_shift_wave_rt<16>(job->qlen, job->q, job->tlen, job->t, job->init_score, job->W, Pm->M, Pm->X, Pm->I, Pm->D, Pm->E, Pm->T, L, tr, tpool, cg, &cells, &ok);
		else              x = wtz_extend_shift_wave_rt<32>(job->qlen, job->q, job->tlen, job->t, job->init_score, job->W, Pm->M, Pm->X, Pm->I, Pm->D, Pm->E, Pm->T, L, tr, tpool, cg, &cells, &ok);
		if(lane == 0){ job->x = x; job->cigar = cg.a; job->cigar_len = cg.n; job->bad = (!ok || cg.bad); job->cells = cells; job->done = 3; }
	} else if(lane == 0){
		wtz_swmem_t mem; wtz_swmem_init(mem, tpool);
		wtz_cigar_t cg; cg.init(pool, 64);
		unsigned long long cells = 0;
		wtz_aln_t x = wtz_extend_shift(job->qlen, job->q, job->tlen, job->t, job->init_score, job->W, Pm->M, Pm->X, Pm->I, Pm->D, Pm->E, Pm->T, mem, cg, &cells);
		job->x = x; job->cigar = cg.a; job->cigar_len = cg.n; job->bad = (mem.bad || cg.bad); job->cells = cells; job->done = 3;
	}
}

#endif /* __HIPCC__ */
#endif
