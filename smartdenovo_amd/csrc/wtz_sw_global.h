/*
 * wtz_sw_global.h — K-sw2, ksw_global2 (ksw.c:503-586), one 64-lane wavefront per problem; rows run over the target, lanes over the query band:
 *     wtz_global_wave            the ring form (any band the rings hold): the row of wtz_sw_shift.h with MINUS_INF sentinels;
 *     wtz_gwalk_step             the branch-free traceback step of lane 0 (ksw.c:560-586);
 *     wtz_global_reg<C, ZG>      the register form: C band columns per lane, 4-bit trace in LDS or (ZG) in the pool.
 * wtz_gap_problem_wave (wtz_tasks.h) picks the form of a gap.
 */
#ifndef WTZ_SW_GLOBAL_H
#define WTZ_SW_GLOBAL_H

#include "wtz_wave.h"

#ifdef __HIPCC__

/* ---- K-sw2, ksw_global2 (ksw.c:503-586), one wavefront per problem: rows run over the target, lanes over the query band.
 *      Same cell recurrence as the extensions with MINUS_INF sentinels, the lh3 first-row / first-column initialisation,
 *      no early exit; the score is H(tlen-1, qlen-1) and the traceback starts from that cell.  CIGAR on lane 0. ---- */
template<typename SQ, typename ST>
WTZ_D int32_t wtz_global_wave(int32_t qlen, const SQ &query, int32_t tlen, const ST &target, int32_t M, int32_t X,
		int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, int32_t w, const wtz_wave_lds_t &L, wtz_trace_t &tr, wtz_pool_t *pool,
		wtz_cigar_t &cig, bool *ok){
	const int lane = (int)(threadIdx.x & 63);
	const int32_t PM = L.PM, oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
	*ok = true;
	if(lane == 0) cig.n = 0;
	const int32_t n_col = qlen < 2 * w + 1 ? qlen : 2 * w + 1;
	const int32_t C0 = (n_col + 63) / 64, C = (C0 | 1), C4 = (C + 3) / 4;
	const uint32_t zrow = (uint32_t)C4 * 256u;
	if(!wtz_trace_prepare(tr, pool, zrow, tlen, false)){ *ok = false; return 0; }
	uint8_t **zchunk = tr.chunk; uint8_t *z = NULL;
	{   /* stage the query [0, qlen) as 2-bit codes */
		const int32_t nw = (qlen + 31) / 32 + 1;
		for(int32_t ww = lane; ww < nw; ww += 64){
			uint64_t v = 0; const int32_t b0 = ww * 32;
			for(int32_t k = 0; k < 32 && b0 + k < qlen; k++) v |= ((uint64_t)query.at(b0 + k)) << (2 * k);
			L.tb[ww] = v;
		}
	}
	int32_t begp = 0, endp = 0, i, h_lastrow = 0, end_last = 0;
	const int32_t CE = C * (-e_ins);
	for(i = 0; i < tlen; i++){
		if((i & 63) == 0){
			const uint32_t ci = (uint32_t)i >> 6;
			unsigned long long za = 0;
			if(ci < tr.n_chunk){ z = zchunk[ci]; }
			else {
				if(lane == 0){ uint8_t *p = (uint8_t*)wtz_pool_alloc(pool, (size_t)zrow * 64); zchunk[ci] = p; za = (unsigned long long)(uintptr_t)p; }
				za = __shfl(za, 0, 64);
				z = (uint8_t*)(uintptr_t)za;
				if(z == NULL){ *ok = false; return 0; }
				tr.n_chunk = ci + 1;
			}
		}
		const int32_t beg = i > w ? i - w : 0;
		const int32_t end = i + w + 1 < qlen ? i + w + 1 : qlen;
		const uint32_t tbase = target.at(i);
		const int32_t j0 = beg + lane * C;
		uint64_t qbits = 0;
		int32_t agg = -0x7F000000;
		{
			int32_t saved = 0;
			for(int32_t k = 0; k < C; k++){
				const int32_t j = j0 + k;
				if((k & 31) == 0){        /* the lane's next 32 query bases (bands wider than 64 x 32 columns have more than 32 columns per lane) */
					const int32_t jq = j0 + k;
					const int32_t jj = jq < qlen ? jq : (qlen > 0 ? qlen - 1 : 0);
					const int32_t ww = jj >> 5, sh = (jj & 31) * 2;
					const uint64_t w0 = L.tb[ww], w1 = L.tb[ww + 1];
					qbits = sh ? ((w0 >> sh) | (w1 << (64 - sh))) : w0;
				}
				if(j < end){
					int32_t pred;
					if(i == 0){ pred = (j == 0) ? 0 : ((j <= w) ? -(o_ins + e_ins * j) : WTZ_MINUS_INF); }       /* eh[] initialisation, ksw.c:519-523 */
					else if(k == 0){
						if(j - 1 >= begp && j - 1 < endp) pred = L.Hs[(j - 1) & PM];
						else pred = (j == 0) ? -(o_del + e_del * i) : WTZ_MINUS_INF;
					} else pred = saved;
					saved = (i > 0 && j >= begp && j < endp) ? L.Hs[j & PM] : WTZ_MINUS_INF;
					const uint32_t qb = (uint32_t)(qbits >> (2 * (k & 31))) & 3u;
					const int32_t m = pred + ((tbase == qb) ? M : X);
					L.Hs[j & PM] = m;
					const int32_t cand = m - oe_ins + (C - 1 - k) * (-e_ins);
					agg = agg > cand ? agg : cand;
				}
			}
		}
		const int32_t f_in = wtz_f_carry(agg, lane, CE, -0x7F000000, WTZ_MINUS_INF);
		int32_t h_last = 0;
		{
			int32_t f = f_in; uint32_t zword = 0;
			uint32_t *zr = (uint32_t*)(z + (size_t)(i & 63) * zrow) + lane;
			for(int32_t k = 0; k < C; k++){
				const int32_t j = j0 + k;
				if(j < end){
					const int32_t m = L.Hs[j & PM];
					int32_t e = (j >= begp && j < endp) ? L.Es[j & PM] : WTZ_MINUS_INF;
					uint32_t d; int32_t h;
					if(m >= e){ d = 0; h = m; } else { d = 1; h = e; }
					if(h < f){ d = 2; h = f; }
					h_last = h;
					int32_t t = m - oe_del; e -= e_del; if(e > t) d |= 1u << 2; else e = t;
					t = m - oe_ins; f -= e_ins; if(f > t) d |= 2u << 4; else f = t;
					L.Hs[j & PM] = h; L.Es[j & PM] = e;
					zword |= d << (8 * (k & 3));
				}
				if((k & 3) == 3 || k == C - 1){ zr[(size_t)(k >> 2) * 64] = zword; zword = 0; }
			}
		}
		if(end > beg){ const int32_t lastlane = (end - 1 - beg) / C; h_lastrow = __builtin_amdgcn_readlane(h_last, __builtin_amdgcn_readfirstlane(lastlane)); }
		begp = beg; endp = end; end_last = end;
	}
	const int32_t score = (end_last == qlen) ? h_lastrow : ((qlen <= w) ? -(o_ins + e_ins * qlen) : WTZ_MINUS_INF);
	__threadfence_block();     /* the trace was written by lanes of THIS wave: ordering inside the wave is enough (an agent-scope fence would write back the whole L2) */
	if(lane == 0){
		uint32_t which = 0;
		int32_t ii = tlen - 1, k = (ii + w + 1 < qlen ? ii + w + 1 : qlen) - 1;
		while(ii >= 0 && k >= 0){
			const int32_t col = k - (ii > w ? ii - w : 0);
			const int32_t ln = col / C, kk = col - ln * C;
			const uint8_t zv = zchunk[ii >> 6][(size_t)(ii & 63) * zrow + (size_t)(kk >> 2) * 256 + (size_t)ln * 4 + (kk & 3)];
			which = (zv >> (which << 1)) & 3;
			if(which == 0){ wtz_cigar_push(cig, 0, 1); --ii; --k; }
			else if(which == 1){ wtz_cigar_push(cig, 2, 1); --ii; }
			else { wtz_cigar_push(cig, 1, 1); --k; }
		}
		if(ii >= 0) wtz_cigar_push(cig, 2, (uint32_t)(ii + 1));
		if(k >= 0) wtz_cigar_push(cig, 1, (uint32_t)(k + 1));
		wtz_cigar_reverse(cig.a, cig.n);
	}
	return score;
}

/* one step of the ksw_global2 traceback on lane 0, without branches (see wtz_walk_step): rows run over the target (its base comes from
 * the 32-base words held in VGPRs), columns over the query (2-bit words in LDS); `which` 0 / 1 / 2 = from H / E (deletion, row up) /
 * F (insertion, column left) */
typedef struct { int32_t ii, k; uint32_t which, run_op, run_len, nr; int32_t mat, mis; } wtz_gwalk_t;
WTZ_D void wtz_gwalk_step(wtz_gwalk_t &g, uint32_t nib, const uint32_t *qb32, uint32_t tw_lo, uint32_t tw_hi, uint32_t *runs){
	const uint32_t h3 = nib & 3u, h = h3 > 2u ? 2u : h3;
	const uint32_t wh = ((h | (nib & 4u) | ((nib & 8u) << 2)) >> (g.which << 1)) & 3u;
	const uint32_t op = (0x18u >> (wh << 1)) & 3u;                 /* 0 -> M, 1 -> D (2), 2 -> I (1) */
	const uint32_t qv = (qb32[g.k >> 4] >> ((g.k & 15) * 2)) & 3u;
	const int ts = __builtin_amdgcn_readfirstlane((g.ii & 2047) >> 5);
	const uint32_t tlo = (uint32_t)__builtin_amdgcn_readlane((int)tw_lo, ts), thi = (uint32_t)__builtin_amdgcn_readlane((int)tw_hi, ts);
	const uint32_t tv = (((g.ii & 16) ? thi : tlo) >> ((g.ii & 15) * 2)) & 3u;
	const uint32_t is0 = wh == 0 ? 1u : 0u, is1 = wh == 1 ? 1u : 0u, is2 = wh == 2 ? 1u : 0u, eq = qv == tv ? 1u : 0u;
	g.mat += (int32_t)(is0 & eq); g.mis += (int32_t)(is0 & (eq ^ 1u));
	g.ii -= (int32_t)(is0 | is1); g.k -= (int32_t)(is0 | is2);
	const bool same = op == g.run_op;
	g.nr += (!same && g.run_len) ? 1u : 0u;
	g.run_len = same ? g.run_len + 1u : 1u; g.run_op = op; g.which = wh;
	runs[g.nr] = (g.run_len << 4) | op;
}

/*
 * K-sw2 (ksw_global2) for gaps whose band fits two columns per lane: the register form of wtz_global_wave.  Rows run over
 * the target (its row base is scalar, from 32-base words held in VGPRs), lanes over the query band (2-bit words in LDS);
 * the fixed band moves right by one column per row once i > w, so the hand-over is the same DPP move as in K-sw1; the
 * trace is 4 bits per cell in LDS.  Besides the CIGAR runs (traceback order, in `runs`) it returns the match / mismatch
 * counts of the M runs, which the caller would otherwise have to recount base by base (hzm_aln.h:1424-1436).
 * Requirements (caller): n_col <= 64*C, (qlen+63)/32+1 <= qb words; LDS trace (ZG false): ((tlen+1)/2)*zrow + 4*(qlen+tlen+4) <= LDS
 * trace bytes and tlen <= 2048; pool trace (ZG true): any tlen, `stage` = 4 KB of LDS.
 */
template<int C, bool ZG = false>
WTZ_D int32_t wtz_global_reg(int32_t qlen, const wtz_seq_packed &query, int32_t tlen, const wtz_seq_packed &target, int32_t M, int32_t X,
		int32_t o_del, int32_t e_del, int32_t o_ins, int32_t e_ins, int32_t w, uint64_t *qb, uint8_t *ztr, uint32_t zrow,
		uint32_t *runs, uint32_t *n_runs, int32_t *n_mat, int32_t *n_mis, uint8_t *stage = NULL){
	/* ZG: the trace does not fit LDS and lives in the pool (HBM); the rows store it through a global-address-space pointer and
	 * the traceback walks LDS-staged blocks of 32 packed rows (64 DP rows) x the whole band (<= 4 KB in `stage`) */
	const int lane = (int)(threadIdx.x & 63);
	const int32_t oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
	*n_runs = 0; *n_mat = 0; *n_mis = 0;
	{
		const int32_t nw = (qlen + 31) / 32 + 1;
		for(int32_t ww = lane; ww < nw; ww += 64) qb[ww] = wtz_pack32(query, ww * 32, qlen);
	}
	__threadfence_block();
	const uint32_t *qb32 = (const uint32_t*)qb;
	int32_t hp[C], ep[C]; uint32_t nibp[C];
	#pragma unroll
	for(int k = 0; k < C; k++){ hp[k] = WTZ_MINUS_INF; ep[k] = WTZ_MINUS_INF; nibp[k] = 0; }
	const int32_t CE = C * (-e_ins);
	const int32_t colrel0 = lane * C;
	uint32_t tw_lo = 0, tw_hi = 0, tcur = 0, qwin = 0; int32_t qwin_left = 0;
	int32_t begp = 0, i, h_lastrow = 0, end_last = 0;
	for(i = 0; i < tlen; i++){
		const int32_t beg = i > w ? i - w : 0;
		const int32_t end = i + w + 1 < qlen ? i + w + 1 : qlen;
		if((i & 2047) == 0){ const uint64_t v = wtz_pack32(target, i + lane * 32, tlen); tw_lo = (uint32_t)v; tw_hi = (uint32_t)(v >> 32); }
		if((i & 15) == 0){
			const int32_t ts = __builtin_amdgcn_readfirstlane((i & 2047) >> 5);
			tcur = (i & 16) ? (uint32_t)__builtin_amdgcn_readlane((int)tw_hi, ts) : (uint32_t)__builtin_amdgcn_readlane((int)tw_lo, ts);
		}
		const uint32_t tbase = (tcur >> ((i & 15) * 2)) & 3u;
		const int32_t j0 = beg + colrel0;
		const bool moved = (i > 0) && (beg != begp);
		if(moved){ qwin >>= 2; qwin_left--; }
		if(i == 0 || qwin_left < C){
			const int32_t jj = j0 < qlen ? j0 : (qlen > 0 ? qlen - 1 : 0);
			const uint32_t lo = qb32[jj >> 4], hi = qb32[(jj >> 4) + 1];
			qwin = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(jj & 15) * 2u);
			qwin_left = 16;
		}
		int32_t pred[C], ein[C];
		if(i == 0){
			#pragma unroll
			for(int k = 0; k < C; k++){ const int32_t j = j0 + k; pred[k] = (j == 0) ? 0 : ((j <= w) ? -(o_ins + e_ins * j) : WTZ_MINUS_INF); ein[k] = WTZ_MINUS_INF; }      /* eh[] initialisation, ksw.c:519-523 */
		} else if(moved){
			const int32_t nxt = wtz_dpp_wave_shl1(WTZ_MINUS_INF, ep[0]);
			#pragma unroll
			for(int k = 0; k < C; k++){ pred[k] = hp[k]; ein[k] = (k + 1 < C) ? ep[k + 1] : nxt; }
		} else {
			int32_t prv = wtz_dpp_wave_shr1(WTZ_MINUS_INF, hp[C - 1]);
			prv = (lane == 0) ? -(o_del + e_del * i) : prv;             /* first column, ksw.c:533 */
			#pragma unroll
			for(int k = 0; k < C; k++){ pred[k] = k ? hp[k - 1] : prv; ein[k] = ep[k]; }
		}
		int32_t mv[C]; bool valid[C]; int32_t agg = -0x7F000000;
		#pragma unroll
		for(int k = 0; k < C; k++){
			const uint32_t qbase = (qwin >> (2 * k)) & 3u;
			mv[k] = pred[k] + ((tbase == qbase) ? M : X);
			valid[k] = (j0 + k < end);
			const int32_t cand = mv[k] - oe_ins + (C - 1 - k) * (-e_ins);
			agg = (valid[k] && cand > agg) ? cand : agg;
		}
		int32_t f = wtz_f_carry(agg, lane, CE, -0x7F000000, WTZ_MINUS_INF);
		#pragma unroll
		for(int k = 0; k < C; k++){
			const int32_t m = mv[k], e = ein[k];
			const int32_t h0 = m > e ? m : e;
			const int32_t te = m - oe_del, e2 = e - e_del, tf = m - oe_ins, f2 = f - e_ins;
			/* decisions as sign bits of differences (all values within +-2^30 + a few thousand: no overflow), see wtz_extend_fixed_reg */
			uint32_t nib = (uint32_t)(tf - f2) >> 31;
			nib = __builtin_amdgcn_alignbit(nib, (uint32_t)(te - e2), 31);
			nib = __builtin_amdgcn_alignbit(nib, (uint32_t)(h0 - f), 31);
			nib = __builtin_amdgcn_alignbit(nib, (uint32_t)(m - e), 31);
			const int32_t h = h0 > f ? h0 : f;
			const int32_t en = e2 > te ? e2 : te;
			f = f2 > tf ? f2 : tf;
			hp[k] = valid[k] ? h : WTZ_MINUS_INF; ep[k] = valid[k] ? en : WTZ_MINUS_INF;
			nib = valid[k] ? nib : 0u;
			if(i & 1){
				if((uint32_t)(colrel0 + k) < zrow){
					if(ZG) wtz_as_global(ztr)[(size_t)(i >> 1) * zrow + colrel0 + k] = (uint8_t)(nibp[k] | (nib << 4));
					else ztr[(size_t)(i >> 1) * zrow + colrel0 + k] = (uint8_t)(nibp[k] | (nib << 4));
				}
			}
			else nibp[k] = nib;
		}
		if(end > beg && i + 1 == tlen){
			const int32_t idx = end - 1 - beg;
			int32_t hsel = hp[0];
			#pragma unroll
			for(int k = 1; k < C; k++) hsel = (idx % C == k) ? hp[k] : hsel;
			h_lastrow = __builtin_amdgcn_readlane(hsel, __builtin_amdgcn_readfirstlane(idx / C));
		}
		begp = beg; end_last = end;
	}
	if(tlen > 0 && !((tlen - 1) & 1)){
		#pragma unroll
		for(int k = 0; k < C; k++) if((uint32_t)(colrel0 + k) < zrow) ztr[(size_t)((tlen - 1) >> 1) * zrow + colrel0 + k] = (uint8_t)nibp[k];
	}
	const int32_t score = (end_last == qlen) ? h_lastrow : ((qlen <= w) ? -(o_ins + e_ins * qlen) : WTZ_MINUS_INF);
	__threadfence_block();
	if(ZG){
		wtz_gwalk_t g; g.which = 0; g.nr = 0; g.run_op = 0xFFu; g.run_len = 0; g.mat = g.mis = 0;
		g.ii = tlen - 1; g.k = (g.ii + w + 1 < qlen ? g.ii + w + 1 : qlen) - 1;
		int32_t ii = g.ii, k = g.k;
		uint32_t *stage32 = (uint32_t*)stage;
		const int32_t RB = zrow <= 128 ? 32 : (zrow <= 256 ? 16 : 8);         /* packed rows per staged block: RB * zrow <= 4 KB */
		int32_t cur_tblk = (tlen - 1) >> 11;                                    /* the 2048-row block of target words the DP loop left in tw_lo / tw_hi */
		while(ii >= 0 && k >= 0){
			const int32_t p1 = ii >> 1, p0 = p1 >= RB - 1 ? p1 - (RB - 1) : 0;
			if((ii >> 11) != cur_tblk){
				cur_tblk = ii >> 11;
				const uint64_t v = wtz_pack32(target, (cur_tblk << 11) + lane * 32, tlen); tw_lo = (uint32_t)v; tw_hi = (uint32_t)(v >> 32);
			}
			{
				const uint32_t nd = (uint32_t)(p1 - p0 + 1) * (zrow >> 2);
				const uint32_t *src = (const uint32_t*)(ztr + (size_t)p0 * zrow);
				for(uint32_t xw = (uint32_t)lane; xw < nd; xw += 64) stage32[xw] = src[xw];
			}
			__threadfence_block();
			if(lane == 0){
				while((g.ii | g.k) >= 0 && (g.ii >> 1) >= p0 && (g.ii >> 11) == cur_tblk){
					const int32_t col = g.k - (g.ii > w ? g.ii - w : 0);
					const uint32_t zv = stage[(size_t)((g.ii >> 1) - p0) * zrow + col];
					wtz_gwalk_step(g, zv >> ((g.ii & 1) * 4), (const uint32_t*)qb, tw_lo, tw_hi, runs);
				}
			}
			ii = __builtin_amdgcn_readfirstlane(g.ii); k = __builtin_amdgcn_readfirstlane(g.k);
			__threadfence_block();
		}
		if(lane == 0){
			uint32_t run_op = g.run_op, run_len = g.run_len, nr = g.nr;
			if(ii >= 0){ if(run_len && run_op == 2u) run_len += (uint32_t)(ii + 1); else { if(run_len) runs[nr++] = (run_len << 4) | run_op; run_op = 2u; run_len = (uint32_t)(ii + 1); } }
			if(k >= 0){ if(run_len && run_op == 1u) run_len += (uint32_t)(k + 1); else { if(run_len) runs[nr++] = (run_len << 4) | run_op; run_op = 1u; run_len = (uint32_t)(k + 1); } }
			if(run_len) runs[nr++] = (run_len << 4) | run_op;
			*n_runs = nr; *n_mat = g.mat; *n_mis = g.mis;
		}
		return score;
	}
	if(lane == 0){
		wtz_gwalk_t g; g.which = 0; g.nr = 0; g.run_op = 0xFFu; g.run_len = 0; g.mat = g.mis = 0;
		g.ii = tlen - 1; g.k = (g.ii + w + 1 < qlen ? g.ii + w + 1 : qlen) - 1;
		while((g.ii | g.k) >= 0){
			const int32_t col = g.k - (g.ii > w ? g.ii - w : 0);
			const uint32_t zv = ztr[(size_t)(g.ii >> 1) * zrow + col];
			wtz_gwalk_step(g, zv >> ((g.ii & 1) * 4), (const uint32_t*)qb, tw_lo, tw_hi, runs);
		}
		const int32_t ii = g.ii, k = g.k; const int32_t mat = g.mat, mis = g.mis;
		uint32_t run_op = g.run_op, run_len = g.run_len, nr = g.nr;
		if(ii >= 0){ if(run_len && run_op == 2u) run_len += (uint32_t)(ii + 1); else { if(run_len) runs[nr++] = (run_len << 4) | run_op; run_op = 2u; run_len = (uint32_t)(ii + 1); } }
		if(k >= 0){ if(run_len && run_op == 1u) run_len += (uint32_t)(k + 1); else { if(run_len) runs[nr++] = (run_len << 4) | run_op; run_op = 1u; run_len = (uint32_t)(k + 1); } }
		if(run_len) runs[nr++] = (run_len << 4) | run_op;
		*n_runs = nr; *n_mat = mat; *n_mis = mis;
	}
	return score;
}

#endif /* __HIPCC__ */
#endif
