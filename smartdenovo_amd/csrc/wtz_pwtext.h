/*
 * K-pwtext: the three-line picture of a pairwise alignment - kswx_cigar2pairwise (kswx.h:1150-1194) and the marker loop of pairaln.c:115-125 - from a CIGAR
 * (len << 4 | op; op 0 = both bases, 1 = query base over '-', 2 = '-' over target base) and two packed 2-bit views.  Output of one alignment of `cols` columns:
 * query line, marker line, target line, each cols bytes and a '\n' (the order of pairaln.c:126).  The same bodies run with ONE lane in the host emulation.
 *
 * Pass one (wtz_pwtext_scan, one wavefront per alignment): every lane takes 4 consecutive operations, sums them, and three wave scans (wtz_coop_excl_scan)
 * give each operation its first column, first query base and first target base; a fourth gives the operations of length > 0 (kswx.h:1157 skips the others)
 * their place in the TABLE, one 64-bit entry per kept operation: column | query base << 17 | target base << 34 | op << 51 (all three < 2^17: both sides <= 65 535).
 *
 * Pass two (wtz_pwtext_tile, one wavefront per TILE of WTZ_PWT_TILE = 512 columns of one alignment; the '\n' is column `cols` of every line): parallel over
 * columns, not over operations - 20 000 columns may be one operation or 15 000.
 *   1. the table entry of the tile's first column: a search with all lanes (NLANES + 1 intervals per step: three loads deep for 15 000 entries; a plain
 *      binary search with one lane);
 *   2. the tile's entries - at most one per column, since every entry has a column - go to LDS, 64 per step, until one starts behind the tile;
 *   3. every lane owns 8 consecutive columns: a binary search in LDS for its first column, ONE wtz_pack32 per side for its up to 8 bases (the view accessors:
 *      reverse-complement views and strand -1 as everywhere), a walk over its columns, 8 bytes per line into the LDS picture of the tile;
 *   4. the three lines go out: the bytes in front of the first 4-byte-aligned ADDRESS and behind the last one as byte stores, everything between as dword stores
 *      whose source is two LDS words and a funnel shift (line offsets are not aligned: cols + 1 per line, and nothing is padded).
 * LDS per wavefront: 4 KB of entries + 3 x 520 bytes of picture.
 */
#ifndef WTZ_PWTEXT_H
#define WTZ_PWTEXT_H

#include "wtz_sw.h"

#define WTZ_PWT_TILE 512            /* columns of a tile */
#define WTZ_PWT_CPL 8               /* consecutive columns of a lane */
#define WTZ_PWT_LINE_WORDS (WTZ_PWT_TILE / 4 + 2)      /* a line of the picture in LDS: the tile and the word the funnel shift reads behind it */
#define WTZ_PWT_MAXLEN 65535

/* q, t: the views from the alignment's start (qb, tb) on; qlen, tlen: what is left of them there.  cig_off / tab_off / text_off: the alignment's first CIGAR
 * word, table entry and byte inside the launch group's blocks */
typedef struct { wtz_seq_packed q, t; int32_t qlen, tlen; uint32_t n_ops, cols; unsigned long long cig_off, tab_off, text_off; } wtz_pwtprob_t;
typedef struct { uint32_t prob, tile; } wtz_pwttile_t;

#define WTZ_PWT_COL(e) ((uint32_t)(e) & 0x1FFFFu)
#define WTZ_PWT_QAT(e) ((uint32_t)((e) >> 17) & 0x1FFFFu)
#define WTZ_PWT_TAT(e) ((uint32_t)((e) >> 34) & 0x1FFFFu)
#define WTZ_PWT_OP(e)  ((uint32_t)((e) >> 51) & 3u)

/* pass one: the table of an alignment; returns its number of entries (every lane) */
WTZ_HD uint32_t wtz_pwtext_scan(const uint32_t *cig, uint32_t n_ops, unsigned long long *tab){
	const uint32_t lane = WTZ_LANE, NL = WTZ_NLANES;
	uint32_t c_col = 0, c_q = 0, c_t = 0, c_n = 0;      /* carried over the steps */
	for(uint32_t base = 0; base < n_ops; base += NL * 4u){
		const uint32_t i0 = base + lane * 4u;
		uint32_t w[4];
		#pragma unroll
		for(int k = 0; k < 4; k++) w[k] = i0 + (uint32_t)k < n_ops ? cig[i0 + k] : 0u;
		uint32_t s_col = 0, s_q = 0, s_t = 0, s_n = 0;
		#pragma unroll
		for(int k = 0; k < 4; k++){ const uint32_t len = w[k] >> 4, op = w[k] & 0xFu; s_col += len; s_q += op == 2u ? 0u : len; s_t += op == 1u ? 0u : len; s_n += len ? 1u : 0u; }
		uint32_t t_col, t_q, t_t, t_n;
		uint32_t col = c_col + wtz_coop_excl_scan(s_col, &t_col), qa = c_q + wtz_coop_excl_scan(s_q, &t_q), ta = c_t + wtz_coop_excl_scan(s_t, &t_t);
		uint32_t at = c_n + wtz_coop_excl_scan(s_n, &t_n);
		#pragma unroll
		for(int k = 0; k < 4; k++){
			const uint32_t len = w[k] >> 4, op = w[k] & 0xFu;
			if(len) tab[at++] = (unsigned long long)col | ((unsigned long long)qa << 17) | ((unsigned long long)ta << 34) | ((unsigned long long)op << 51);
			col += len; qa += op == 2u ? 0u : len; ta += op == 1u ? 0u : len;
		}
		c_col += t_col; c_q += t_q; c_t += t_t; c_n += t_n;
	}
	return c_n;
}

/* the last entry of tab[0, n) whose column is <= c (tab[0] starts at column 0, n >= 1): all lanes probe, the same result on every lane */
WTZ_HD uint32_t wtz_pwtext_find(const unsigned long long *tab, uint32_t n, uint32_t c){
	const uint32_t lane = WTZ_LANE, NL = WTZ_NLANES;
	uint32_t a = 0, b = n;
	while(b - a > 1u){
		const uint32_t step = (b - a + NL) / (NL + 1u);      /* >= 1 and < b - a */
		const uint32_t idx = a + (lane + 1u) * step;
		const bool le = idx < b && WTZ_PWT_COL(tab[idx]) <= c;
		const uint32_t cnt = (uint32_t)__builtin_popcountll(wtz_coop_ballot(le));      /* the columns ascend: the lanes that hold are the first cnt */
		a += cnt * step;
		b = a + step < b ? a + step : b;
	}
	return a;
}

WTZ_HD uint32_t wtz_pwtext_letters(uint32_t b){ return (0x54474341u >> (8u * b)) & 0xFFu; }      /* bit_base_table: A C G T */

/* pass two: tile `tile` of alignment p.  ent: WTZ_PWT_TILE entries, pic: 3 * WTZ_PWT_LINE_WORDS words (LDS on the device); text: the launch group's text block */
WTZ_HD void wtz_pwtext_tile(const wtz_pwtprob_t &p, uint32_t tile, const unsigned long long *tab, uint32_t n_ent, unsigned long long *ent, uint32_t *pic, char *text){
	const uint32_t lane = WTZ_LANE, NL = WTZ_NLANES;
	const uint32_t cols = wtz_coop_bcast32(p.cols), c0 = tile * WTZ_PWT_TILE;
	const uint32_t nc = cols + 1u - c0 < WTZ_PWT_TILE ? cols + 1u - c0 : WTZ_PWT_TILE;      /* with the '\n' */
	uint32_t n_stg = 0;
	if(c0 < cols && n_ent){
		const uint32_t lo = wtz_pwtext_find(tab, n_ent, c0), c_last = c0 + nc - 1u;
		for(uint32_t k = 0; ; k += NL){      /* at most TILE entries start inside the tile */
			const uint32_t idx = lo + k + lane;
			const unsigned long long e = idx < n_ent ? tab[idx] : ~0ull;
			const bool in = idx < n_ent && (k + lane == 0u || WTZ_PWT_COL(e) <= c_last) && k + lane < WTZ_PWT_TILE;
			if(in) ent[k + lane] = e;
			const uint32_t got = (uint32_t)__builtin_popcountll(wtz_coop_ballot(in));
			n_stg += got;
			if(got < NL || n_stg >= WTZ_PWT_TILE) break;
		}
	}
	WTZ_WAVE_SYNC();
	for(uint32_t g = lane; g < WTZ_PWT_TILE / WTZ_PWT_CPL; g += NL){
		const uint32_t cg = c0 + g * WTZ_PWT_CPL;
		uint32_t lq[2] = {0, 0}, lm[2] = {0, 0}, lt[2] = {0, 0};
		if(cg <= cols){
			uint32_t e = 0, e_end = cols, op = 0, qi = 0, ti = 0;
			unsigned long long qw = 0, tw = 0;
			if(cg < cols){
				uint32_t a = 0, b = n_stg;
				while(b - a > 1u){ const uint32_t m = (a + b) >> 1; if(WTZ_PWT_COL(ent[m]) <= cg){ a = m; } else { b = m; } }
				e = a;
				const unsigned long long en = ent[e];
				const uint32_t d = cg - WTZ_PWT_COL(en);
				op = WTZ_PWT_OP(en);
				const uint32_t q0 = WTZ_PWT_QAT(en) + (op == 2u ? 0u : d), t0 = WTZ_PWT_TAT(en) + (op == 1u ? 0u : d);
				e_end = e + 1u < n_stg ? WTZ_PWT_COL(ent[e + 1u]) : cols;
				qw = wtz_pack32(p.q, (int32_t)q0, p.qlen); tw = wtz_pack32(p.t, (int32_t)t0, p.tlen);
			}
			#pragma unroll
			for(uint32_t j = 0; j < WTZ_PWT_CPL; j++){
				const uint32_t c = cg + j;
				uint32_t a, m, b;
				if(c < cols){
					if(c >= e_end){ e++; op = WTZ_PWT_OP(ent[e]); e_end = e + 1u < n_stg ? WTZ_PWT_COL(ent[e + 1u]) : cols; }
					a = '-'; b = '-';
					if(op != 2u){ a = wtz_pwtext_letters((uint32_t)(qw >> (2u * qi)) & 3u); qi++; }
					if(op != 1u){ b = wtz_pwtext_letters((uint32_t)(tw >> (2u * ti)) & 3u); ti++; }
					m = a == '-' ? '-' : (a == b ? '|' : (b == '-' ? '-' : '*'));      /* pairaln.c:116-124 */
				} else if(c == cols){ a = m = b = '\n'; }
				else { a = m = b = 0; }
				lq[j >> 2] |= a << (8u * (j & 3u)); lm[j >> 2] |= m << (8u * (j & 3u)); lt[j >> 2] |= b << (8u * (j & 3u));
			}
		}
		pic[0 * WTZ_PWT_LINE_WORDS + 2u * g] = lq[0]; pic[0 * WTZ_PWT_LINE_WORDS + 2u * g + 1u] = lq[1];
		pic[1 * WTZ_PWT_LINE_WORDS + 2u * g] = lm[0]; pic[1 * WTZ_PWT_LINE_WORDS + 2u * g + 1u] = lm[1];
		pic[2 * WTZ_PWT_LINE_WORDS + 2u * g] = lt[0]; pic[2 * WTZ_PWT_LINE_WORDS + 2u * g + 1u] = lt[1];
	}
	if(lane == 0){ for(uint32_t l = 0; l < 3; l++){ pic[l * WTZ_PWT_LINE_WORDS + WTZ_PWT_TILE / 4] = 0; pic[l * WTZ_PWT_LINE_WORDS + WTZ_PWT_TILE / 4 + 1] = 0; } }
	WTZ_WAVE_SYNC();
	/* the lines go out: bytes [G, G + nc) of the text block from bytes [0, nc) of the line's picture */
#if defined(__HIP_DEVICE_COMPILE__)
	WTZ_GLOBAL_AS char *out = wtz_as_global(text);
#else
	char *out = text;
#endif
	for(uint32_t l = 0; l < 3; l++){
		const uint32_t *src = pic + l * WTZ_PWT_LINE_WORDS;
		const unsigned long long G = wtz_coop_bcast64(p.text_off) + (unsigned long long)l * (cols + 1u) + c0;
		const uintptr_t addr = (uintptr_t)text + (uintptr_t)G;
		uint32_t head = (uint32_t)((4u - (uint32_t)(addr & 3u)) & 3u);
		if(head > nc) head = nc;
		const uint32_t nd = (nc - head) >> 2, tail0 = head + 4u * nd;
		for(uint32_t k = lane; k < head; k += NL) out[G + k] = (char)(src[0] >> (8u * k));
		for(uint32_t d = lane; d < nd; d += NL){
			const uint32_t s = head + 4u * d, sh = 8u * (s & 3u);
			const uint32_t w0 = src[s >> 2], w1 = src[(s >> 2) + 1u];
			const uint32_t v = sh ? (w0 >> sh) | (w1 << (32u - sh)) : w0;
#if defined(__HIP_DEVICE_COMPILE__)
			*(WTZ_GLOBAL_AS uint32_t*)(out + G + s) = v;
#else
			memcpy(out + G + s, &v, 4);
#endif
		}
		for(uint32_t k = tail0 + lane; k < nc; k += NL) out[G + k] = (char)(src[k >> 2] >> (8u * (k & 3u)));
	}
	WTZ_WAVE_SYNC();
}

#if defined(__HIPCC__) && !defined(WTZ_EMUL)
/* block b = one wavefront = alignment b */
__global__ void __launch_bounds__(64) wtz_kernel_pwscan(const wtz_pwtprob_t *pr, uint32_t n, const uint32_t *cig, unsigned long long *tab, uint32_t *n_ent){
	if(blockIdx.x >= n) return;
	const wtz_pwtprob_t p = pr[blockIdx.x];
	const uint32_t k = wtz_pwtext_scan(cig + p.cig_off, wtz_coop_bcast32(p.n_ops), tab + p.tab_off);
	if(WTZ_LANE == 0) n_ent[blockIdx.x] = k;
}
/* block b = one wavefront = tile tiles[b] */
__global__ void __launch_bounds__(64) wtz_kernel_pwtext(const wtz_pwtprob_t *pr, const wtz_pwttile_t *tiles, uint32_t n_tiles, const unsigned long long *tab, const uint32_t *n_ent, char *text){
	__shared__ unsigned long long ent[WTZ_PWT_TILE];
	__shared__ uint32_t pic[3 * WTZ_PWT_LINE_WORDS];
	if(blockIdx.x >= n_tiles) return;
	const wtz_pwttile_t t = tiles[blockIdx.x];
	const wtz_pwtprob_t p = pr[t.prob];
	wtz_pwtext_tile(p, t.tile, tab + p.tab_off, wtz_coop_bcast32(n_ent[t.prob]), ent, pic, text);
}
#endif
#endif
