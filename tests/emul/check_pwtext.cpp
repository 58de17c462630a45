/*
 * check_pwtext — the bodies of smartdenovo_amd/csrc/wtz_pwtext.h (wtz_pwtext_scan, wtz_pwtext_find, wtz_pwtext_tile) in the host emulation over random CIGARs and
 * views, against a scalar restatement of kswx_cigar2pairwise (kswx.h:1150-1194) and the marker loop of pairaln.c:115-125 written here.  Every buffer has exactly
 * the planned size (the table: one entry per operation; the picture: 3 * (cols + 1) bytes at an arbitrary offset of a heap block with nothing behind it), so that
 * a sanitizer build sees every byte the bodies touch:
 *     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DWTZ_EMUL -Iinclude -Ismartdenovo_amd/csrc -o check_pwtext tests/emul/check_pwtext.cpp && ./check_pwtext
 * Prints "<n> alignments, <k> bad"; exit status 1 when k > 0.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "wtz_common.h"
#include "wtz_pwtext.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n){ rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)((rng_state >> 11) % n); }

/* the reads of the test: 2-bit packed as dna.h:78 does, exactly the words the bases need */
static std::vector<uint8_t> g_base;
static std::vector<uint64_t> g_bits;

static uint32_t base_of(int64_t start, int32_t strand, uint32_t comp, int32_t i){ const uint32_t b = g_base[(size_t)(start + (int64_t)i * strand)]; return comp ? 3u - b : b; }

static std::string restate(const wtz_pwtprob_t &p, const std::vector<uint32_t> &cig){
	std::string a, b, m;
	int32_t x = 0, y = 0;
	for(uint32_t w : cig){
		const uint32_t op = w & 0xFu; const int32_t len = (int32_t)(w >> 4);
		if(len == 0) continue;
		for(int32_t j = 0; j < len; j++){
			a += op == 2 ? '-' : "ACGT"[base_of(p.q.start, p.q.strand, p.q.comp, x + j)];
			b += op == 1 ? '-' : "ACGT"[base_of(p.t.start, p.t.strand, p.t.comp, y + j)];
		}
		if(op != 2) x += len;
		if(op != 1) y += len;
	}
	for(size_t i = 0; i < a.size(); i++) m += a[i] == '-' ? '-' : (a[i] == b[i] ? '|' : (b[i] == '-' ? '-' : '*'));
	return a + "\n" + m + "\n" + b + "\n";
}

int main(){
	const size_t NB = 70000;
	g_base.resize(NB); g_bits.assign((NB + 31) / 32, 0);
	for(size_t i = 0; i < NB; i++){ g_base[i] = (uint8_t)rnd(4); g_bits[i >> 5] |= (uint64_t)g_base[i] << (((~i) & 31u) << 1); }
	unsigned n_aln = 0, bad = 0;
	for(unsigned it = 0; it < 1500; it++){
		/* the shape: mostly small, some around the tile and wave sizes, a few long; runs of length 1, zero-length operations, long runs */
		const uint32_t kind = rnd(10);
		uint32_t want = kind < 5 ? rnd(70) : (kind < 8 ? 480 + rnd(80) + 512 * rnd(3) : (kind == 8 ? 1 + rnd(3000) : 18000 + rnd(4000)));
		const uint32_t style = rnd(4);      /* 0: unit runs, 1: short runs, 2: long runs, 3: mixed with zero-length operations */
		std::vector<uint32_t> cig; uint32_t cols = 0, nq = 0, nt = 0;
		while(cols < want){
			uint32_t len = style == 0 ? 1 : (style == 1 ? 1 + rnd(6) : (style == 2 ? 1 + rnd(900) : (rnd(4) == 0 ? 0 : 1 + rnd(40))));
			if(len > want - cols) len = want - cols;
			const uint32_t op = rnd(3);
			cig.push_back(len << 4 | op); cols += len; if(op != 2) nq += len; if(op != 1) nt += len;
		}
		if(style == 3 && rnd(2)) cig.push_back(rnd(3));      /* a zero-length operation at the end */
		if(nq > 30000 || nt > 30000) continue;
		wtz_pwtprob_t p; memset(&p, 0, sizeof p);
		/* the views: forward or backward, complemented or not, anywhere in the bases (the first and the last base included) */
		for(int side = 0; side < 2; side++){
			wtz_seq_packed &s = side ? p.t : p.q; const uint32_t len = side ? nt : nq;
			s.bits = g_bits.data(); s.strand = rnd(2) ? 1 : -1; s.comp = rnd(2);
			const uint32_t room = (uint32_t)NB - len, at = rnd(8) == 0 ? 0 : (rnd(8) == 0 ? room : rnd(room + 1));      /* the lowest base the view touches */
			s.start = s.strand > 0 ? (int64_t)at : (int64_t)at + (len ? len - 1 : 0);
		}
		p.qlen = (int32_t)nq; p.tlen = (int32_t)nt; p.n_ops = (uint32_t)cig.size(); p.cols = cols;
		const std::string want_text = restate(p, cig);
		/* buffers of exactly the planned size */
		uint32_t *d_cig = (uint32_t*)malloc(cig.size() * 4 + 1); for(size_t k = 0; k < cig.size(); k++) d_cig[k] = cig[k];
		unsigned long long *tab = (unsigned long long*)malloc(cig.size() * 8 + 1);
		const uint32_t lead = rnd(8);
		p.text_off = lead;
		char *text = (char*)malloc(lead + 3 * ((size_t)cols + 1));
		memset(text, '#', lead + 3 * ((size_t)cols + 1));
		const uint32_t n_ent = wtz_pwtext_scan(d_cig, p.n_ops, tab);
		std::vector<unsigned long long> ent(WTZ_PWT_TILE); std::vector<uint32_t> pic(3 * WTZ_PWT_LINE_WORDS);
		for(uint32_t t = 0; t <= cols / WTZ_PWT_TILE; t++) wtz_pwtext_tile(p, t, tab, n_ent, ent.data(), pic.data(), text);
		bool ok = want_text.size() == 3 * ((size_t)cols + 1) && memcmp(text + lead, want_text.data(), want_text.size()) == 0;
		for(uint32_t k = 0; k < lead; k++) ok = ok && text[k] == '#';
		/* the table: one entry per operation of length > 0, columns ascending from 0 */
		uint32_t kept = 0; for(uint32_t w : cig) kept += (w >> 4) ? 1u : 0u;
		ok = ok && n_ent == kept && (n_ent == 0 || WTZ_PWT_COL(tab[0]) == 0);
		for(uint32_t k = 1; k < n_ent; k++) ok = ok && WTZ_PWT_COL(tab[k]) > WTZ_PWT_COL(tab[k - 1]);
		if(n_ent){ const uint32_t c = rnd(cols), e = wtz_pwtext_find(tab, n_ent, c); ok = ok && WTZ_PWT_COL(tab[e]) <= c && (e + 1 == n_ent || WTZ_PWT_COL(tab[e + 1]) > c); }
		if(!ok){ bad++; if(bad <= 5) fprintf(stderr, "alignment %u (%u columns, %zu operations, style %u) differs\n", it, cols, cig.size(), style); }
		n_aln++;
		free(d_cig); free(tab); free(text);
	}
	printf("%u alignments, %u bad\n", n_aln, bad);
	return bad ? 1 : 0;
}
