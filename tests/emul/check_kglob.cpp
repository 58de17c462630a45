/* wtz_kglob_problem<C> (wtz_sw_kglob.h, the one-lane host form) of all six C against a plain scalar restatement of ksw_global2 written here from the text of
 * ksw.c:503-586 (boundary rows, the tie rules m >= e, h >= f, e > t, f > t, the walk with its two tails): score, run list word for word, matches and
 * mismatches of the op-0 runs, cells.  Seeded problems: 64 C - 1, 64 C and 64 C + 1 band slots for every C and 2 047, copies, mutated copies, unrelated pairs,
 * all-A pairs, two-letter alphabets, |qlen - tlen| = w, w = 0, every gap setting of kglobvec.GAPS; both strands and the complement on either side; every
 * problem in an array of exactly the words its bases need, with a trace and a run buffer of exactly the words the host plans (the sanitizer sees every
 * index).  Each problem runs in the form the host would choose and in every wider one: the result must not depend on C.  The lane-crossing primitives
 * are the identity here (one lane): only the device run covers them.
 *     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -DWTZ_EMUL -I include -I smartdenovo_amd/csrc tests/emul/check_kglob.cpp -o check_kglob && ./check_kglob */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define WTZ_EMUL 1
#include "wtz_sw_kglob.h"

static const int32_t NEG = -0x40000000;
struct ref_out { int32_t score, mat, mis; unsigned long long cells; std::vector<uint32_t> cigar; };
static void push(std::vector<uint32_t> &c, uint32_t op, uint32_t len){ if(!c.empty() && (c.back() & 0xFu) == op) c.back() += len << 4; else c.push_back(len << 4 | op); }
static ref_out ref_global(const std::vector<uint8_t> &q, const std::vector<uint8_t> &t, const wtz_kglobsc_t &S, int32_t w){
	const int32_t qlen = (int32_t)q.size(), tlen = (int32_t)t.size(), oe_del = S.o_del + S.e_del, oe_ins = S.o_ins + S.e_ins;
	const int32_t n_col = qlen < 2 * w + 1 ? qlen : 2 * w + 1;
	std::vector<int32_t> eh_h(qlen + 1), eh_e(qlen + 1);
	std::vector<uint8_t> z((size_t)n_col * tlen);
	ref_out r; r.cells = 0;
	int32_t j;
	eh_h[0] = 0; eh_e[0] = NEG;
	for(j = 1; j <= qlen && j <= w; j++){ eh_h[j] = -(S.o_ins + S.e_ins * j); eh_e[j] = NEG; }
	for(; j <= qlen; j++) eh_h[j] = eh_e[j] = NEG;
	for(int32_t i = 0; i < tlen; i++){
		int32_t f = NEG, beg = i > w ? i - w : 0, end = i + w + 1 < qlen ? i + w + 1 : qlen;
		int32_t h1 = beg == 0 ? -(S.o_del + S.e_del * (i + 1)) : NEG;
		r.cells += (unsigned long long)(end > beg ? end - beg : 0);
		for(j = beg; j < end; j++){
			int32_t m = eh_h[j], e = eh_e[j], h, tt; uint8_t d;
			eh_h[j] = h1;
			m += q[j] == t[i] ? S.M : S.X;
			d = m >= e ? 0 : 1; h = m >= e ? m : e;
			d = h >= f ? d : 2; h = h >= f ? h : f;
			h1 = h;
			tt = m - oe_del; e -= S.e_del; d |= e > tt ? 1 << 2 : 0; e = e > tt ? e : tt; eh_e[j] = e;
			tt = m - oe_ins; f -= S.e_ins; d |= f > tt ? 2 << 4 : 0; f = f > tt ? f : tt;
			z[(size_t)i * n_col + (j - beg)] = d;
		}
		eh_h[end] = h1; eh_e[end] = NEG;
	}
	r.score = eh_h[qlen];
	int32_t i = tlen - 1, k = (i + w + 1 < qlen ? i + w + 1 : qlen) - 1, which = 0;
	while(i >= 0 && k >= 0){
		which = z[(size_t)i * n_col + (k - (i > w ? i - w : 0))] >> (which << 1) & 3;
		if(which == 0){ push(r.cigar, 0, 1); --i; --k; }
		else if(which == 1){ push(r.cigar, 2, 1); --i; }
		else { push(r.cigar, 1, 1); --k; }
	}
	if(i >= 0) push(r.cigar, 2, (uint32_t)(i + 1));
	if(k >= 0) push(r.cigar, 1, (uint32_t)(k + 1));
	for(size_t a = 0, b = r.cigar.size(); a + 1 < b; a++, b--){ const uint32_t x = r.cigar[a]; r.cigar[a] = r.cigar[b - 1]; r.cigar[b - 1] = x; }
	r.mat = r.mis = 0;
	int32_t x1 = 0, x2 = 0;
	for(uint32_t c : r.cigar){ const int32_t len = (int32_t)(c >> 4); if((c & 0xFu) == 0){ for(int32_t a = 0; a < len; a++){ if(q[x1 + a] == t[x2 + a]) r.mat++; else r.mis++; } x1 += len; x2 += len; } else if((c & 0xFu) == 1) x1 += len; else x2 += len; }
	return r;
}

static uint32_t rnd(uint32_t n){ return (uint32_t)(lrand48() % (long)n); }
static std::vector<uint8_t> rseq(int n, int k){ std::vector<uint8_t> s(n); for(auto &b : s) b = (uint8_t)rnd(k); return s; }
static std::vector<uint8_t> mutate(const std::vector<uint8_t> &s, double rate, int k){
	std::vector<uint8_t> o;
	for(size_t i = 0; i < s.size(); ){
		const double r = drand48();
		if(r < rate * 0.3){ for(int c = 1 + (drand48() < 0.2 ? 1 + (int)rnd(7) : 0); c > 0; c--) o.push_back((uint8_t)rnd(k)); }
		else if(r < rate * 0.6){ i += 1 + (drand48() < 0.2 ? 1 + rnd(7) : 0); continue; }
		else if(r < rate){ o.push_back((uint8_t)((s[i] + 1 + rnd(k - 1)) % k)); i++; continue; }
		o.push_back(s[i]); i++;
	}
	if(o.empty()) o.push_back(0);
	return o;
}
static void fit(std::vector<uint8_t> &s, int n, int k){ while((int)s.size() < n) s.push_back((uint8_t)rnd(k)); s.resize(n); }
static void put(uint64_t *bits, long i, uint32_t b){ const int sh = (int)((~i) & 31) * 2; bits[i >> 5] = (bits[i >> 5] & ~(3ull << sh)) | ((uint64_t)b << sh); }

template<int C> static void run(wtz_kglobprob_t p, const wtz_kglobsc_t &S, wtz_kglobres_t &r, std::vector<uint32_t> &runs){
	std::vector<uint32_t> tr((size_t)wtz_kglob_trace_words(C, p.tlen)), stg(WTZ_KGLOB_STAGE_WORDS);
	runs.assign(p.run_cap, 0);
	wtz_kglob_problem<C>(p, S, tr.data(), runs.data(), stg.data(), r);
}

int main(){
	srand48(13);
	static const int32_t GAPS[4][4] = {{3, 1, 3, 1}, {2, 1, 4, 1}, {3, 1, 3, 2}, {0, 1, 0, 1}};
	static const int FORMS[6] = {1, 2, 4, 8, 16, 32};
	long n = 0, bad = 0, nruns = 0, per_form[6] = {0, 0, 0, 0, 0, 0};
	std::vector<int> edge;
	for(int c = 1; c <= 16; c <<= 1) for(int d = -1; d <= 1; d++) edge.push_back(64 * c + d);
	edge.push_back(2047);
	for(int it = 0; it < 400; it++){
		wtz_kglobsc_t S; S.M = 2; S.X = -5; const int g = (int)rnd(4);
		S.o_del = GAPS[g][0]; S.e_del = GAPS[g][1]; S.o_ins = GAPS[g][2]; S.e_ins = GAPS[g][3];
		const int k = it % 3 == 0 ? 2 : 4;
		int ql, tl, w;
		if(it < 6 * (int)edge.size()){      /* the form edges: symmetric bands for odd counts, a short target or a short query otherwise */
			const int Sl = edge[it / 6], shape = (Sl & 1) ? it % 3 : 1 + it % 2;
			if(shape == 0){ w = (Sl - 1) / 2; tl = w + 1 + (int)rnd(40); ql = tl + (int)rnd(w < 9 ? w + 1 : 10); }
			else { const int sh = Sl / 3 > 2 ? Sl / 3 : 2; w = Sl - sh; const int ot = w + 1 + (int)rnd(sh); if(shape == 1){ ql = sh; tl = ot; } else { ql = ot; tl = sh; } }
		} else {
			static const int WS[] = {0, 1, 3, 10, 31, 32, 33, 40, 100, 127, 128, 300, 512, 800, 1023};
			w = WS[rnd(15)];
			ql = 1 + (int)rnd(w >= 300 ? 1500 : (w >= 100 ? 500 : 200));
			const int d = w ? (it % 5 == 0 ? w : (int)rnd(w + 1)) : 0;      /* every fifth: the corner on the band's edge */
			tl = (it & 1) ? ql + d : ql - d; if(tl < 1) tl = ql + d;
		}
		std::vector<uint8_t> q = it % 7 == 3 ? std::vector<uint8_t>(ql, 0) : rseq(ql, k), t;
		if(it % 7 == 3) t = std::vector<uint8_t>(tl, 0);
		else if(it % 4 == 0) t = rseq(tl, k);
		else { t = it % 4 == 1 ? q : mutate(q, it % 4 == 2 ? 0.12 : 0.3, k); fit(t, tl, k); }
		const int qs = (it & 1) ? -1 : 1, ts = (it & 2) ? -1 : 1; const uint32_t qc = (it >> 2) & 1, tc = (it >> 3) & 1;
		const bool tight = it % 3 == 1;
		const long padl = tight ? 0 : rnd(70), padm = rnd(70), padr = tight ? 0 : rnd(70);
		const long NB = padl + ql + padm + tl + padr, NWD = (NB + 31) / 32;
		uint64_t *bits = (uint64_t*)malloc((size_t)NWD * 8);
		for(long i = 0; i < NWD; i++) bits[i] = ((uint64_t)lrand48() << 33) ^ ((uint64_t)lrand48() << 11) ^ (uint64_t)lrand48();
		wtz_kglobprob_t p; memset(&p, 0, sizeof p);
		p.q.bits = p.t.bits = bits; p.q.strand = qs; p.t.strand = ts; p.q.comp = qc; p.t.comp = tc;
		p.q.start = qs > 0 ? padl : padl + ql - 1;
		const long t0 = padl + ql + padm;
		p.t.start = ts > 0 ? t0 : t0 + tl - 1;
		for(int i = 0; i < ql; i++) put(bits, p.q.start + qs * (long)i, qc ? 3u - q[i] : q[i]);
		for(int i = 0; i < tl; i++) put(bits, p.t.start + ts * (long)i, tc ? 3u - t[i] : t[i]);
		p.qlen = ql; p.tlen = tl; p.w = w; p.dlo = w < tl - 1 ? w : tl - 1; p.run_cap = (uint32_t)(ql + tl);
		const int32_t slots = wtz_kglob_slots(ql, tl, w), form = wtz_kext_form(slots);
		if(it < 6 * (int)edge.size() && slots != edge[it / 6]){ printf("edge problem %d has %d slots, not %d\n", it, slots, edge[it / 6]); return 2; }
		const ref_out ref = ref_global(q, t, S, w);
		n++;
		for(int fi = 0; fi < 6; fi++){
			if(FORMS[fi] < form) continue;
			wtz_kglobres_t r; memset(&r, 0, sizeof r); std::vector<uint32_t> runs;
			switch(FORMS[fi]){ case 1: run<1>(p, S, r, runs); break; case 2: run<2>(p, S, r, runs); break; case 4: run<4>(p, S, r, runs); break; case 8: run<8>(p, S, r, runs); break; case 16: run<16>(p, S, r, runs); break; default: run<32>(p, S, r, runs); }
			nruns++; if(FORMS[fi] == form) per_form[fi]++;
			const bool same = !r.bad && r.score == ref.score && r.mat == ref.mat && r.mis == ref.mis && r.cells == ref.cells && r.n_runs == ref.cigar.size()
				&& r.runs == runs.data() + (runs.size() - r.n_runs) && (r.n_runs == 0 || !memcmp(r.runs, ref.cigar.data(), (size_t)r.n_runs * 4));
			if(!same){
				if(bad < 8) printf("MISMATCH problem %d C %d (form %d, %d slots) q %d t %d w %d gaps %d: score %d / %d, runs %u / %zu, mat %d / %d, mis %d / %d, cells %llu / %llu\n", it, FORMS[fi], form, slots,
					ql, tl, w, g, r.score, ref.score, r.n_runs, ref.cigar.size(), r.mat, ref.mat, r.mis, ref.mis, r.cells, ref.cells);
				bad++;
			}
		}
		free(bits);
	}
	printf("problems by the form the host chooses, C = 1 ... 32: %ld %ld %ld %ld %ld %ld\n", per_form[0], per_form[1], per_form[2], per_form[3], per_form[4], per_form[5]);
	for(int fi = 0; fi < 6; fi++) if(per_form[fi] < 10){ printf("form %d has too few problems\n", FORMS[fi]); return 2; }
	printf("%ld problems, %ld runs, %ld bad\n", n, nruns, bad);
	return bad != 0;
}
