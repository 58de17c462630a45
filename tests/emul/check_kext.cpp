/* wtz_kext_problem<C> (wtz_sw_kext.h, the one-lane host form) of all six C against a plain scalar restatement of ksw_extend2, written here from
 * kextvec.py_extend (tests/kextvec.py): the six ints, the rows entered and their cells.  A few hundred seeded problems: 64 C - 1, 64 C and 64 C + 1 live diagonals
 * for every C, mutated copies, unrelated pairs, cut copies, two-letter alphabets, every start score / z-drop / end bonus / gap setting of kextvec; both strands and
 * the complement on either side; every problem in an array of its own that has exactly the words its bases need, a third of them with the query's view on the
 * first base of the array and the target's on the last.  Each problem runs in the form the host would choose and in every wider one: the result must not depend on C.
 * The lane-crossing primitives are the identity here (one lane): only the device run covers them. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define WTZ_EMUL 1
#include "wtz_sw_kext.h"

struct ref_out { int32_t six[6]; uint32_t rows; unsigned long long cells; };
static int32_t imax(int32_t a, int32_t b){ return a > b ? a : b; }
static int32_t imin(int32_t a, int32_t b){ return a < b ? a : b; }
static int32_t clamp_w(int32_t qlen, const wtz_kextsc_t &S, int32_t w, int32_t end_bonus){
	const int32_t mxs = imax(S.M, S.X);
	w = imin(w, imax(1, (int32_t)((double)(qlen * mxs + end_bonus - S.o_ins) / S.e_ins + 1.)));
	return imin(w, imax(1, (int32_t)((double)(qlen * mxs + end_bonus - S.o_del) / S.e_del + 1.)));
}
/* kextvec.py_extend, line by line */
static ref_out ref_extend(const std::vector<uint8_t> &q, const std::vector<uint8_t> &t, const wtz_kextsc_t &S, int32_t w, int32_t end_bonus, int32_t h0){
	const int32_t qlen = (int32_t)q.size(), tlen = (int32_t)t.size(), oe_del = S.o_del + S.e_del, oe_ins = S.o_ins + S.e_ins;
	h0 = imax(h0, 0);
	std::vector<int32_t> eh_h(qlen + 2, 0), eh_e(qlen + 2, 0);
	eh_h[0] = h0; eh_h[1] = h0 > oe_ins ? h0 - oe_ins : 0;
	for(int32_t j = 2; j <= qlen && eh_h[j - 1] > S.e_ins; j++) eh_h[j] = eh_h[j - 1] - S.e_ins;
	w = clamp_w(qlen, S, w, end_bonus);
	int32_t mx = h0, max_i = -1, max_j = -1, max_ie = -1, gscore = -1, max_off = 0, beg = 0, end = qlen;
	ref_out r; r.rows = 0; r.cells = 0;
	for(int32_t i = 0; i < tlen; i++){
		int32_t f = 0, m = 0, mj = -1, h1 = imax(0, h0 - (S.o_del + S.e_del * (i + 1)));
		beg = imax(beg, i - w); end = imin(imin(end, i + w + 1), qlen);
		r.rows++; r.cells += (unsigned long long)imax(0, end - beg);
		int32_t j = beg;
		for(; j < end; j++){
			int32_t Mv = eh_h[j]; const int32_t e = eh_e[j];
			eh_h[j] = h1;
			Mv += q[j] == t[i] ? S.M : S.X;
			const int32_t h = imax(imax(Mv, e), f);
			h1 = h;
			if(!(m > h)) mj = j;
			m = imax(m, h);
			eh_e[j] = imax(e - S.e_del, imax(Mv - oe_del, 0));
			f = imax(f - S.e_ins, imax(Mv - oe_ins, 0));
		}
		eh_h[end] = h1; eh_e[end] = 0;
		if(j == qlen){ if(!(gscore > h1)) max_ie = i; gscore = imax(gscore, h1); }
		if(m == 0) break;
		if(m > mx){ mx = m; max_i = i; max_j = mj; max_off = imax(max_off, abs(mj - i)); }
		else if(S.zdrop > 0){
			if(i - max_i > mj - max_j){ if(mx - m - ((i - max_i) - (mj - max_j)) * S.e_del > S.zdrop) break; }
			else if(mx - m - ((mj - max_j) - (i - max_i)) * S.e_ins > S.zdrop) break;
		}
		for(j = mj; j >= beg && eh_h[j]; j--){}
		beg = j + 1;
		for(j = mj + 2; j <= end && eh_h[j]; j++){}
		end = j;
	}
	const int32_t six[6] = {mx, max_j + 1, max_i + 1, max_ie + 1, gscore, max_off};
	memcpy(r.six, six, sizeof six);
	return r;
}

static uint32_t rnd(uint32_t n){ return (uint32_t)(lrand48() % (long)n); }
static std::vector<uint8_t> rseq(int n, int k){ std::vector<uint8_t> s(n); for(auto &b : s) b = (uint8_t)rnd(k); return s; }
static std::vector<uint8_t> mutate(const std::vector<uint8_t> &s, double rate, int k){
	std::vector<uint8_t> o;
	for(size_t i = 0; i < s.size(); ){
		const double r = drand48();
		if(r < rate * 0.4){ for(int c = 1 + (drand48() < 0.2 ? 1 + (int)rnd(7) : 0); c > 0; c--) o.push_back((uint8_t)rnd(k)); }
		else if(r < rate * 0.8){ i += 1 + (drand48() < 0.2 ? 1 + rnd(7) : 0); continue; }
		else if(r < rate){ o.push_back((uint8_t)((s[i] + 1 + rnd(k - 1)) % k)); i++; continue; }
		o.push_back(s[i]); i++;
	}
	if(o.empty()) o.push_back(0);
	return o;
}
static void fit(std::vector<uint8_t> &s, int n, int k){ while((int)s.size() < n) s.push_back((uint8_t)rnd(k)); s.resize(n); }
/* base i of the array: bits ((~i) & 31) * 2 of word i / 32 (the layout of hipabi.pack_reads) */
static void put(uint64_t *bits, long i, uint32_t b){ const int sh = (int)((~i) & 31) * 2; bits[i >> 5] = (bits[i >> 5] & ~(3ull << sh)) | ((uint64_t)b << sh); }

template<int C> static void run(const wtz_kextprob_t &p, const wtz_kextsc_t &S, wtz_kextres_t &r){ wtz_kext_problem<C>(p, S, r); }

int main(){
	srand48(11);
	static const int32_t GAPS[4][4] = {{3, 1, 3, 1}, {2, 1, 3, 1}, {3, 1, 2, 1}, {4, 2, 4, 2}}, H0S[] = {-5, 0, 1, 30, 400, 5000, 32767}, EB[] = {0, 30, 100}, ZD[] = {-1, 40};
	static const int FORMS[6] = {1, 2, 4, 8, 16, 32};
	long n = 0, bad = 0, runs = 0, per_form[6] = {0, 0, 0, 0, 0, 0}, stops[2] = {0, 0};
	std::vector<int> edge;
	for(int c = 1; c <= 16; c <<= 1) for(int d = -1; d <= 1; d++) edge.push_back(64 * c + d);
	edge.push_back(2047);
	for(int it = 0; it < 420; it++){
		wtz_kextsc_t S; S.M = 2; S.X = -5; const int g = (int)rnd(4);
		S.o_del = GAPS[g][0]; S.e_del = GAPS[g][1]; S.o_ins = GAPS[g][2]; S.e_ins = GAPS[g][3]; S.zdrop = ZD[rnd(2)];
		const int32_t end_bonus = EB[rnd(3)]; int32_t h0 = H0S[rnd(7)], w;
		const int k = it % 3 == 0 ? 2 : 4;
		std::vector<uint8_t> q, t;
		if(it < 6 * (int)edge.size()){      /* the form edges: symmetric bands for odd counts, a short target or a short query otherwise */
			const int Sl = edge[it / 6], shape = Sl == 2047 ? 0 : ((Sl & 1) ? it % 3 : 1 + it % 2);
			int ql, tl;
			if(shape == 0){ w = (Sl - 1) / 2; ql = w + 1 + (int)rnd(40); tl = w + 1 + (int)rnd(40); }
			else { w = imin(1023, Sl / 2 + 1 + (int)rnd(imax(2, Sl / 8))); const int sh = Sl - w, ot = w + 1 + (int)rnd(40); if(shape == 1){ ql = ot; tl = sh; } else { ql = sh; tl = ot; } }
			q = rseq(ql, k); t = (it % 6 == 5) ? rseq(tl, k) : mutate(q, 0.12, k); fit(t, tl, k);
			S.o_del = S.o_ins = 3; S.e_del = S.e_ins = 1;      /* the clamp must not bite here */
		} else {
			static const int WS[] = {0, 1, 3, 10, 31, 32, 33, 40, 100, 127, 128, 300, 512, 800, 1023};
			w = WS[rnd(15)];
			const int hi = w >= 300 ? 1500 : (w >= 100 ? 500 : 200);
			q = rseq(1 + (int)rnd(hi), k);
			if(it % 4 == 0) t = rseq(1 + (int)rnd(hi), k);
			else {
				t = mutate(q, it % 3 == 0 ? 0.12 : (it % 3 == 1 ? 0.25 : 0.35), k);
				if(it & 1){ t.resize(1 + rnd((uint32_t)t.size())); fit(t, (int)t.size() + 1 + (int)rnd(hi / 2 + w), k); }
			}
		}
		/* the two views in an array of exactly the words the bases need */
		const int qs = (it & 1) ? -1 : 1, ts = (it & 2) ? -1 : 1; const uint32_t qc = (it >> 2) & 1, tc = (it >> 3) & 1;
		const bool tight = it % 3 == 1;
		const long padl = tight ? 0 : rnd(70), padm = rnd(70), padr = tight ? 0 : rnd(70);
		const long NB = padl + (long)q.size() + padm + (long)t.size() + padr, NW = (NB + 31) / 32;
		uint64_t *bits = (uint64_t*)malloc((size_t)NW * 8);
		for(long i = 0; i < NW; i++) bits[i] = ((uint64_t)lrand48() << 33) ^ ((uint64_t)lrand48() << 11) ^ (uint64_t)lrand48();
		wtz_kextprob_t p;
		p.q.bits = p.t.bits = bits; p.q.strand = qs; p.t.strand = ts; p.q.comp = qc; p.t.comp = tc;
		p.q.start = qs > 0 ? padl : padl + (long)q.size() - 1;
		const long t0 = padl + (long)q.size() + padm;
		p.t.start = ts > 0 ? t0 : t0 + (long)t.size() - 1;
		for(size_t i = 0; i < q.size(); i++) put(bits, p.q.start + qs * (long)i, qc ? 3u - q[i] : q[i]);
		for(size_t i = 0; i < t.size(); i++) put(bits, p.t.start + ts * (long)i, tc ? 3u - t[i] : t[i]);
		for(size_t i = 0; i < q.size(); i++) if(p.q.at((int32_t)i) != q[i]){ printf("view of q broken\n"); return 2; }
		for(size_t i = 0; i < t.size(); i++) if(p.t.at((int32_t)i) != t[i]){ printf("view of t broken\n"); return 2; }
		/* the plan of the host (kext_plan, kext_slots) */
		p.qlen = (int32_t)q.size(); p.tlen = (int32_t)t.size(); p.h0 = h0 < 0 ? 0 : h0; p.w = clamp_w(p.qlen, S, w, end_bonus); p.dlo = imin(p.w, p.tlen - 1);
		const int32_t slots = p.dlo + imin(p.w, p.qlen - 1) + 1, form = wtz_kext_form(slots);
		if(it < 6 * (int)edge.size() && slots != edge[it / 6]){ printf("edge problem %d has %d slots, not %d\n", it, slots, edge[it / 6]); return 2; }
		const ref_out ref = ref_extend(q, t, S, w, end_bonus, h0);
		n++;
		for(int fi = 0; fi < 6; fi++){
			if(FORMS[fi] < form) continue;
			wtz_kextres_t r; memset(&r, 0, sizeof r);
			switch(FORMS[fi]){ case 1: run<1>(p, S, r); break; case 2: run<2>(p, S, r); break; case 4: run<4>(p, S, r); break; case 8: run<8>(p, S, r); break; case 16: run<16>(p, S, r); break; default: run<32>(p, S, r); }
			runs++; if(FORMS[fi] == form) per_form[fi]++;
			const int32_t got[6] = {r.score, r.qle, r.tle, r.gtle, r.gscore, r.max_off};
			if(memcmp(got, ref.six, sizeof got) || r.rows != ref.rows || r.cells != ref.cells){
				if(bad < 8) printf("MISMATCH problem %d C %d (form %d, %d slots) q %d t %d w %d h0 %d: got %d %d %d %d %d %d rows %u cells %llu, expected %d %d %d %d %d %d rows %u cells %llu\n", it, FORMS[fi], form, slots,
					p.qlen, p.tlen, w, h0, got[0], got[1], got[2], got[3], got[4], got[5], r.rows, r.cells, ref.six[0], ref.six[1], ref.six[2], ref.six[3], ref.six[4], ref.six[5], ref.rows, ref.cells);
				bad++;
			}
		}
		stops[ref.rows == (uint32_t)p.tlen ? 0 : 1]++;
		free(bits);
	}
	printf("problems by the form the host chooses, C = 1 ... 32: %ld %ld %ld %ld %ld %ld; ran to the last row %ld, stopped before it %ld\n", per_form[0], per_form[1], per_form[2], per_form[3], per_form[4], per_form[5], stops[0], stops[1]);
	for(int fi = 0; fi < 6; fi++) if(per_form[fi] < 10){ printf("form %d has too few problems\n", FORMS[fi]); return 2; }
	printf("%ld problems, %ld runs, %ld bad\n", n, runs, bad);
	return bad != 0;
}
