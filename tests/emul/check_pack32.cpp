/* wtz_pack32 (wtz_sw.h) and wtz_kext_bases (wtz_sw_kext.h) against 32 single-base extractions: every first base b0 in [0, len + 40) of a view, K-kext's
 * negative first bases in [-70, 0), both strands, complement, and views that touch the first and the last base of an array that has exactly the words
 * hipabi.pack_reads hands over ((bases + 31) / 32, nothing behind them): a word load that leaves the array is an error a sanitizer build of this program reports. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define WTZ_EMUL 1
#include "wtz_sw_kext.h"
static long bad = 0, n = 0;
static void check(const wtz_seq_packed &s, int len, int b0, bool kext){
	uint64_t ref = 0; for(int k = 0; k < 32; k++) if(b0 + k >= 0 && b0 + k < len) ref |= ((uint64_t)s.at(b0 + k)) << (2 * k);
	const uint64_t got = kext ? wtz_kext_bases(s, b0, len) : wtz_pack32(s, b0, len);
	n++; if(ref != got){ if(bad < 5) printf("MISMATCH %s strand %d comp %u start %ld len %d b0 %d ref %016lx got %016lx\n", kext ? "wtz_kext_bases" : "wtz_pack32", s.strand, s.comp, (long)s.start, len, b0, (unsigned long)ref, (unsigned long)got); bad++; }
}
static void check_view(const wtz_seq_packed &s, int len){
	for(int b0 = 0; b0 < len + 40; b0++) check(s, len, b0, false);
	for(int b0 = -70; b0 < len + 40; b0++) check(s, len, b0, true);
}
int main(){
	srand48(5);
	/* array sizes around a word boundary: the last word full, holding one base, holding 31 */
	const int NBS[] = {4992, 4993, 5000, 5023, 5024, 5025, 33, 32, 31, 1};
	for(int NB : NBS){
		const int NW = (NB + 31) / 32;
		uint64_t *bits = (uint64_t*)malloc((size_t)NW * 8);
		for(int i = 0; i < NW; i++) bits[i] = ((uint64_t)lrand48() << 33) ^ ((uint64_t)lrand48() << 11) ^ (uint64_t)lrand48();
		for(int it = 0; it < 400; it++){
			wtz_seq_packed s; s.bits = bits; s.strand = (lrand48() & 1) ? 1 : -1; s.comp = lrand48() & 1;
			int len = 1 + lrand48() % 300; if(len > NB) len = NB;
			const int where = it % 4;      /* 0, 1: anywhere; 2: the view touches the first base of the array; 3: its last base */
			const long lo = where == 2 ? 0 : (where == 3 ? NB - len : lrand48() % (NB - len + 1));      /* lowest base of the view */
			s.start = s.strand > 0 ? lo : lo + len - 1;
			check_view(s, len);
		}
		free(bits);
	}
	printf("%ld tests, %ld bad\n", n, bad);
	return bad != 0;
}
