/* wtz_pair_order (wtz_tasks.h), the block -> pair map of the K_pair / K_pair_dm launches: for every (xg, nh, n_rest) of the grid below, with and without a
 * heavy-first list, the map is a bijection on [0, nh + n_rest), blocks below nh go through `ord` unchanged, the blocks behind them are the XCD order of the
 * plan positions nh .. n - 1 (the identity with xg = 0), and a list is applied behind the XCD order.  The image for xg = 3, nh = 0, n_rest = 29 is printed: the
 * test compares it with the list written out from the expression the launches used to carry. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <vector>
#include <atomic>
#include <algorithm>
#define WTZ_EMUL 1
#include "wtz_tasks.h"
static long bad = 0, n_cases = 0;
static void fail(const char *what, uint32_t xg, uint64_t nh, uint64_t n_rest, uint64_t b){
	if(bad++ < 8) printf("BAD %s: xg %u nh %llu n_rest %llu block %llu\n", what, xg, (unsigned long long)nh, (unsigned long long)n_rest, (unsigned long long)b);
}
static void check(uint32_t xg, uint64_t nh, uint64_t n_rest){
	const uint64_t n = nh + n_rest;
	std::vector<uint32_t> ord(n);
	for(uint64_t i = 0; i < n; i++) ord[i] = (uint32_t)(n - 1 - i);          /* a list that moves every position */
	const wtz_pair_order plain = { nh, n_rest, xg, NULL }, listed = { nh, n_rest, xg, ord.data() };
	std::vector<uint8_t> seen(n, 0), seen_l(n, 0);
	for(uint64_t b = 0; b < n; b++){
		const uint32_t t = plain(b), tl = listed(b);
		if(t >= n || seen[t]) fail("not a bijection", xg, nh, n_rest, b); else seen[t] = 1;
		if(tl >= n || seen_l[tl]) fail("not a bijection (list)", xg, nh, n_rest, b); else seen_l[tl] = 1;
		if(t < n && tl != ord[t]) fail("the list is not applied behind the XCD order", xg, nh, n_rest, b);
		if(b < nh && (t != b || tl != ord[b])) fail("a heavy block does not map through the list unchanged", xg, nh, n_rest, b);
		if(b >= nh && t < nh) fail("a block behind the heavy ones maps among them", xg, nh, n_rest, b);
		if(xg == 0 && t != b) fail("xg = 0 is not the identity", xg, nh, n_rest, b);
		if(xg && b >= nh){          /* full groups of 8 * xg: block r of a group takes position (r mod 8) * xg + r / 8 of it; the rest of the range keeps its place */
			const uint64_t per = 8ull * xg, b2 = b - nh, g = b2 / per, r = b2 % per;
			const uint64_t want = (g + 1) * per <= n_rest ? nh + g * per + (r % 8) * xg + r / 8 : b;
			if(t != want) fail("not the XCD order", xg, nh, n_rest, b);
		}
	}
	n_cases++;
}
int main(){
	const uint32_t XG[] = {0, 1, 3, 256};
	const uint64_t NH[] = {0, 8, 9};
	for(uint32_t xg : XG) for(uint64_t nh : NH){
		const long long per = 8ll * xg;
		const long long NR[] = {0, 1, per - 1, per, per + 1, 3 * per + 5};
		for(long long n_rest : NR) if(n_rest >= 0) check(xg, nh, (uint64_t)n_rest);
	}
	const wtz_pair_order o = { 0, 29, 3, NULL };
	printf("image xg 3 nh 0 n_rest 29:");
	for(uint64_t b = 0; b < 29; b++) printf(" %u", o(b));
	printf("\n%ld cases, %ld bad\n", n_cases, bad);
	return bad != 0;
}
