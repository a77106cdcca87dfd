// TEST INFRASTRUCTURE: the host twins of the packed 16-bit helpers of ksw2_lane_ll.h against their plain definitions, and the bytes of
// the register column profile that lie past the alphabet.  No admitted input can tell a wrapping add from a saturating one (the host
// admits a pair only while H + smax <= 65535) or reach a profile byte k >= m (a column code is < m), so both are checked here, directly.
// Compiled and run by tests/test_local_edges_cpu.py; prints the first difference and returns 1.  Never shipped.
#include <stdio.h>
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

static int sat(int v) { return v < 0 ? 0 : v > 0xffff ? 0xffff : v; }

static int check_ops()
{
	static const uint32_t v[] = { 0, 1, 2, 84, 85, 127, 254, 255, 256, 0x7fff, 0x8000, 0x8001, 65450, 65534, 65535 };
	const int n = (int)(sizeof(v) / sizeof(v[0]));
	for (int a = 0; a < n; ++a)
		for (int b = 0; b < n; ++b)
			for (int c = 0; c < n; c += 3) {
				const uint32_t x = v[a] | (v[c] << 16), y = v[b] | (v[(c + a) % n] << 16);
				const int xl = (int)v[a], xh = (int)v[c], yl = (int)v[b], yh = (int)v[(c + a) % n];
				const uint32_t add = (uint32_t)sat(xl + yl) | ((uint32_t)sat(xh + yh) << 16), sub = (uint32_t)sat(xl - yl) | ((uint32_t)sat(xh - yh) << 16);
				const uint32_t mx = (uint32_t)(xl > yl ? xl : yl) | ((uint32_t)(xh > yh ? xh : yh) << 16), mn = (uint32_t)(xl < yl ? xl : yl) | ((uint32_t)(xh < yh ? xh : yh) << 16);
				if (k2a_ll_adds(x, y) != add) { printf("adds(%08x, %08x) = %08x, expected %08x\n", x, y, k2a_ll_adds(x, y), add); return 1; }
				if (k2a_ll_subs(x, y) != sub) { printf("subs(%08x, %08x) = %08x, expected %08x\n", x, y, k2a_ll_subs(x, y), sub); return 1; }
				if (k2a_ll_max(x, y) != mx) { printf("max(%08x, %08x) = %08x, expected %08x\n", x, y, k2a_ll_max(x, y), mx); return 1; }
				if (k2a_ll_min(x, y) != mn) { printf("min(%08x, %08x) = %08x, expected %08x\n", x, y, k2a_ll_min(x, y), mn); return 1; }
			}
	/* the row maximum's mask: all ones in a half whose difference is > 0 */
	if (k2a_ll_mul(k2a_ll_min(0x00050000u, 0x10001u), 0xffffffffu) != 0xffff0000u || k2a_ll_mul(k2a_ll_min(0x0000ffffu, 0x10001u), 0xffffffffu) != 0x0000ffffu) {
		printf("mask multiply\n"); return 1;
	}
	if (k2a_ll_perm(0x07060504u, 0x03020100u, 0x0c05000cu) != 0x00050000u) { printf("perm\n"); return 1; }
	return 0;
}

/* gen_begin with m < 4: the profile registers hold pen bytes of codes 0 .. m - 1 only -- byte k >= m of a row's word would come from
 * the next row of the table (or from behind it) */
template<bool PK>
static int check_profile(int m)
{
	uint8_t tab[2 * 5 * 5 + 8], rows[K2A_LL_ROWS];
	memset(tab, 0xee, sizeof(tab));
	for (int i = 0; i < K2A_LL_ROWS; ++i) rows[i] = (uint8_t)(i % m);
	K2aLL par = {}; par.m = m; par.smax = 5; par.oe = 3; par.ge = 1;
	K2aLLTask tk; memset(&tk, 0, sizeof(tk)); tk.nrows = K2A_LL_ROWS; tk.ncols = 4;
	K2aLaneLL<PK, false> L;
	L.init(par, tk, 63);
	L.gen_begin(0, rows, rows, tab);
	const uint32_t live = m >= 4 ? 0xffffffffu : (1u << (8 * m)) - 1u;
	for (int c = 0; c < K2A_LL_C; ++c) {
		if ((L.pa[c] & ~live) != 0 || (PK && (L.pb[PK ? c : 0] & ~live) != 0)) { printf("m = %d: profile word %08x holds a byte past the alphabet\n", m, L.pa[c]); return 1; }
		if ((L.pa[c] & live) != (0xeeeeeeeeu & live)) { printf("m = %d: profile word %08x\n", m, L.pa[c]); return 1; }
		if (m < 5 && L.pw[c] != 0) { printf("m = %d: code-4 word %08x\n", m, L.pw[c]); return 1; }
	}
	return 0;
}

int main()
{
	if (check_ops()) return 1;
	for (int m = 1; m <= 5; ++m) if (check_profile<false>(m) || check_profile<true>(m)) return 1;
	printf("ok\n");
	return 0;
}
