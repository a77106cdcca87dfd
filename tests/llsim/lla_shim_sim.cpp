// TEST INFRASTRUCTURE: k2a_shim_launch_ll_rev (ksw2_shim.h) on the host -- the start-cell pass of ksw2amd_ll_align_batch: the REV form of
// the local-alignment lane code (ksw2_lane_ll.h) for 64 lanes in lock step with the kernel's schedule (k2a_ll_rev_kernel): limits read from
// the forward results, the bounding rectangle of the two halves, reversed row / column indexing with clamped loads, DPP rotate of the
// bottom row, lane 63 -> boundary -> lane 0 across generations, one key reduction per task.  Linked by tests/lla_util.py next to
// tests/llsim/ll_shim_sim.cpp, tests/sim/ksw2_shim_sim.cpp and the product's host objects.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

template<bool PK, bool LDSP>
static void lla_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, const K2aLLRes *fres, K2aLLBeg *beg)
{
	static K2aLaneLL<PK, LDSP, true> L[64];
	const int NH = PK ? 2 : 1;
	const int mm = par.m * par.m;
	const uint8_t *ltab = tab + (tk.swapped ? mm : 0);
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	int rl[2] = { 0, 0 }, cl[2] = { 0, 0 }, fq[2] = { 0, 0 }, ft[2] = { 0, 0 };
	for (int h = 0; h < NH; ++h) {
		const K2aLLRes r = fres[tk.res[h]];
		const bool pos = r.score > 0;
		fq[h] = r.qe; ft[h] = r.te;
		rl[h] = pos ? (tk.swapped ? r.qe : r.te) + 1 : 0;
		cl[h] = pos ? (tk.swapped ? r.te : r.qe) + 1 : 0;
		rl[h] = k2a_min(rl[h], tk.nrows); cl[h] = k2a_min(cl[h], tk.ncols);
	}
	for (int l = 0; l < 64; ++l) { L[l].init(par, tk, l); L[l].set_limits(rl, cl); }
	const int ncols = L[0].ncols, ngen = (L[0].nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	const int cl0 = cl[0], cl1 = cl[PK ? 1 : 0];
	for (int g = 0; g < ngen; ++g) {
		const bool from_bnd = g > 0, to_bnd = g + 1 < ngen;
		uint32_t hin[64] = { 0 }, ein[64] = { 0 }, ho[64], eo[64];
		for (int l = 0; l < 64; ++l) L[l].gen_begin(g, r0, r1, ltab);
		for (int k = 0; k < nsteps; ++k) {
			for (int l = 0; l < 64; ++l) {
				const int jj = k - l;
				ho[l] = eo[l] = 0;
				if (jj < 0 || jj >= ncols) continue;
				uint32_t h = hin[l], e = ein[l];
				if (l == 0) { h = from_bnd ? bnd[2 * jj] : 0u; e = from_bnd ? bnd[2 * jj + 1] : 0u; }
				const int j0 = k2a_max(cl0 - 1 - jj, 0), j1 = k2a_max(cl1 - 1 - jj, 0);
				const uint32_t qc = PK ? (uint32_t)c0[j0] | ((uint32_t)c1[j1] << 8) : (uint32_t)c0[j0];
				L[l].step(jj, h, e, qc, ltab, ho[l], eo[l]);
				if (to_bnd && l == 63) { bnd[2 * jj] = ho[l]; bnd[2 * jj + 1] = eo[l]; }
			}
			for (int l = 0; l < 64; ++l) { hin[l] = ho[(l + 63) & 63]; ein[l] = eo[(l + 63) & 63]; }   // wave_ror:1
		}
		for (int l = 0; l < 64; ++l) L[l].gen_end();
	}
	for (int h = 0; h < NH; ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) {
			K2aLLBeg b;
			b.score = k.s; b.qb = k.s > 0 ? fq[h] - k.qe : -1; b.tb = k.s > 0 ? ft[h] - k.te : -1;
			beg[tk.res[h]] = b;
		}
	}
}

extern "C" int k2a_shim_launch_ll_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                      uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	for (int t = 0; t < ntasks; ++t) {
		if (pk && lds) lla_task<true, true>(*par, tasks[t], seq, tab, scratch, res, beg);
		else if (pk) lla_task<true, false>(*par, tasks[t], seq, tab, scratch, res, beg);
		else if (lds) lla_task<false, true>(*par, tasks[t], seq, tab, scratch, res, beg);
		else lla_task<false, false>(*par, tasks[t], seq, tab, scratch, res, beg);
	}
	return 0;
}
