// TEST INFRASTRUCTURE: k2a_shim_launch_ll (ksw2_shim.h) on the host -- the local-alignment lane code (ksw2_lane_ll.h) for 64 lanes in
// lock step, with the kernel's schedule: DPP rotate of the bottom row, lane 63 -> boundary -> lane 0 across generations, one key
// reduction per task.  Linked by tests/test_local_cpu.py next to tests/sim/ksw2_shim_sim.cpp and the product's host objects.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

template<bool PK, bool LDSP>
static void ll_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, K2aLLRes *res)
{
	static K2aLaneLL<PK, LDSP> L[64];
	const int mm = par.m * par.m;
	const uint8_t *ltab = tab + (tk.swapped ? mm : 0);
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	const int ncols = tk.ncols, ngen = (tk.nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	for (int l = 0; l < 64; ++l) L[l].init(par, tk, l);
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
				const uint32_t qc = PK ? (uint32_t)c0[jj] | ((uint32_t)c1[jj] << 8) : (uint32_t)c0[jj];
				L[l].step(jj, h, e, qc, ltab, ho[l], eo[l]);
				if (to_bnd && l == 63) { bnd[2 * jj] = ho[l]; bnd[2 * jj + 1] = eo[l]; }
			}
			for (int l = 0; l < 64; ++l) { hin[l] = ho[(l + 63) & 63]; ein[l] = eo[(l + 63) & 63]; }   // wave_ror:1
		}
		for (int l = 0; l < 64; ++l) L[l].gen_end();
	}
	for (int h = 0; h < (PK ? 2 : 1); ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) { res[tk.res[h]].score = k.s; res[tk.res[h]].qe = k.qe; res[tk.res[h]].te = k.te; }
	}
}

extern "C" int k2a_shim_launch_ll(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                  uint8_t *scratch, K2aLLRes *res, void *)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	for (int t = 0; t < ntasks; ++t) {
		if (pk && lds) ll_task<true, true>(*par, tasks[t], seq, tab, scratch, res);
		else if (pk) ll_task<true, false>(*par, tasks[t], seq, tab, scratch, res);
		else if (lds) ll_task<false, true>(*par, tasks[t], seq, tab, scratch, res);
		else ll_task<false, false>(*par, tasks[t], seq, tab, scratch, res);
	}
	return 0;
}
