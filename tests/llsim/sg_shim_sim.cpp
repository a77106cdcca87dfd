// TEST INFRASTRUCTURE: k2a_shim_launch_sg (ksw2_shim.h) on the host -- the semi-global form of the local-alignment lane code
// (ksw2_lane_ll.h, FIT) for 64 lanes in lock step, with the kernel's schedule: DPP rotate of the bottom row, lane 63 -> boundary -> lane 0
// across generations, row -1 from fit_top for lane 0 of the first generation, one key reduction per task, the bias taken off the score.
// Launches that had tasks are counted.  Linked by tests/sg_util.py next to tests/llsim/llf_shim_sim.cpp.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

static long g_sg_launches;

template<bool PK, bool LDSP>
static void sg_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, K2aLLRes *res)
{
	static K2aLaneLL<PK, LDSP, false, false, false, true> L[64];
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	const int ncols = tk.ncols, ngen = (tk.nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	for (int l = 0; l < 64; ++l) L[l].init(par, tk, l);
	for (int g = 0; g < ngen; ++g) {
		const bool from_bnd = g > 0, to_bnd = g + 1 < ngen;
		uint32_t hin[64] = { 0 }, ein[64] = { 0 }, ho[64], eo[64];
		for (int l = 0; l < 64; ++l) L[l].gen_begin(g, r0, r1, tab);
		for (int k = 0; k < nsteps; ++k) {
			for (int l = 0; l < 64; ++l) {
				const int jj = k - l;
				ho[l] = eo[l] = 0;
				if (jj < 0 || jj >= ncols) continue;
				uint32_t h = hin[l], e = ein[l];
				if (l == 0) {
					if (from_bnd) { h = bnd[2 * jj]; e = bnd[2 * jj + 1]; }
					else L[0].fit_top(jj, h, e);
				}
				const uint32_t qc = PK ? (uint32_t)c0[jj] | ((uint32_t)c1[jj] << 8) : (uint32_t)c0[jj];
				L[l].step(jj, h, e, qc, tab, ho[l], eo[l]);
				if (to_bnd && l == 63) { bnd[2 * jj] = ho[l]; bnd[2 * jj + 1] = eo[l]; }
			}
			for (int l = 0; l < 64; ++l) { hin[l] = ho[(l + 63) & 63]; ein[l] = eo[(l + 63) & 63]; }   // wave_ror:1
		}
		for (int l = 0; l < 64; ++l) L[l].gen_end();
	}
	for (int h = 0; h < (PK ? 2 : 1); ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) { res[tk.res[h]].score = k.s - L[0].fit_bias(); res[tk.res[h]].qe = k.qe; res[tk.res[h]].te = k.te; }
	}
}

extern "C" long sg_sim_launches(void) { return g_sg_launches; }
extern "C" void sg_sim_reset_launches(void) { g_sg_launches = 0; }

extern "C" int k2a_shim_launch_sg(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                  uint8_t *scratch, K2aLLRes *res, void *)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	++g_sg_launches;
	for (int t = 0; t < ntasks; ++t) {
		if (tasks[t].swapped) return -1;                   // rows are always the target
		if (pk && lds) sg_task<true, true>(*par, tasks[t], seq, tab, scratch, res);
		else if (pk) sg_task<true, false>(*par, tasks[t], seq, tab, scratch, res);
		else if (lds) sg_task<false, true>(*par, tasks[t], seq, tab, scratch, res);
		else sg_task<false, false>(*par, tasks[t], seq, tab, scratch, res);
	}
	return 0;
}
