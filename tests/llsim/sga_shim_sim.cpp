// TEST INFRASTRUCTURE: k2a_shim_launch_sg_rev (ksw2_shim.h) on the host -- the start pass of ksw2amd_sg_align_batch: the FIT x REV form of
// the local-alignment lane code (ksw2_lane_ll.h) for 64 lanes in lock step with the kernel's schedule (k2a_sg_rev_kernel): the rows read
// from the forward results whatever the sign of the score and clamped into the task, the whole reversed query as columns, the bounding
// rectangle of the two halves, reversed indexing with clamped loads, row -1 from fit_top for lane 0 of the first generation, DPP rotate of
// the bottom row, lane 63 -> boundary -> lane 0 across generations, one key reduction per task, the bias taken off the score.  Launches
// that had tasks are counted.  Linked by tests/sga_util.py next to tests/llsim/llf_shim_sim.cpp and sg_shim_sim.cpp.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

static long g_sga_launches;

template<bool PK, bool LDSP>
static void sga_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, const K2aLLRes *fres, K2aLLBeg *beg)
{
	static K2aLaneLL<PK, LDSP, true, false, false, true> L[64];
	const int NH = PK ? 2 : 1;
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	int rl[2] = { 0, 0 }, cl[2] = { 0, 0 }, ft[2] = { 0, 0 };
	for (int h = 0; h < NH; ++h) {
		const K2aLLRes r = fres[tk.res[h]];
		ft[h] = r.te;
		rl[h] = k2a_min(k2a_max(r.te + 1, 0), tk.nrows); cl[h] = tk.ncols;
	}
	for (int l = 0; l < 64; ++l) { L[l].init(par, tk, l); L[l].set_limits(rl, cl); }
	const int ncols = L[0].ncols, ngen = (L[0].nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	const int cl0 = cl[0], cl1 = cl[PK ? 1 : 0];
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
				const int j0 = k2a_max(cl0 - 1 - jj, 0), j1 = k2a_max(cl1 - 1 - jj, 0);
				const uint32_t qc = PK ? (uint32_t)c0[j0] | ((uint32_t)c1[j1] << 8) : (uint32_t)c0[j0];
				L[l].step(jj, h, e, qc, tab, ho[l], eo[l]);
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
			b.score = k.s - L[0].fit_bias(); b.qb = 0; b.tb = ft[h] - k.te;
			beg[tk.res[h]] = b;
		}
	}
}

extern "C" long sga_sim_launches(void) { return g_sga_launches; }
extern "C" void sga_sim_reset_launches(void) { g_sga_launches = 0; }

extern "C" int k2a_shim_launch_sg_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                      uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	++g_sga_launches;
	for (int t = 0; t < ntasks; ++t) {
		if (tasks[t].swapped) return -1;                   // rows are always the target
		if (pk && lds) sga_task<true, true>(*par, tasks[t], seq, tab, scratch, res, beg);
		else if (pk) sga_task<true, false>(*par, tasks[t], seq, tab, scratch, res, beg);
		else if (lds) sga_task<false, true>(*par, tasks[t], seq, tab, scratch, res, beg);
		else sga_task<false, false>(*par, tasks[t], seq, tab, scratch, res, beg);
	}
	return 0;
}
