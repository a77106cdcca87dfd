// TEST INFRASTRUCTURE: k2a_shim_launch_ov_rev and k2a_shim_launch_ovd_rev (ksw2_shim.h) on the host -- the start pass of ksw2amd_ov_align_batch /
// ksw2amd_ovd_align_batch: the FIT x OV x REV forms of the local-alignment lane code (ksw2_lane_ll.h, without and with DUAL) for 64 lanes in
// lock step with the kernels' schedule (k2a_ov_rev_kernel, k2a_ovd_rev_kernel): rows and columns read from the forward results and clamped
// into the task (rl = te + 1, cl = qe + 1 per half), the bounding rectangle of the two halves, reversed indexing with clamped loads, row -1
// from fit_top for lane 0 of the first generation, DPP rotate of the bottom row, lane 63 -> boundary -> lane 0 across generations (16 bytes per
// column in the two-piece form), one key reduction per task, the bias taken off the score, qb and tb from the key's column and row.  Launches
// that had tasks are counted.  Linked by tests/ova_util.py next to tests/llsim/ov_shim_sim.cpp and the semi-global twins.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

static long g_ova_launches, g_ovda_launches;

template<bool PK, bool LDSP, bool DUAL>
static void ova_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, const K2aLLRes *fres, K2aLLBeg *beg)
{
	static K2aLaneLL<PK, LDSP, true, false, DUAL, true, true> L[64];
	const int NH = PK ? 2 : 1, W = DUAL ? 4 : 2;            // boundary words per column
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	int rl[2] = { 0, 0 }, cl[2] = { 0, 0 }, ft[2] = { 0, 0 }, fq[2] = { 0, 0 };
	for (int h = 0; h < NH; ++h) {
		const K2aLLRes r = fres[tk.res[h]];
		ft[h] = r.te; fq[h] = r.qe;
		rl[h] = k2a_min(k2a_max(r.te + 1, 0), tk.nrows); cl[h] = k2a_min(k2a_max(r.qe + 1, 1), tk.ncols);
	}
	for (int l = 0; l < 64; ++l) { L[l].init(par, tk, l); L[l].set_limits(rl, cl); }
	const int ncols = L[0].ncols, ngen = (L[0].nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	const int cl0 = cl[0], cl1 = cl[PK ? 1 : 0];
	for (int g = 0; g < ngen; ++g) {
		const bool from_bnd = g > 0, to_bnd = g + 1 < ngen;
		uint32_t hin[64] = { 0 }, ein[64] = { 0 }, e2in[64] = { 0 }, ho[64], eo[64], e2o[64];
		for (int l = 0; l < 64; ++l) L[l].gen_begin(g, r0, r1, tab);
		for (int k = 0; k < nsteps; ++k) {
			for (int l = 0; l < 64; ++l) {
				const int jj = k - l;
				ho[l] = eo[l] = e2o[l] = 0;
				if (jj < 0 || jj >= ncols) continue;
				uint32_t h = hin[l], e = ein[l], e2 = e2in[l];
				if (l == 0) {
					if (from_bnd) { h = bnd[W * jj]; e = bnd[W * jj + 1]; if (DUAL) e2 = bnd[W * jj + 2]; }
					else if (DUAL) L[0].fit_top(jj, h, e, e2);
					else L[0].fit_top(jj, h, e);
				}
				const int j0 = k2a_max(cl0 - 1 - jj, 0), j1 = k2a_max(cl1 - 1 - jj, 0);
				const uint32_t qc = PK ? (uint32_t)c0[j0] | ((uint32_t)c1[j1] << 8) : (uint32_t)c0[j0];
				if (DUAL) L[l].step(jj, h, e, e2, qc, tab, ho[l], eo[l], e2o[l]);
				else L[l].step(jj, h, e, qc, tab, ho[l], eo[l]);
				if (to_bnd && l == 63) {
					bnd[W * jj] = ho[l]; bnd[W * jj + 1] = eo[l];
					if (DUAL) { bnd[W * jj + 2] = e2o[l]; bnd[W * jj + 3] = 0; }
				}
			}
			for (int l = 0; l < 64; ++l) { hin[l] = ho[(l + 63) & 63]; ein[l] = eo[(l + 63) & 63]; e2in[l] = e2o[(l + 63) & 63]; }   // wave_ror:1
		}
		for (int l = 0; l < 64; ++l) L[l].gen_end();
	}
	for (int h = 0; h < NH; ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) {
			K2aLLBeg b;
			b.score = k.s - L[0].fit_bias(); b.qb = fq[h] - k.qe; b.tb = ft[h] - k.te;
			beg[tk.res[h]] = b;
		}
	}
}

extern "C" long ova_sim_launches(void) { return g_ova_launches; }
extern "C" long ovda_sim_launches(void) { return g_ovda_launches; }
extern "C" void ova_sim_reset_launches(void) { g_ova_launches = g_ovda_launches = 0; }

template<bool DUAL>
static int ova_launch(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch,
                      const K2aLLRes *res, K2aLLBeg *beg)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	++(DUAL ? g_ovda_launches : g_ova_launches);
	for (int t = 0; t < ntasks; ++t) {
		if (tasks[t].swapped) return -1;                   // rows are always the target
		if (tasks[t].pad & ~3) return -1;                  // the free ends: two bits
		if (pk && (tasks[t].pad & 1) && tasks[t].ncols > 65536) return -1;      // the packed last-row maximum keeps a 16-bit column
		if (DUAL && tasks[t].nrows > K2A_LL_ROWS && (tasks[t].boff & 15)) return -1;      // the kernel moves a boundary entry as one 16-byte access
		if (pk && lds) ova_task<true, true, DUAL>(*par, tasks[t], seq, tab, scratch, res, beg);
		else if (pk) ova_task<true, false, DUAL>(*par, tasks[t], seq, tab, scratch, res, beg);
		else if (lds) ova_task<false, true, DUAL>(*par, tasks[t], seq, tab, scratch, res, beg);
		else ova_task<false, false, DUAL>(*par, tasks[t], seq, tab, scratch, res, beg);
	}
	return 0;
}

extern "C" int k2a_shim_launch_ov_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                      uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *)
{
	return ova_launch<false>(pk, lds, par, tasks, ntasks, seq, tab, scratch, res, beg);
}

extern "C" int k2a_shim_launch_ovd_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                       uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *)
{
	return ova_launch<true>(pk, lds, par, tasks, ntasks, seq, tab, scratch, res, beg);
}
