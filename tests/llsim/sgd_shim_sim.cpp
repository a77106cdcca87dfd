// TEST INFRASTRUCTURE: k2a_shim_launch_sgd and k2a_shim_launch_sgd_rev (ksw2_shim.h) on the host -- the FIT x DUAL forms of the
// local-alignment lane code (ksw2_lane_ll.h), without and with REV, for 64 lanes in lock step with the kernels' schedule (k2a_sgd_kernel,
// k2a_sgd_rev_kernel): the twins of tests/llsim/sg_shim_sim.cpp and sga_shim_sim.cpp plus the second piece -- E2 rotates with H and E, the
// boundary between generations holds 16 bytes per column (H, E, E2, pad), and lane 0 of the first generation takes H', E' and E2' of row -1 from
// fit_top.  Launches that had tasks are counted.  Linked by tests/sgd_util.py next to llf_shim_sim.cpp, sg_shim_sim.cpp and sga_shim_sim.cpp.
// Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

static long g_sgd_launches, g_sgd_rev_launches;

template<bool PK, bool LDSP, bool REV>
static void sgd_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, K2aLLRes *res, const K2aLLRes *fres,
                     K2aLLBeg *beg)
{
	static K2aLaneLL<PK, LDSP, REV, false, true, true> L[64];
	const int NH = PK ? 2 : 1;
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	int rl[2] = { 0, 0 }, cl[2] = { 0, 0 }, ft[2] = { 0, 0 };
	for (int l = 0; l < 64; ++l) L[l].init(par, tk, l);
	if (REV) {
		for (int h = 0; h < NH; ++h) {
			const K2aLLRes r = fres[tk.res[h]];
			ft[h] = r.te;
			rl[h] = k2a_min(k2a_max(r.te + 1, 0), tk.nrows); cl[h] = tk.ncols;
		}
		for (int l = 0; l < 64; ++l) L[l].set_limits(rl, cl);
	}
	const int ncols = REV ? L[0].ncols : tk.ncols, ngen = ((REV ? L[0].nrows : tk.nrows) + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
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
					if (from_bnd) { h = bnd[4 * jj]; e = bnd[4 * jj + 1]; e2 = bnd[4 * jj + 2]; }
					else L[0].fit_top(jj, h, e, e2);
				}
				uint32_t qc;
				if (REV) {
					const int j0 = k2a_max(cl0 - 1 - jj, 0), j1 = k2a_max(cl1 - 1 - jj, 0);
					qc = PK ? (uint32_t)c0[j0] | ((uint32_t)c1[j1] << 8) : (uint32_t)c0[j0];
				} else qc = PK ? (uint32_t)c0[jj] | ((uint32_t)c1[jj] << 8) : (uint32_t)c0[jj];
				L[l].step(jj, h, e, e2, qc, tab, ho[l], eo[l], e2o[l]);
				if (to_bnd && l == 63) { bnd[4 * jj] = ho[l]; bnd[4 * jj + 1] = eo[l]; bnd[4 * jj + 2] = e2o[l]; bnd[4 * jj + 3] = 0; }
			}
			for (int l = 0; l < 64; ++l) { hin[l] = ho[(l + 63) & 63]; ein[l] = eo[(l + 63) & 63]; e2in[l] = e2o[(l + 63) & 63]; }   // wave_ror:1
		}
		for (int l = 0; l < 64; ++l) L[l].gen_end();
	}
	for (int h = 0; h < NH; ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) {
			if (REV) {
				K2aLLBeg b;
				b.score = k.s - L[0].fit_bias(); b.qb = 0; b.tb = ft[h] - k.te;
				beg[tk.res[h]] = b;
			} else { res[tk.res[h]].score = k.s - L[0].fit_bias(); res[tk.res[h]].qe = k.qe; res[tk.res[h]].te = k.te; }
		}
	}
}

extern "C" long sgd_sim_launches(void) { return g_sgd_launches; }
extern "C" long sgd_sim_rev_launches(void) { return g_sgd_rev_launches; }
extern "C" void sgd_sim_reset_launches(void) { g_sgd_launches = g_sgd_rev_launches = 0; }

template<bool REV>
static int sgd_launch(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch,
                      K2aLLRes *res, const K2aLLRes *fres, K2aLLBeg *beg)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	++(REV ? g_sgd_rev_launches : g_sgd_launches);
	for (int t = 0; t < ntasks; ++t) {
		if (tasks[t].swapped) return -1;                   // rows are always the target
		if (tasks[t].nrows > K2A_LL_ROWS && (tasks[t].boff & 15)) return -1;      // the kernel moves a boundary entry as one 16-byte access
		if (pk && (lds || !K2A_SGD_PK_REG)) sgd_task<true, true, REV>(*par, tasks[t], seq, tab, scratch, res, fres, beg);
		else if (pk) sgd_task<true, false, REV>(*par, tasks[t], seq, tab, scratch, res, fres, beg);
		else if (lds) sgd_task<false, true, REV>(*par, tasks[t], seq, tab, scratch, res, fres, beg);
		else sgd_task<false, false, REV>(*par, tasks[t], seq, tab, scratch, res, fres, beg);
	}
	return 0;
}

extern "C" int k2a_shim_launch_sgd(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                   uint8_t *scratch, K2aLLRes *res, void *)
{
	return sgd_launch<false>(pk, lds, par, tasks, ntasks, seq, tab, scratch, res, 0, 0);
}

extern "C" int k2a_shim_launch_sgd_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                       uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *)
{
	return sgd_launch<true>(pk, lds, par, tasks, ntasks, seq, tab, scratch, 0, res, beg);
}
