// TEST INFRASTRUCTURE: k2a_shim_launch_ov and k2a_shim_launch_ovd (ksw2_shim.h) on the host -- the overlap forms of the local-alignment lane
// code (ksw2_lane_ll.h, FIT with OV, without and with DUAL) for 64 lanes in lock step with the kernels' schedule (k2a_ov_kernel,
// k2a_ovd_kernel): the twins of tests/llsim/sg_shim_sim.cpp and sgd_shim_sim.cpp with the task's free query ends taken from its pad -- row -1
// from fit_top as the ends say, the last row's running maximum inside step() and gen_end().  The two-piece form keeps 16 bytes of boundary per
// column.  A packed task with the query's end free must have a 16-bit column index.  Launches that had tasks are counted.  Linked by
// tests/ov_util.py next to the semi-global twins.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"

static long g_ov_launches, g_ovd_launches;

template<bool PK, bool LDSP, bool DUAL>
static void ov_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, K2aLLRes *res)
{
	static K2aLaneLL<PK, LDSP, false, false, DUAL, true, true> L[64];
	const int W = DUAL ? 4 : 2;                            // boundary words per column
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);
	const int ncols = tk.ncols, ngen = (tk.nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	for (int l = 0; l < 64; ++l) L[l].init(par, tk, l);
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
				const uint32_t qc = PK ? (uint32_t)c0[jj] | ((uint32_t)c1[jj] << 8) : (uint32_t)c0[jj];
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
	for (int h = 0; h < (PK ? 2 : 1); ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) { res[tk.res[h]].score = k.s - L[0].fit_bias(); res[tk.res[h]].qe = k.qe; res[tk.res[h]].te = k.te; }
	}
}

extern "C" long ov_sim_launches(void) { return g_ov_launches; }
extern "C" long ovd_sim_launches(void) { return g_ovd_launches; }
extern "C" void ov_sim_reset_launches(void) { g_ov_launches = g_ovd_launches = 0; }

template<bool DUAL>
static int ov_launch(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch,
                     K2aLLRes *res)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	++(DUAL ? g_ovd_launches : g_ov_launches);
	for (int t = 0; t < ntasks; ++t) {
		if (tasks[t].swapped) return -1;                   // rows are always the target
		if (tasks[t].pad & ~3) return -1;                  // the free ends: two bits
		if (pk && (tasks[t].pad & 2) && tasks[t].ncols > 65536) return -1;      // the packed last-row maximum keeps a 16-bit column
		if (DUAL && tasks[t].nrows > K2A_LL_ROWS && (tasks[t].boff & 15)) return -1;      // the kernel moves a boundary entry as one 16-byte access
		if (pk && lds) ov_task<true, true, DUAL>(*par, tasks[t], seq, tab, scratch, res);
		else if (pk) ov_task<true, false, DUAL>(*par, tasks[t], seq, tab, scratch, res);
		else if (lds) ov_task<false, true, DUAL>(*par, tasks[t], seq, tab, scratch, res);
		else ov_task<false, false, DUAL>(*par, tasks[t], seq, tab, scratch, res);
	}
	return 0;
}

extern "C" int k2a_shim_launch_ov(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                  uint8_t *scratch, K2aLLRes *res, void *)
{
	return ov_launch<false>(pk, lds, par, tasks, ntasks, seq, tab, scratch, res);
}

extern "C" int k2a_shim_launch_ovd(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                                   uint8_t *scratch, K2aLLRes *res, void *)
{
	return ov_launch<true>(pk, lds, par, tasks, ntasks, seq, tab, scratch, res);
}
