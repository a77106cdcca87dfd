// TEST INFRASTRUCTURE: k2a_shim_launch_lld_sub (ksw2_shim.h) on the host (tests/llds_util.py) -- the lane code of ksw2amd_lld_sub_batch in
// lock step with the kernels' schedules:
//  * the forward pass: K2aLaneLL<PK, LDSP, false, SUB = true, DUAL = true> (ksw2_lane_ll.h) for 64 lanes as k2a_lld_fsub_kernel runs them:
//    H, E and E2 of the bottom row rotate to the lane below, lane 63 -> 16-byte boundary entry -> lane 0 across generations, and
//    sub_store() next to gen_end() writes the row profile at prof + 128 * tk.pad;
//  * the reduction of k2a_ll_sub_kernel (ksw2_lane_llsub.h), unchanged: one wavefront per result slot, 64 lanes striding over the rows,
//    the xor butterfly, lane 0's write.
// The launch rule is the product's: packed tasks take the LDS profile unless K2A_LLD_PK_REG.  Launches that had tasks are counted.
// Linked by tests/llds_util.py next to the other twins and the product's host objects.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"
#include "../../ksw2_amd/csrc/ksw2_lane_llsub.h"

static long g_llds_launches;

template<bool PK, bool LDSP>
static void llds_task(const K2aLL &par, const K2aLLTask &tk, const uint8_t *seq, const uint8_t *tab, uint8_t *scratch, K2aLLRes *res, uint8_t *prof)
{
	static K2aLaneLL<PK, LDSP, false, true, true> L[64];
	const int mm = par.m * par.m;
	const uint8_t *ltab = tab + (tk.swapped ? mm : 0);
	const uint8_t *r0 = seq + tk.roff[0], *r1 = seq + tk.roff[PK ? 1 : 0], *c0 = seq + tk.coff[0], *c1 = seq + tk.coff[PK ? 1 : 0];
	uint32_t *bnd = (uint32_t*)(scratch + tk.boff);          // four words per column: H, E, E2, pad
	const int ncols = tk.ncols, ngen = (tk.nrows + K2A_LL_ROWS - 1) / K2A_LL_ROWS, nsteps = ncols + 63;
	for (int l = 0; l < 64; ++l) L[l].init(par, tk, l);
	for (int g = 0; g < ngen; ++g) {
		const bool from_bnd = g > 0, to_bnd = g + 1 < ngen;
		uint32_t hin[64] = { 0 }, ein[64] = { 0 }, e2in[64] = { 0 }, ho[64], eo[64], e2o[64];
		for (int l = 0; l < 64; ++l) L[l].gen_begin(g, r0, r1, ltab);
		for (int k = 0; k < nsteps; ++k) {
			for (int l = 0; l < 64; ++l) {
				const int jj = k - l;
				ho[l] = eo[l] = e2o[l] = 0;
				if (jj < 0 || jj >= ncols) continue;
				uint32_t h = hin[l], e = ein[l], e2 = e2in[l];
				if (l == 0) { h = from_bnd ? bnd[4 * jj] : 0u; e = from_bnd ? bnd[4 * jj + 1] : 0u; e2 = from_bnd ? bnd[4 * jj + 2] : 0u; }
				const uint32_t qc = PK ? (uint32_t)c0[jj] | ((uint32_t)c1[jj] << 8) : (uint32_t)c0[jj];
				L[l].step(jj, h, e, e2, qc, ltab, ho[l], eo[l], e2o[l]);
				if (to_bnd && l == 63) { bnd[4 * jj] = ho[l]; bnd[4 * jj + 1] = eo[l]; bnd[4 * jj + 2] = e2o[l]; bnd[4 * jj + 3] = 0; }
			}
			for (int l = 0; l < 64; ++l) { hin[l] = ho[(l + 63) & 63]; ein[l] = eo[(l + 63) & 63]; e2in[l] = e2o[(l + 63) & 63]; }   // wave_ror:1
		}
		for (int l = 0; l < 64; ++l) { L[l].gen_end(); L[l].sub_store(prof + (size_t)tk.pad * 128); }
	}
	for (int h = 0; h < (PK ? 2 : 1); ++h) {
		K2aLLKey k = L[0].key[h];
		for (int l = 1; l < 64; ++l) if (k2a_ll_better(L[l].key[h].s, L[l].key[h].te, L[l].key[h].qe, k)) k = L[l].key[h];
		if (h == 0 || tk.res[1] != tk.res[0]) { res[tk.res[h]].score = k.s; res[tk.res[h]].qe = k.qe; res[tk.res[h]].te = k.te; }
	}
}

static void llds_reduce(int smax, const K2aLLTask &tk, int pk, int h, const K2aLLRes *res, const uint8_t *prof, int excl, K2aLLSub *sub)
{
	if (h == 1 && tk.res[1] == tk.res[0]) return;
	const K2aLLRes r = res[tk.res[h]];
	const uint32_t *p = (const uint32_t*)(prof + (size_t)tk.pad * 128);
	K2aLLSubKey k[64];
	for (int lane = 0; lane < 64; ++lane) k2a_llsub_lane(p, pk != 0, h, tk.nrows, r.te, k2a_llsub_window(excl, r.score, smax), lane, k[lane]);
	for (int d = 1; d < 64; d <<= 1) {                         // the xor butterfly: every lane takes its partner's key when it is better
		K2aLLSubKey o[64];
		for (int lane = 0; lane < 64; ++lane) o[lane] = k[lane ^ d];
		for (int lane = 0; lane < 64; ++lane) if (k2a_llsub_better(o[lane].s, o[lane].t, k[lane])) k[lane] = o[lane];
	}
	k2a_llsub_finish(p, pk != 0, h, k[0], sub[tk.res[h]]);
}

extern "C" {

long llds_sim_launches(void) { return g_llds_launches; }
void llds_sim_reset_launches(void) { g_llds_launches = 0; }

int k2a_shim_launch_lld_sub(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                            uint8_t *scratch, K2aLLRes *res, uint8_t *prof, int excl, K2aLLSub *sub, void *)
{
	if (ntasks <= 0) return 0;
	if (par->m < 1 || par->m > K2A_MAXM || (!lds && par->m > 5)) return -1;
	++g_llds_launches;
	for (int t = 0; t < ntasks; ++t) {
		if (tasks[t].swapped) return -1;                       // rows must be the target
		if (tasks[t].nrows > K2A_LL_ROWS && (tasks[t].boff & 15)) return -1;      // the 16-byte boundary entries
		if (pk && (lds || !K2A_LLD_PK_REG)) llds_task<true, true>(*par, tasks[t], seq, tab, scratch, res, prof);
		else if (pk) llds_task<true, false>(*par, tasks[t], seq, tab, scratch, res, prof);
		else if (lds) llds_task<false, true>(*par, tasks[t], seq, tab, scratch, res, prof);
		else llds_task<false, false>(*par, tasks[t], seq, tab, scratch, res, prof);
	}
	for (int t = 0; t < ntasks; ++t)                           // behind the forward launch: one wavefront per result slot
		for (int h = 0; h < (pk ? 2 : 1); ++h) llds_reduce(par->smax, tasks[t], pk, h, res, prof, excl, sub);
	return 0;
}

}
