// TEST INFRASTRUCTURE: the device side of the flat local-alignment batches on the host (tests/llf_util.py).
//  * k2a_shim_launch_ll_check: the lane code of k2a_ll_check_kernel (ksw2_lane_llchk.h) for 64 lanes per wavefront in the kernel's
//    schedule -- K2A_LLCHK_WAVE blocks per wavefront, the entries of its first and last block found once, the lanes' lowest pair
//    reduced and one minimum into *bad per wavefront that saw a bad code.
//  * k2a_shim_launch_ll / k2a_shim_launch_ll_rev: the twins of tests/llsim/ll_shim_sim.cpp and lla_shim_sim.cpp, compiled in here under
//    other names behind wrappers that COUNT the launches: a test can show that no alignment kernel ran on a chunk with a bad code.
// Linked next to tests/sim/ksw2_shim_sim.cpp and the product's host objects instead of those two files.  Never shipped.
#include <string.h>
#include "../../ksw2_amd/csrc/ksw2_shim.h"
#include "../../ksw2_amd/csrc/ksw2_lane_ll.h"
#include "../../ksw2_amd/csrc/ksw2_lane_llchk.h"

#define k2a_shim_launch_ll llf_inner_launch_ll
#include "ll_shim_sim.cpp"
#undef k2a_shim_launch_ll
#define k2a_shim_launch_ll_rev llf_inner_launch_ll_rev
#include "lla_shim_sim.cpp"
#undef k2a_shim_launch_ll_rev

static long g_align_launches, g_check_launches, g_check_blocks;

extern "C" {

// launches that had tasks (the product's launchers return before the launch when ntasks == 0)
long llf_sim_align_launches(void) { return g_align_launches; }
long llf_sim_check_launches(void) { return g_check_launches; }
long llf_sim_check_blocks(void) { return g_check_blocks; }      // 16-byte blocks the check looked at since the last reset
void llf_sim_reset_counters(void) { g_align_launches = g_check_launches = g_check_blocks = 0; }

int k2a_shim_launch_ll(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                       uint8_t *scratch, K2aLLRes *res, void *stream)
{
	if (ntasks > 0) ++g_align_launches;
	return llf_inner_launch_ll(pk, lds, par, tasks, ntasks, seq, tab, scratch, res, stream);
}

int k2a_shim_launch_ll_rev(int pk, int lds, const K2aLL *par, const K2aLLTask *tasks, int ntasks, const uint8_t *seq, const uint8_t *tab,
                           uint8_t *scratch, const K2aLLRes *res, K2aLLBeg *beg, void *stream)
{
	if (ntasks > 0) ++g_align_launches;
	return llf_inner_launch_ll_rev(pk, lds, par, tasks, ntasks, seq, tab, scratch, res, beg, stream);
}

int k2a_shim_launch_ll_check(const K2aLLChk *ent, int nent, uint32_t nblocks, const uint8_t *seq, int m, uint32_t *bad, void *)
{
	if (nent <= 0 || nblocks == 0) return 0;
	if (m < 1 || m > K2A_MAXM) return -1;
	++g_check_launches;
	g_check_blocks += nblocks;
	const uint32_t waves = (nblocks + K2A_LLCHK_WAVE - 1) / K2A_LLCHK_WAVE;
	for (uint32_t wave = 0; wave < waves; ++wave) {
		const uint32_t c0 = wave * K2A_LLCHK_WAVE, c1 = (nblocks - c0 > K2A_LLCHK_WAVE ? c0 + K2A_LLCHK_WAVE : nblocks) - 1;
		const int elo = k2a_llchk_find(ent, 0, nent - 1, c0), ehi = k2a_llchk_find(ent, elo, nent - 1, c1);
		uint32_t best[64];
		bool any = false;
		for (int lane = 0; lane < 64; ++lane) {
			best[lane] = k2a_llchk_lane(ent, elo, ehi, c0, c1, lane, seq, (uint32_t)m);
			any = any || best[lane] != K2A_LLCHK_NONE;
		}
		if (!any) continue;                                    // the ballot
		for (int d = 1; d < 64; d <<= 1)                       // the xor butterfly
			for (int lane = 0; lane < 64; ++lane) { const uint32_t o = best[lane ^ d]; if (lane < (lane ^ d)) { const uint32_t mn = o < best[lane] ? o : best[lane]; best[lane] = best[lane ^ d] = mn; } }
		if (best[0] < *bad) *bad = best[0];                    // the atomic min
	}
	return 0;
}

}
