/*
 * ksw2_lane_llsub.h -- per-lane code of k2a_ll_sub_kernel, the reduction behind the forward pass of ksw2amd_ll_sub_batch (DESIGN.md
 * section 3.17), shared by the gfx950 kernel (ksw2_shim_hip.hip) and the lock-step simulator of the tests (tests/llsim).
 *
 * Input: a task's row profile as K2aLaneLL<.., SUB>::sub_store left it -- 8 bytes per row, in blocks of 128 bytes per K2A_LL_C rows (one
 * lane's strip): the 16 row maxima R(t), then the 16 first columns that reached them; a packed task keeps its two alignments in the
 * 16-bit halves of both words.  Rows are the target.
 * Output per alignment: the largest R(t) over the rows with |t - te| > d, then the smallest such t (te2), and that row's column (qe2).
 * The plain maximum over rows: runs of adjacent rows are not merged into peaks.
 */
#ifndef KSW2_LANE_LLSUB_H_
#define KSW2_LANE_LLSUB_H_

#include "ksw2_lane.h"

struct K2aLLSubKey { int s, t; };      /* larger row maximum, then smaller row */
K2A_FN bool k2a_llsub_better(int s, int t, const K2aLLSubKey &k) { return s > k.s || (s == k.s && s > 0 && t < k.t); }

/* rows excluded on either side of te: excl when >= 0, else ceil(score / smax) (an alignment of that score spans at least as many rows) */
K2A_FN int k2a_llsub_window(int excl, int score, int smax) { return excl >= 0 ? excl : (int)(((uint32_t)score + (uint32_t)smax - 1u) / (uint32_t)smax); }

/* word index of row t's maximum in the profile (its column: K2A_LL_C words further); half h's value of a profile word */
K2A_FN int64_t k2a_llsub_word(int64_t t) { return (t / K2A_LL_C) * (2 * K2A_LL_C) + t % K2A_LL_C; }
K2A_FN int k2a_llsub_half(uint32_t w, bool pk, int h) { return (int)(pk ? (w >> (16 * h)) & 0xffffu : w); }

/* lane's share of the rows: t = lane, lane + 64, ... < nrows outside the window (rows ascending: strict > keeps the smallest t) */
K2A_FN void k2a_llsub_lane(const uint32_t *prof, bool pk, int h, int nrows, int te, int d, int lane, K2aLLSubKey &k)
{
	k.s = 0; k.t = -1;
	for (int64_t t = lane; t < nrows; t += 64) {
		const int64_t dt = t - te;
		if (dt <= d && dt >= -(int64_t)d) continue;
		const int s = k2a_llsub_half(prof[k2a_llsub_word(t)], pk, h);
		if (s > k.s) { k.s = s; k.t = (int)t; }
	}
}

/* the result from the reduced key (one lane): the column of row te2 */
K2A_FN void k2a_llsub_finish(const uint32_t *prof, bool pk, int h, const K2aLLSubKey &k, K2aLLSub &out)
{
	out.score2 = k.s > 0 ? k.s : 0;
	out.te2 = k.s > 0 ? k.t : -1;
	out.qe2 = k.s > 0 ? k2a_llsub_half(prof[k2a_llsub_word(k.t) + K2A_LL_C], pk, h) : -1;
}

#endif
