/*
 * ksw2_lane_llchk.h -- per-lane code of the residue-code check of the flat local-alignment batches (ksw2amd_ll_batch_flat /
 * ksw2amd_ll_align_batch_flat), shared by the gfx950 kernel k2a_ll_check_kernel (ksw2_shim_hip.hip) and the
 * lock-step simulator of the tests (tests/llsim/llf_shim_sim.cpp).
 *
 * The flat entries borrow the caller's arena, so no host loop sees the bytes; the local-alignment kernels index their pen table with
 * them, so a code >= m must be found before any of them is launched.  The host lists every distinct sequence of a chunk once
 * (K2aLLChk, ksw2_types.h) and numbers the 16-byte blocks they cover, blocks cut at 16-byte aligned ADDRESSES: a wavefront takes
 * K2A_LLCHK_WAVE consecutive blocks whatever entries they belong to (work is spread by bytes, not by sequences), a lane one block at a
 * time.  A block that lies inside its sequence is one 16-byte load and four word tests; the head and tail blocks of a sequence are read
 * byte by byte, only the bytes that belong to it -- nothing outside a referenced sequence is ever read.
 *
 * Four codes at once: m <= 127, so for a word x "some byte >= m" is
 *   (((x & 0x7f7f7f7f) + (128 - m) * 0x01010101) | x) & 0x80808080
 * (low seven bits + (128 - m) carries into bit 7 exactly when they are >= m, never into the next byte: at most 127 + 127; or-ing x
 * itself catches the bytes >= 128).
 */
#ifndef KSW2_LANE_LLCHK_H_
#define KSW2_LANE_LLCHK_H_

#include "ksw2_lane.h"

struct K2aChkWord4 { uint32_t x, y, z, w; };      /* one aligned 16-byte load */

K2A_FN uint32_t k2a_llchk_word(uint32_t x, uint32_t m)
{
	return (((x & 0x7f7f7f7fu) + (128u - m) * 0x01010101u) | x) & 0x80808080u;
}

/* the entry of block c: the last e in [lo, hi] with ent[e].first <= c (ent[lo].first <= c is given) */
K2A_FN int k2a_llchk_find(const K2aLLChk *ent, int lo, int hi, uint32_t c)
{
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (ent[mid].first <= c) lo = mid; else hi = mid - 1;
	}
	return lo;
}

/* block k of entry e: true when one of its bytes that belong to the sequence is >= m */
K2A_FN bool k2a_llchk_block(const uint8_t *seq, const K2aLLChk &e, uint32_t k, uint32_t m)
{
	const uint8_t *p = seq + e.off, *end = p + e.len;
	const uint8_t *a = p - ((uintptr_t)p & 15u) + (size_t)k * 16u;      /* 16-byte aligned; the first block starts at or before p */
	if (a >= p && a + 16 <= end) {
		const K2aChkWord4 v = *(const K2aChkWord4*)a;
		return (k2a_llchk_word(v.x, m) | k2a_llchk_word(v.y, m) | k2a_llchk_word(v.z, m) | k2a_llchk_word(v.w, m)) != 0;
	}
	bool bad = false;
	for (int b = 0; b < 16; ++b) {
		const uint8_t *q = a + b;
		if (q >= p && q < end && *q >= m) bad = true;
	}
	return bad;
}

/* a wavefront's share: blocks [c0, c1] of the chunk; [elo, ehi] = the entries they lie in (found once per wavefront).  The lane's
 * lowest offending pair, or K2A_LLCHK_NONE */
K2A_FN uint32_t k2a_llchk_lane(const K2aLLChk *ent, int elo, int ehi, uint32_t c0, uint32_t c1, int lane, const uint8_t *seq, uint32_t m)
{
	uint32_t best = K2A_LLCHK_NONE;
	for (uint32_t c = c0 + (uint32_t)lane; c <= c1; c += 64) {
		const int e = k2a_llchk_find(ent, elo, ehi, c);
		const K2aLLChk en = ent[e];
		if (k2a_llchk_block(seq, en, c - en.first, m) && en.pair < best) best = en.pair;
	}
	return best;
}

#endif
