/*
 * ksw2_lane_ll.h -- per-lane code of the local-alignment kernels (ksw_ll_i16 / ksw2amd_ll_batch, ksw2.h:92-93), shared by the gfx950
 * kernel (ksw2_shim_hip.hip) and the lock-step simulator of the tests (tests/llsim).
 *
 * Contract: H(i,j) = max(0, H(i-1,j-1) + s(t_i, q_j), E(i,j), F(i,j)) with Gotoh E / F, a gap of length l
 * costing gapo + l * gape, over the full unbanded matrix; the result is the largest H and its cell, ties broken by the smallest
 * target index, then the smallest query index; a best score of 0 reports (-1, -1).
 *
 * Every value of a local alignment is >= 0, so E and F are held clamped at 0: H = max(0, ...) does not change, and the boundary
 * (row -1, column -1) is all zeros.  Two number formats share the schedule:
 *   int32 (PK = false): one alignment per wavefront, exact for any length;
 *   packed (PK = true): two alignments of the same shape per wavefront, one per 16-bit half of every register, in unsigned
 *     saturating arithmetic (v_pk_add_u16 / v_pk_sub_u16 with clamp, v_pk_max_u16).  Exact as long as H + smax never exceeds
 *     65535: the host admits a pair only when (min(qlen, tlen) + 1) * smax <= 65535 (ksw2_host_ll.c, ll_pk_admit).
 *
 * Schedule (the strip schedule of ksw2_lane.h without a band): rows are the longer sequence, cut into generations of 64 strips of
 * C rows; lane l owns strip l of a generation and walks the columns one per step, skewed by l steps, so the bottom row's (H, E) of
 * strip l reaches lane l + 1 by one DPP rotate per value and step.  Lane 63's bottom row goes to a per-task boundary in HBM
 * (8 bytes per column; DUAL: 16, H, E, E2 and a pad word moved as one access) that lane 0 reads in the next generation.  Generations run one after the other: 63 idle lane-steps per
 * generation and lane, and every lane changes strips at the same step.
 *
 * Maximum: every row keeps its largest H and the first column that reached it (strict >, columns ascending); at the end of a
 * generation the rows are folded into the lane's key (score, -te, -qe), and the 64 keys are reduced once per task.
 *
 * Scores come from pen = smax - s, a byte per (row code, column code): with m <= 5 from two (int32) or three (packed) registers
 * per row built at the start of a generation and one v_perm_b32 per row and step ("column profile"); for any m up to 127 from a
 * table in LDS (one ds_read_u8 per row, alignment and step).
 */
#ifndef KSW2_LANE_LL_H_
#define KSW2_LANE_LL_H_

#include "ksw2_lane.h"

/* ---- packed 16-bit helpers: a uint32 holds two unsigned halves */
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short k2a_ll_u16x2 __attribute__((ext_vector_type(2)));
K2A_FN k2a_ll_u16x2 k2a_ll_h2(uint32_t a) { return __builtin_bit_cast(k2a_ll_u16x2, a); }
K2A_FN uint32_t k2a_ll_w2(k2a_ll_u16x2 a) { return __builtin_bit_cast(uint32_t, a); }
K2A_FN uint32_t k2a_ll_adds(uint32_t a, uint32_t b) { return k2a_ll_w2(__builtin_elementwise_add_sat(k2a_ll_h2(a), k2a_ll_h2(b))); }
K2A_FN uint32_t k2a_ll_subs(uint32_t a, uint32_t b) { return k2a_ll_w2(__builtin_elementwise_sub_sat(k2a_ll_h2(a), k2a_ll_h2(b))); }
K2A_FN uint32_t k2a_ll_max(uint32_t a, uint32_t b) { return k2a_ll_w2(__builtin_elementwise_max(k2a_ll_h2(a), k2a_ll_h2(b))); }
K2A_FN uint32_t k2a_ll_min(uint32_t a, uint32_t b) { return k2a_ll_w2(__builtin_elementwise_min(k2a_ll_h2(a), k2a_ll_h2(b))); }
K2A_FN uint32_t k2a_ll_mul(uint32_t a, uint32_t b) { return k2a_ll_w2(k2a_ll_h2(a) * k2a_ll_h2(b)); }
K2A_FN uint32_t k2a_ll_perm(uint32_t s0, uint32_t s1, uint32_t sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
#else
K2A_FN uint32_t k2a_ll_op(uint32_t a, uint32_t b, int op)
{
	uint32_t r = 0;
	for (int h = 0; h < 2; ++h) {
		const int32_t x = (int32_t)((a >> (16 * h)) & 0xffffu), y = (int32_t)((b >> (16 * h)) & 0xffffu);
		int32_t v = op == 0 ? x + y : op == 1 ? x - y : op == 2 ? (x > y ? x : y) : op == 3 ? (x < y ? x : y) : (int32_t)((uint32_t)(x * y) & 0xffffu);
		v = v < 0 ? 0 : v > 0xffff ? 0xffff : v;
		r |= (uint32_t)v << (16 * h);
	}
	return r;
}
K2A_FN uint32_t k2a_ll_adds(uint32_t a, uint32_t b) { return k2a_ll_op(a, b, 0); }
K2A_FN uint32_t k2a_ll_subs(uint32_t a, uint32_t b) { return k2a_ll_op(a, b, 1); }
K2A_FN uint32_t k2a_ll_max(uint32_t a, uint32_t b) { return k2a_ll_op(a, b, 2); }
K2A_FN uint32_t k2a_ll_min(uint32_t a, uint32_t b) { return k2a_ll_op(a, b, 3); }
K2A_FN uint32_t k2a_ll_mul(uint32_t a, uint32_t b) { return k2a_ll_op(a, b, 4); }
/* v_perm_b32: byte k of the result = byte sel_k of {s0:s1} (s1 = bytes 0-3); selector 12 = 0x00 (the only other one used here) */
K2A_FN uint32_t k2a_ll_perm(uint32_t s0, uint32_t s1, uint32_t sel)
{
	const uint64_t d = ((uint64_t)s0 << 32) | s1;
	uint32_t r = 0;
	for (int k = 0; k < 4; ++k) {
		const uint32_t b = (sel >> (8 * k)) & 0xffu;
		const uint32_t v = b < 8 ? (uint32_t)(d >> (8 * b)) & 0xffu : b >= 13 ? 0xffu : 0u;
		r |= v << (8 * k);
	}
	return r;
}
#endif

/* the lane's best cell so far: larger score, then smaller te, then smaller qe */
struct K2aLLKey { int s, te, qe; };
K2A_FN bool k2a_ll_better(int s, int te, int qe, const K2aLLKey &k)
{
	return s > k.s || (s == k.s && (te < k.te || (te == k.te && qe < k.qe)));
}
K2A_FN void k2a_ll_key_reset(K2aLLKey &k) { k.s = 0; k.te = -1; k.qe = -1; }

/* PK: two alignments per lane (packed form); LDSP: scores from the LDS table (else the register column profile, m <= 5).
 * REV: the start-cell pass of ksw2amd_ll_align_batch -- the same recurrence over the REVERSED prefixes that
 * end in the forward pass's best cell: half h covers rows [0, rl[h]) and columns [0, cl[h]) of the task (set_limits), row i holds
 * r[rl - 1 - i] and column j holds c[cl - 1 - j].  The two halves of a packed task run over their bounding rectangle; a cell depends
 * only on cells above and to its left, so the cells outside a half's own rectangle cannot change one inside it and only have to be
 * kept out of that half's maximum: the row-maximum update carries a per-half column test, gen_end a per-half row test. */
/* 16 bytes of the row profile (ksw2amd_ll_sub_batch): four rows' maxima, or their first columns */
#if defined(__clang__)
typedef uint32_t k2a_ll_v4 __attribute__((ext_vector_type(4)));
#else
typedef uint32_t k2a_ll_v4 __attribute__((vector_size(16)));
#endif

/* SUB (with REV = false, rows = target): the forward pass of ksw2amd_ll_sub_batch.  Nothing changes in the
 * recurrence; sub_store(), called next to gen_end(), writes the lane's rows of (rmax, rcol) to the task's row profile in HBM, from
 * which k2a_ll_sub_kernel (ksw2_lane_llsub.h) takes the best row outside the window around the best cell. */
/* DUAL: the two-piece gap cost of ksw2amd_lld_batch, min(gapo + l * gape, gapo2 + l * gape2) for a gap of
 * length l: a second pair of gap states E2 / F2 under (oe2, ge2) beside E / F, clamped at 0 like them (max(0, .., max(X, 0)) = max(0, .., X),
 * and max(H - oe, max(X, 0) - ge, 0) = max(max(H - oe, X - ge), 0) because -ge <= 0: H never sees the clamp), f2[] per row and
 * an e2 chain down the strip that reaches the lane below (and the boundary) with H and E.  With DUAL = false nothing of it exists. */
/* FIT (rows = target, never with SUB; with DUAL: below): the semi-global mode of ksw2amd_sg_batch -- the whole query
 * against the best interval of the target, no clamp at 0.  With B = gapo + ncols * gape every true H(t, j) >= -(gapo + (j + 1) * gape) >= -B
 * (insert the query up to column j), so the cell update runs unchanged on H' = H + B >= 0; E' and F' held clamped at 0 stand for values
 * <= -B, which reach an H only where H = -B itself.  What differs is the boundary -- column -1 is B in every row (H(t, -1) = 0), row -1 is
 * B - (gapo + (j + 1) * gape) = (ncols - 1 - j) * gape (fit_top) -- and the maximum: it is taken over the last column only, which is what
 * hl[] holds when a lane has walked its columns, so step() keeps no row maximum at all and gen_end folds hl[] into (largest H', smallest
 * row).  The key starts at -1, below any H'; the score is H' - B.
 * FIT with REV: the start pass of ksw2amd_sg_align_batch -- the global alignment of the whole reversed query against
 * the reversed target prefix that ends in the forward pass's row te, anchored at (te, ncols - 1) and free to end in any row.  Row i holds
 * r[te - i] (rl = te + 1), column j holds c[ncols - 1 - j] (cl = ncols for every half).  Row -1 is fit_top as it stands; column -1 is the
 * global boundary H'(i, -1) = B - (gapo + (i + 1) * gape) = (ncols - 1 - i) * gape held at 0 (fit_left) where the forward pass has B.  The key
 * starts at (0, row -1): H'(-1, ncols - 1) = 0 is the empty interval, and k2a_ll_better lets it win its ties.
 * FIT with DUAL (with and without REV): the same two passes under the two-piece cost of ksw2amd_sgd_batch / ksw2amd_sgd_align_batch
 * (DESIGN.md section 3.22).  cost(l) = min(gapo + l * gape, gapo2 + l * gape2), the pieces as the caller orders them; B = cost(ncols), row -1
 * is B - cost(j + 1) with E' and E2' opened from it, column -1 of the reverse pass is max(B - cost(i + 1), 0), and F2' of column 0 is opened
 * from column -1 like F'.  cost() is non-decreasing, so cost(j + 1) <= B and the arguments above carry over; step() is DUAL's as it stands. */
/* OV (with FIT, with and without DUAL; with REV: below): the overlap mode of ksw2amd_ov_batch / ksw2amd_ovd_batch --
 * FIT with free query ends, chosen per task by `ends` (K2aLLTask.pad: bit 0 the query's start, bit 1 its end; wavefront-uniform).
 * Bit 0: row -1 is H(-1, j) = 0, i.e. H' = B in every column with E' = sat(B - oe) (and E2') opened from it, in place of fit_top's ramp.
 * Every true H(t, j) is still >= -cost(j + 1) >= -B (start in column -1 of row t, insert the query up to j), so the bias and the clamped gap
 * states hold as they do for FIT.
 * Bit 1: the cells of the last target row are candidates too.  That row lies in the last generation, in one lane, in strip register
 * clast = (nrows - 1) % C -- the same register in every lane, so in that generation every lane folds hl[clast] after each step into one
 * running (maximum, first column) per half (strict >, columns ascending; packed: the row-maximum idiom of the local step, 16-bit column),
 * and in gen_end the lane that owns row nrows - 1 folds (maximum, nrows - 1, column) into its key beside the last column.  The fold starts
 * at (0, column 0), which is never above the real cell of column 0 (H' >= 0) and equals it when that cell is 0.
 * OV with REV: the start pass of ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch -- FIT with REV over the reversed
 * prefix that ends in the forward pass's cell (te, qe): rl = te + 1 and cl = qe + 1 per half, and qe may lie before the last column.  B stays
 * cost(bcols) of the forward task's columns, so row -1 (always fit_top's ramp here, whatever bit 0 says) and fit_left are taken from bcols and
 * not from the rectangle.  Packed: a half stops changing hl[] once jj has left its own columns (cmask), so hl[] holds the half's last column
 * cl[h] - 1 when the lane has walked the task's.  The key starts at row -1 of that column, (B - cost(cl[h]), -1, cl[h] - 1).  Bit 0 (the free
 * query start of the forward pass) makes the rectangle's last row a candidate row: in the generation that holds row rl[h] - 1 every lane folds
 * strip register clr[h] = (rl[h] - 1) % C of half h as the forward pass folds clast -- generation and register may differ between the halves --
 * and in gen_end its owner folds column -1, max(B - cost(rl[h]), 0), then (maximum, first column) into the key: smallest row, then smallest
 * column, so the last row loses to every other row of the last column and wins over the corner (rl - 1, cl - 1). */
template<bool PK, bool LDSP, bool REV = false, bool SUB = false, bool DUAL = false, bool FIT = false, bool OV = false>
struct K2aLaneLL {
	enum { C = K2A_LL_C, NH = PK ? 2 : 1 };
	int nrows, ncols, swapped, m, lane, i0;
	uint32_t smax, oe, ge;                     /* packed: the value in both halves */
	uint32_t oe2, ge2;                         /* DUAL: the second piece */
	uint32_t bias;                             /* FIT: B, in both halves when packed */
	uint32_t hu_prev;                          /* H(i0 - 1, jj - 1): what the lane above delivered one step earlier */
	uint32_t hl[C], f[C], rmax[C], rcol[C];    /* H(i, jj - 1), F(i, jj), row maximum and its first column */
	uint32_t f2[DUAL ? C : 1];                 /* DUAL: F2(i, jj) */
	uint32_t pa[C], pb[PK ? C : 1], pw[LDSP ? 1 : C];   /* register profile: pen bytes for column codes 0..3 (pa: low half, pb: high
	                                                     * half), pw: code 4; LDS profile: pa / pb = row code * m */
	int ends, clast;                           /* OV: the task's free query ends; the last row's strip register in the last generation, else -1 */
	uint32_t lmax, lcol;                       /* OV: the last row's largest H' so far and its first column */
	int bcols, clr[OV && REV ? NH : 1];        /* OV with REV: the columns B was taken from; the last row's strip register per half in its generation, else -1 */
	K2aLLKey key[NH];
	int rl[REV ? NH : 1], cl[REV ? NH : 1];    /* REV: rows / columns of each half's prefix rectangle (0: the half scored 0) */

	/* REV, after init: the halves' limits; the task then runs over rows [0, max rl) and columns [0, max cl) */
	K2A_FN void set_limits(const int *rl_, const int *cl_)
	{
		nrows = ncols = 0;
		for (int h = 0; h < (REV ? NH : 1); ++h) {
			rl[h] = rl_[h]; cl[h] = cl_[h];
			nrows = k2a_max(nrows, rl[h]); ncols = k2a_max(ncols, cl[h]);
			if (OV && REV) {                       /* row -1 of the half's last column: the empty target interval */
				key[h].s = fit_bias() - ov_cost(cl[h]); key[h].te = -1; key[h].qe = cl[h] - 1;
			}
		}
	}

	K2A_FN void init(const K2aLL &par, const K2aLLTask &tk, int lane_)
	{
		nrows = tk.nrows; ncols = tk.ncols; swapped = tk.swapped; m = par.m; lane = lane_;
		const uint32_t x = PK ? 0x10001u : 1u;
		smax = (uint32_t)par.smax * x; oe = (uint32_t)par.oe * x; ge = (uint32_t)par.ge * x;
		if (DUAL) { oe2 = (uint32_t)par.oe2 * x; ge2 = (uint32_t)par.ge2 * x; }
		for (int h = 0; h < NH; ++h) k2a_ll_key_reset(key[h]);
		if (FIT) {
			bias = (uint32_t)(par.oe - par.ge + ncols * par.ge) * x;
			if (DUAL) bias = (uint32_t)k2a_min(par.oe - par.ge + ncols * par.ge, par.oe2 - par.ge2 + ncols * par.ge2) * x;      /* cost(ncols) */
			if (!REV) for (int h = 0; h < NH; ++h) key[h].s = -1;      /* REV: (0, -1), row -1 of the last column */
		}
		if (OV) { ends = tk.pad; clast = -1; lmax = lcol = 0; }
		if (OV && REV) { bcols = ncols; for (int h = 0; h < NH; ++h) clr[OV && REV ? h : 0] = -1; }
	}

	/* FIT: B, and row -1 of column k for lane 0 of the first generation: H'(-1, k) and E'(0, k) = sat(H'(-1, k) - oe) */
	K2A_FN int fit_bias() const { return (int)(bias & (PK ? 0xffffu : 0xffffffffu)); }
	K2A_FN void fit_top(int k, uint32_t &h, uint32_t &e) const
	{
		if (OV && !REV && (ends & 1)) { h = bias; e = PK ? k2a_ll_subs(bias, oe) : (uint32_t)k2a_max((int)bias - (int)oe, 0); return; }      /* H(-1, k) = 0 */
		const int v = ((OV && REV ? bcols : ncols) - 1 - k) * (int)(ge & (PK ? 0xffffu : 0xffffffffu)), w = k2a_max(v - (int)(oe & (PK ? 0xffffu : 0xffffffffu)), 0);
		h = (uint32_t)v * (PK ? 0x10001u : 1u); e = (uint32_t)w * (PK ? 0x10001u : 1u);
	}

	/* FIT with DUAL: cost(l), l >= 1, from the lane's copies of the four costs */
	K2A_FN int fit_cost(int l) const
	{
		const uint32_t mk = PK ? 0xffffu : 0xffffffffu;
		return k2a_min((int)(oe & mk) + (l - 1) * (int)(ge & mk), (int)(oe2 & mk) + (l - 1) * (int)(ge2 & mk));
	}
	/* ... row -1 of column k: H'(-1, k) = B - cost(k + 1), E'(0, k) = sat(H' - oe), E2'(0, k) = sat(H' - oe2) */
	K2A_FN void fit_top(int k, uint32_t &h, uint32_t &e, uint32_t &e2) const
	{
		const uint32_t mk = PK ? 0xffffu : 0xffffffffu;
		if (OV && !REV && (ends & 1)) {
			h = bias; e = PK ? k2a_ll_subs(bias, oe) : (uint32_t)k2a_max((int)bias - (int)oe, 0);
			e2 = PK ? k2a_ll_subs(bias, oe2) : (uint32_t)k2a_max((int)bias - (int)oe2, 0);
			return;
		}
		const int v = fit_bias() - fit_cost(k + 1), w = k2a_max(v - (int)(oe & mk), 0), w2 = k2a_max(v - (int)(oe2 & mk), 0);
		h = (uint32_t)v * (PK ? 0x10001u : 1u); e = (uint32_t)w * (PK ? 0x10001u : 1u); e2 = (uint32_t)w2 * (PK ? 0x10001u : 1u);
	}

	/* FIT with REV: column -1 of row i, H'(i, -1) = max(ncols - 1 - i, 0) * gape (i = -1: B); DUAL: max(B - cost(i + 1), 0) */
	K2A_FN uint32_t fit_left(int i) const
	{
		if (DUAL) return i < 0 ? bias : (uint32_t)k2a_max(fit_bias() - fit_cost(i + 1), 0) * (PK ? 0x10001u : 1u);
		return i < 0 ? bias : (uint32_t)(k2a_max((OV && REV ? bcols : ncols) - 1 - i, 0) * (int)(ge & (PK ? 0xffffu : 0xffffffffu))) * (PK ? 0x10001u : 1u);
	}

	/* OV with REV: cost(l), l >= 1, under the entry's one or two pieces */
	K2A_FN int ov_cost(int l) const
	{
		const uint32_t mk = PK ? 0xffffu : 0xffffffffu;
		return DUAL ? fit_cost(l) : (int)(oe & mk) + (l - 1) * (int)(ge & mk);
	}
	/* ... and strip register c of hl[], c wavefront-uniform: no indexed register access */
	K2A_FN uint32_t ov_pick(int c) const
	{
		uint32_t v = hl[0];
		switch (c) {
#define K2A_LL_OVSEL(c) case c: v = hl[c]; break;
		K2A_LL_OVSEL(1) K2A_LL_OVSEL(2) K2A_LL_OVSEL(3) K2A_LL_OVSEL(4) K2A_LL_OVSEL(5) K2A_LL_OVSEL(6) K2A_LL_OVSEL(7) K2A_LL_OVSEL(8)
		K2A_LL_OVSEL(9) K2A_LL_OVSEL(10) K2A_LL_OVSEL(11) K2A_LL_OVSEL(12) K2A_LL_OVSEL(13) K2A_LL_OVSEL(14) K2A_LL_OVSEL(15)
#undef K2A_LL_OVSEL
		default: break;
		}
		return v;
	}

	/* start generation g: this lane's rows, their profile, zeroed columns (tab = the task's pen table in LDS, [row code * m + column code]) */
	K2A_FN void gen_begin(int g, const uint8_t *r0, const uint8_t *r1, const uint8_t *tab)
	{
		i0 = g * K2A_LL_ROWS + lane * C;
		if (OV && !REV) { clast = ((ends & 2) && (g + 1) * K2A_LL_ROWS >= nrows) ? (nrows - 1) % C : -1; lmax = lcol = 0; }
		if (OV && REV) {                           /* the halves' last rows: this generation's or not, per half */
			lmax = lcol = 0;
			for (int h = 0; h < NH; ++h) clr[OV && REV ? h : 0] = ((ends & 1) && rl[REV ? h : 0] > 0 && (rl[REV ? h : 0] - 1) / K2A_LL_ROWS == g) ? (rl[REV ? h : 0] - 1) % C : -1;
		}
		hu_prev = !FIT ? 0u : REV ? fit_left(i0 - 1) : bias;
		const uint32_t f0 = !FIT ? 0u : PK ? k2a_ll_subs(bias, oe) : (uint32_t)k2a_max((int)bias - (int)oe, 0);      /* FIT: F'(i, 0) = sat(B - oe) */
#pragma unroll
		for (int c = 0; c < C; ++c) {
			const int i = i0 + c;
			uint32_t a, b;
			if (REV) {                             /* row i of a half is r[rl - 1 - i]; past the half's limit: code 0, never a byte out of bounds */
				a = i < rl[0] ? r0[rl[0] - 1 - i] : 0u;
				b = (PK && i < rl[REV ? NH - 1 : 0]) ? r1[rl[REV ? NH - 1 : 0] - 1 - i] : 0u;
			} else {
				a = i < nrows ? r0[i] : 0u; b = (PK && i < nrows) ? r1[i] : 0u;
			}
			hl[c] = !FIT ? 0u : REV ? fit_left(i) : bias; rmax[c] = 0; rcol[c] = 0;
			f[c] = !(FIT && REV) ? f0 : PK ? k2a_ll_subs(hl[c], oe) : (uint32_t)k2a_max((int)hl[c] - (int)oe, 0);      /* F'(i, 0) = sat(H'(i, -1) - oe) */
			if (DUAL) f2[DUAL ? c : 0] = !FIT ? 0u : PK ? k2a_ll_subs(hl[c], oe2) : (uint32_t)k2a_max((int)hl[c] - (int)oe2, 0);      /* FIT: F2'(i, 0) = sat(H'(i, -1) - oe2) */
			if (LDSP) {
				pa[c] = a * (uint32_t)m;
				if (PK) pb[c] = b * (uint32_t)m;
			} else {
				const uint8_t *ta = tab + a * m, *tb = tab + b * m;
				uint32_t wa = 0, wb = 0, w4 = 0;
				for (int k = 0; k < 4; ++k) {
					if (k < m) { wa |= (uint32_t)ta[k] << (8 * k); if (PK) wb |= (uint32_t)tb[k] << (8 * k); }
				}
				if (m > 4) w4 = (uint32_t)ta[4] | (PK ? (uint32_t)tb[4] << 16 : 0u);
				pa[c] = wa;
				if (PK) pb[c] = wb;
				if (!LDSP) pw[LDSP ? 0 : c] = w4;
			}
		}
	}

	/* one column jj of the strip.  hin / ein: H(i0 - 1, jj) and E(i0, jj) from the lane above (or the boundary);
	 * qc: column code (packed: low byte for the low half, next byte for the high half); hout / eout: the same for the lane below */
	K2A_FN void step(int jj, uint32_t hin, uint32_t ein, uint32_t qc, const uint8_t *tab, uint32_t &hout, uint32_t &eout)
	{
		uint32_t e2out;
		step(jj, hin, ein, 0u, qc, tab, hout, eout, e2out);
	}

	/* the same with the second piece's chain: e2in = E2(i0, jj) from the lane above, e2out for the lane below (DUAL = false: unused) */
	K2A_FN void step(int jj, uint32_t hin, uint32_t ein, uint32_t e2in, uint32_t qc, const uint8_t *tab, uint32_t &hout, uint32_t &eout, uint32_t &e2out)
	{
		uint32_t hd = hu_prev, e = ein, e2 = e2in;
		hu_prev = hin;
		uint32_t sel = 0, wmask = 0, q0 = qc & 0xffu, q1 = (qc >> 8) & 0xffu;
		if (!LDSP) {
			if (PK) {
				sel = (q0 < 4 ? q0 : 12u) | (12u << 8) | ((q1 < 4 ? 4u + q1 : 12u) << 16) | (12u << 24);
				wmask = (q0 == 4 ? 0xffffu : 0u) | (q1 == 4 ? 0xffff0000u : 0u);
			} else sel = q0 | 0x0c0c0c00u;
		}
		const uint32_t jj2 = PK ? (uint32_t)jj * 0x10001u : (uint32_t)jj;
		/* REV, packed: all ones in a half whose own rectangle holds column jj (the int32 form runs its exact rectangle) */
		const uint32_t cmask = (REV && PK) ? (jj < cl[0] ? 0xffffu : 0u) | (jj < cl[REV ? NH - 1 : 0] ? 0xffff0000u : 0u) : 0xffffffffu;
#pragma unroll
		for (int c = 0; c < C; ++c) {
			uint32_t pen;
			if (LDSP) pen = PK ? (uint32_t)tab[pa[c] + q0] | ((uint32_t)tab[pb[c] + q1] << 16) : (uint32_t)tab[pa[c] + q0];
			else if (PK) pen = k2a_ll_perm(pb[c], pa[c], sel) | (pw[LDSP ? 0 : c] & wmask);
			else pen = k2a_ll_perm(pw[LDSP ? 0 : c], pa[c], sel);
			uint32_t h;
			if (PK) {
				h = k2a_ll_max(k2a_ll_max(k2a_ll_subs(k2a_ll_adds(hd, smax), pen), e), f[c]);
				if (DUAL) h = k2a_ll_max(k2a_ll_max(h, e2), f2[DUAL ? c : 0]);
				const uint32_t hoe = k2a_ll_subs(h, oe);
				e = k2a_ll_max(hoe, k2a_ll_subs(e, ge));
				f[c] = k2a_ll_max(hoe, k2a_ll_subs(f[c], ge));
				if (DUAL) {
					const uint32_t hoe2 = k2a_ll_subs(h, oe2);
					e2 = k2a_ll_max(hoe2, k2a_ll_subs(e2, ge2));
					f2[DUAL ? c : 0] = k2a_ll_max(hoe2, k2a_ll_subs(f2[DUAL ? c : 0], ge2));
				}
				if (!FIT) {
					const uint32_t hm = (REV && PK) ? h & cmask : h;                  /* REV: 0 in a half whose rectangle ends before jj */
					const uint32_t d = k2a_ll_subs(hm, rmax[c]);                      /* > 0 in a half where h is a new row maximum */
					const uint32_t mask = k2a_ll_mul(k2a_ll_min(d, 0x10001u), 0xffffffffu);
					rmax[c] = k2a_ll_max(rmax[c], hm);
					rcol[c] = (jj2 & mask) | (rcol[c] & ~mask);
				}
			} else {
				const int t = (int)hd + (int)smax - (int)pen;                          /* e, f >= 0: h >= 0 without a clamp */
				int hi = k2a_max(k2a_max(t, (int)e), (int)f[c]);
				if (DUAL) hi = k2a_max3(hi, (int)e2, (int)f2[DUAL ? c : 0]);
				const int hoe = hi - (int)oe;
				e = (uint32_t)k2a_max3(hoe, (int)e - (int)ge, 0);
				f[c] = (uint32_t)k2a_max3(hoe, (int)f[c] - (int)ge, 0);
				if (DUAL) {
					const int hoe2 = hi - (int)oe2;
					e2 = (uint32_t)k2a_max3(hoe2, (int)e2 - (int)ge2, 0);
					f2[DUAL ? c : 0] = (uint32_t)k2a_max3(hoe2, (int)f2[DUAL ? c : 0] - (int)ge2, 0);
				}
				h = (uint32_t)hi;
				if (!FIT && hi > (int)rmax[c]) { rmax[c] = h; rcol[c] = jj2; }
			}
			hd = hl[c];
			hl[c] = (OV && REV && PK) ? (h & cmask) | (hl[c] & ~cmask) : h;      /* OV with REV: a half past its own last column keeps it */
		}
		hout = hl[C - 1];
		eout = e;
		e2out = e2;
		if (OV && REV) {
			if (clr[0] >= 0 || clr[OV && REV ? NH - 1 : 0] >= 0) {      /* a generation that holds a half's last row, the query's start free */
				uint32_t v = ov_pick(clr[0]);
				if (PK) {
					v = (clr[0] >= 0 ? v & 0xffffu : 0u) | (clr[OV && REV ? NH - 1 : 0] >= 0 ? ov_pick(clr[OV && REV ? NH - 1 : 0]) & 0xffff0000u : 0u);
					const uint32_t d = k2a_ll_subs(v, lmax);
					const uint32_t mask = k2a_ll_mul(k2a_ll_min(d, 0x10001u), 0xffffffffu);
					lmax = k2a_ll_max(lmax, v);
					lcol = (jj2 & mask) | (lcol & ~mask);
				} else if ((int)v > (int)lmax) { lmax = v; lcol = jj2; }
			}
		} else if (OV && clast >= 0) {                    /* the last generation of a task with a free query end: one row's running maximum */
			uint32_t v = hl[0];
			switch (clast) {                       /* wavefront-uniform: no indexed register access */
#define K2A_LL_OVSEL(c) case c: v = hl[c]; break;
			K2A_LL_OVSEL(1) K2A_LL_OVSEL(2) K2A_LL_OVSEL(3) K2A_LL_OVSEL(4) K2A_LL_OVSEL(5) K2A_LL_OVSEL(6) K2A_LL_OVSEL(7) K2A_LL_OVSEL(8)
			K2A_LL_OVSEL(9) K2A_LL_OVSEL(10) K2A_LL_OVSEL(11) K2A_LL_OVSEL(12) K2A_LL_OVSEL(13) K2A_LL_OVSEL(14) K2A_LL_OVSEL(15)
#undef K2A_LL_OVSEL
			default: break;
			}
			if (PK) {
				const uint32_t d = k2a_ll_subs(v, lmax);                              /* > 0 in a half where v is a new maximum */
				const uint32_t mask = k2a_ll_mul(k2a_ll_min(d, 0x10001u), 0xffffffffu);
				lmax = k2a_ll_max(lmax, v);
				lcol = (jj2 & mask) | (lcol & ~mask);
			} else if ((int)v > (int)lmax) { lmax = v; lcol = jj2; }
		}
	}

	/* end of a generation: fold the live rows into the lane's key(s).  Every row is looked at (no early exit: the rows past the
	 * end are masked), and the key is replaced field by field with one condition */
	K2A_FN void gen_end()
	{
#pragma unroll
		for (int c = 0; c < C; ++c) {
			const int i = i0 + c;
#pragma unroll
			for (int h = 0; h < NH; ++h) {
				const uint32_t rm = FIT ? hl[c] : rmax[c];                            /* FIT: H'(i, ncols - 1), the row's last column */
				const int s = (int)(PK ? (rm >> (16 * h)) & 0xffffu : rm);
				const int j = (OV && REV) ? cl[REV ? h : 0] - 1 : FIT ? ncols - 1 : (int)(PK ? (rcol[c] >> (16 * h)) & 0xffffu : rcol[c]);
				const int te = swapped ? j : i, qe = swapped ? i : j;
				const bool take = i < (REV ? rl[REV ? h : 0] : nrows) && (FIT || s > 0) && k2a_ll_better(s, te, qe, key[h]);
				key[h].s = take ? s : key[h].s;
				key[h].te = take ? te : key[h].te;
				key[h].qe = take ? qe : key[h].qe;
			}
		}
		if (OV && REV) {                           /* the owner of a half's last row: column -1, then the row's best cell, beside the last column's */
#pragma unroll
			for (int h = 0; h < NH; ++h) {
				const int lr = rl[REV ? h : 0] - 1;
				const bool own = clr[OV && REV ? h : 0] >= 0 && (unsigned)(lr - i0) < (unsigned)C;
				const int s0 = (int)(PK ? fit_left(lr) & 0xffffu : fit_left(lr));
				const int s = (int)(PK ? (lmax >> (16 * h)) & 0xffffu : lmax), j = (int)(PK ? (lcol >> (16 * h)) & 0xffffu : lcol);
				const bool take0 = own && k2a_ll_better(s0, lr, -1, key[h]);
				key[h].s = take0 ? s0 : key[h].s;
				key[h].te = take0 ? lr : key[h].te;
				key[h].qe = take0 ? -1 : key[h].qe;
				const bool take = own && k2a_ll_better(s, lr, j, key[h]);
				key[h].s = take ? s : key[h].s;
				key[h].te = take ? lr : key[h].te;
				key[h].qe = take ? j : key[h].qe;
			}
		} else if (OV && clast >= 0 && (unsigned)(nrows - 1 - i0) < (unsigned)C) {      /* this lane owns the last row: its best cell, beside the last column's */
#pragma unroll
			for (int h = 0; h < NH; ++h) {
				const int s = (int)(PK ? (lmax >> (16 * h)) & 0xffffu : lmax), j = (int)(PK ? (lcol >> (16 * h)) & 0xffffu : lcol);
				const bool take = k2a_ll_better(s, nrows - 1, j, key[h]);
				key[h].s = take ? s : key[h].s;
				key[h].te = take ? nrows - 1 : key[h].te;
				key[h].qe = take ? j : key[h].qe;
			}
		}
	}

	/* SUB, end of a generation: the lane's C words of rmax, then its C words of rcol -- packed: both halves in a word, as the registers
	 * hold them -- to bytes [8 * i0, 8 * i0 + 128) of the task's row profile `prof` (16-byte aligned), in 16-byte stores of four
	 * consecutive registers.  A lane without a live row writes nothing: the profile ends with the last lane that has one
	 * (K2A_LLSUB_BYTES) */
	K2A_FN void sub_store(uint8_t *prof) const
	{
		if (!SUB || i0 >= nrows) return;
		k2a_ll_v4 *p = (k2a_ll_v4*)(prof + (size_t)i0 * 8);
#pragma unroll
		for (int c = 0; c < C; c += 4) {
			k2a_ll_v4 v, w;
			v[0] = rmax[c]; v[1] = rmax[c + 1]; v[2] = rmax[c + 2]; v[3] = rmax[c + 3];
			w[0] = rcol[c]; w[1] = rcol[c + 1]; w[2] = rcol[c + 2]; w[3] = rcol[c + 3];
			p[c / 4] = v; p[C / 4 + c / 4] = w;
		}
	}
};

#endif
