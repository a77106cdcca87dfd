/*
 * ksw2_lane_rowmask.h -- the live-row masks of a wavefront of K2aLanePk lanes as C wavefront-uniform 64-bit lane masks.
 *
 * K2aLanePk::step discards the cells of rows outside the band: row c of a lane is live at step k iff
 *     dd - w <= c <= min(rows_m1, dd + w),   dd = k - kd                                   (ksw2_lane_pk.h, "live rows lo..hi")
 * -- per lane a shift, a bit-field extract and a select per ROW, although at any step only the one or two lanes whose strip is
 * entering or leaving the band have a row that is not live.  Read across the wavefront, M_c(k) = { lanes whose row c is live at
 * step k } is one sequence shifted in time: inside a strip, row c at step k and row c - 1 at step k - 1 satisfy the same
 * inequality, so
 *     M_c(k) = M_{c-1}(k-1)                                                               (c >= 1)
 *     M_0(k) = { lanes with rows_m1 >= 0 and -w <= dd <= w }                              (one compare per STEP)
 * with corrections only where the fill kernel already branches wavefront-uniformly:
 *  - a strip that starts at column 0 (i0 <= w) has its rows 0 .. w - i0 live at once, not one per step;
 *  - the last strip of an alignment may have fewer than C rows (rows_m1 < C - 1), and the shift would carry its last row's bit on
 *    into rows that do not exist;
 *  - a strip that ends (end_strip) has no live row from the next step on, wherever its band stands.
 * The first two are repaired by setting every row's mask afresh from the lanes' own band tests (refresh: 2 x C compares, at the
 * one step a column-0 strip starts and at every step while some lane of the wavefront holds a partial strip -- the tail of an
 * alignment), the third by clearing the lanes' bits (on_fin).  Otherwise a step costs one compare for all rows, and a row applies
 * its mask with ONE select whose condition is the scalar register pair.
 * (Masking the partial strips per row instead -- a second set of C lane masks "lanes whose strip has a row c" -- does not fit the
 * scalar registers next to the kernel's own: the compiler keeps them in vector-register lanes and reads them back every step,
 * which costs more than the masks save.)
 *
 * Plain C++ on uint64_t, no device builtins: the same text runs in the fill kernel (k2a_fill_pk_body), where the arguments are
 * ballots, and on the host (tests/rowmask/rowmask_check.cpp), where they are assembled lane by lane.  Every member is
 * wavefront-uniform.  Order inside a step: on_init (if a lane ran do_init), advance, refresh (if needs_refresh), the lanes' step,
 * on_fin (if a lane's strip ended).
 */
#ifndef KSW2_LANE_ROWMASK_H_
#define KSW2_LANE_ROWMASK_H_

#include "ksw2_lane.h"      /* K2A_FN */

template<int C>
struct K2aRowMasks {
	uint64_t m[C];          /* bit l of m[c]: row c of lane l is live at this step */
	uint64_t active;        /* the lanes that hold a strip (rows_m1 >= 0) */
	uint64_t partial;       /* ... one of fewer than C rows */
	uint64_t col0;          /* the lanes whose strip started at this very step with rows at column 0 */

	K2A_FN void reset()
	{
#pragma unroll
		for (int c = 0; c < C; ++c) m[c] = 0;
		active = partial = col0 = 0;
	}

	/* behind the step's do_init: initmask = the lanes that ran it, partmask = those whose new strip has fewer than C rows, col0mask =
	 * those whose new strip has rows that start at column 0 (i0 <= w).  (A lane's previous strip has ended by then -- on_fin -- so
	 * its bits in m[] are clear.) */
	K2A_FN void on_init(uint64_t initmask, uint64_t partmask, uint64_t col0mask)
	{
		active |= initmask;
		partial |= partmask & initmask;
		col0 = col0mask & initmask;
	}

	/* top of a step: every row takes over the row above it as of one step ago.  row0_inband = the lanes with -w <= dd <= w (their
	 * row 0 is inside the band if they hold a strip at all). */
	K2A_FN void advance(uint64_t row0_inband)
	{
#pragma unroll
		for (int c = C - 1; c >= 1; --c) m[c] = m[c - 1];
		m[0] = row0_inband & active;
	}

	/* the shift is not the whole story at this step: refresh() has to follow advance() */
	K2A_FN bool needs_refresh() const { return (partial | col0) != 0; }

	/* live_c[c] = the lanes whose own band test calls row c live at this step */
	K2A_FN void refresh(const uint64_t *live_c)
	{
#pragma unroll
		for (int c = 0; c < C; ++c) m[c] = live_c[c];
		col0 = 0;
	}

	/* the lanes of finmask ended their strip at this step (end_strip): all their rows are dead from the next step on */
	K2A_FN void on_fin(uint64_t finmask)
	{
#pragma unroll
		for (int c = 0; c < C; ++c) m[c] &= ~finmask;
		active &= ~finmask;
		partial &= ~finmask;
	}
};

#endif
