/*
 * ksw2_lane_pkfold.h -- the strip epilogues of a deferred packed fill (K2aLanePk, DEFER, G = 64), folded into the task's two books
 * once, behind the step loop, by the whole wavefront.
 *
 * In such a fill nothing inside the step loop reads the books: no group stops early (k2a_fill_pk_body, NOSTOP) and the columns come
 * from the later passes.  So the lane whose strip ends only STORES what the epilogue would have read -- the strip's row maxima
 * rmax[C] and, if a row of the strip reaches the query end, its last H column hl[C], both as the registers hold them (offset form;
 * hl = H - q in the open form) -- into the strip's record behind the K2aCkHead table of the task's checkpoint block:
 *     record s = K2A_CK_REC_WORDS(C) dwords at rec + s * K2A_CK_REC_WORDS(C):  [0, C) = rmax,  [C, 2C) = hl
 * (i0 = s * C; the bases are the strip's K2aCkHead), and k2a_pkfold_task turns the records 0 .. nstrips - 1 into the books.
 *
 * Result: every field of both books is what K2aLanePk::do_fin_seq (its DEFER branch) leaves when it is called on the strips in
 * order -- per alignment half and row i < tlen, until the book is frozen: mqe on reach rows (strictly greater: the first row keeps a
 * tie), mte on row tlen_full - 1, the maximum (strictly greater) or else the freeze test max - H > zdrop, score on the last row if it
 * reaches and the book is not frozen, rows = i + 1 (the freezing row included).  max_q and mte_q become 0 where max / mte are set,
 * as in the loop (the deferred lanes have no columns; the second pass writes them).
 *
 * Shape: lane l takes strips l, l + 64, ... -- one round per 64 strips.  Per half and round:
 *  1. every lane un-biases its strip's rows to int32 (bases differ per strip and half) and takes their maximum;
 *  2. an inclusive prefix maximum over the lanes (six steps through the exchange buffer) plus the carry of the rounds before gives
 *     every strip the book maximum it is entered with -- true as long as no earlier strip froze the book, and what follows the first
 *     freeze is discarded;
 *  3. every lane walks its C rows with do_fin_seq's own tests and keeps what it found in lane-local bests;
 *  4. a ballot names the first strip that froze; lanes up to it take their walk over, the others drop it, and the rounds end.
 * Whoever owns the last target row or the freezing row writes mte / score / dropped / rows itself (one lane each); the lane-local
 * bests (max, mqe with their rows; a lane sees its rows in increasing order) are merged by lane 0 at the end, ties to the smaller
 * row, which is the sequential order's first occurrence.
 *
 * One text for the device and the host: the per-lane parts are loops over `NL` lanes starting at lane0 -- NL = 1 in the kernel
 * (every array below is a register), NL = 64 on the host (tests/stripfold/stripfold_check.cpp), where the loops ARE the wavefront --
 * and lanes meet only in the exchange buffer xb (LDS in the kernel), between K2A_FOLD_SYNC points, and in the ballot.
 * It reads exactly nstrips records: the blocks are recycled and hold other plans' records behind them.
 */
#ifndef KSW2_LANE_PKFOLD_H_
#define KSW2_LANE_PKFOLD_H_

#include "ksw2_lane_pk.h"

/* (K2A_CK_REC_WORDS, K2A_CK_BLOCK_BYTES: ksw2_types.h -- the host sizes the blocks) */
#define K2A_PKFOLD_XB_WORDS 256             /* exchange buffer: two planes of 64 for the scan, four words per lane for the merge */

#if defined(__HIP_DEVICE_COMPILE__)
#define K2A_FOLD_SYNC() __builtin_amdgcn_wave_barrier()
#define K2A_FOLD_BALLOT(p, l) __builtin_amdgcn_ballot_w64(p)
#else
#define K2A_FOLD_SYNC() do {} while (0)
#define K2A_FOLD_BALLOT(p, l) ((uint64_t)((p) ? 1u : 0u) << (l))
#endif

/* does a row of strip s reach the query end?  Only then is the record's hl part written, and read.  (Rows reach from some row on,
 * so the strip's last existing row decides.) */
template<int C>
K2A_FN bool k2a_pkfold_strip_reaches(int s, int qlen, int tlen, int w) { return k2a_min(s * C + C - 1, tlen - 1) + w >= qlen - 1; }

template<int C, int NL>
K2A_FN void k2a_pkfold_task(const K2aScoring &sc, const uint32_t *rec, const K2aCkHead *hd, int nstrips, int qlen, int tlen, int tlen_full, int w,
                            int zdropA, int zdropB, K2aBook *bkA, K2aBook *bkB, uint32_t *xb, int lane0)
{
	const int hq = k2a_hl_q(sc);
	const int none = (int)0x80000000;
	int *xi = (int*)xb;
#pragma nounroll
	for (int half = 0; half < 2; ++half) {
		K2aBook *b = half ? bkB : bkA;
		const int zdrop = half ? zdropB : zdropA, sh = half ? 16 : 0;
		int lm[NL], lmt[NL], lq[NL], lqt[NL];                      /* lane-local bests: maximum and its row, mqe and its row */
		for (int x = 0; x < NL; ++x) { lm[x] = lq[x] = none; lmt[x] = lqt[x] = -1; }
		int carry = b->max;                                        /* the book maximum in front of the round */
		const bool dead = b->dropped != 0 || nstrips <= 0;
		bool frozen = false;
		K2A_FOLD_SYNC();
#pragma nounroll
		for (int s0 = 0; s0 < nstrips && !dead && !frozen; s0 += 64) {
			int H[NL][C], hend[NL][C], ent[NL];
			/* 1. the strips' rows, un-biased; their maxima into the exchange buffer */
			for (int x = 0; x < NL; ++x) {
				const int l = lane0 + x, s = s0 + l;
				int sm = none;
				if (s < nstrips) {
					const uint32_t *r = rec + (size_t)s * K2A_CK_REC_WORDS(C);
					const int base = half ? hd[s].baseB : hd[s].baseA;
					const bool rs = k2a_pkfold_strip_reaches<C>(s, qlen, tlen, w);
#pragma unroll
					for (int c = 0; c < C; ++c) {
						const int i = s * C + c, unb = base - sc.e * i;                  /* plus base, minus row bias */
						H[x][c] = (int)(int16_t)(k2a_ofs_off(r[c]) >> sh) + unb;
						hend[x][c] = rs ? (int)(int16_t)(k2a_ofs_off(r[C + c]) >> sh) + hq + unb : none;
						if (i < tlen) sm = k2a_max(sm, H[x][c]);
					}
				}
				xi[l] = sm;
			}
			K2A_FOLD_SYNC();
			/* 2. inclusive prefix maximum over the lanes: six steps, from one plane of the buffer to the other and back */
			int src = 0;
#pragma nounroll
			for (int d = 1; d < 64; d <<= 1) {
				for (int x = 0; x < NL; ++x) {
					const int l = lane0 + x;
					int v = xi[src + l];
					if (l >= d) v = k2a_max(v, xi[src + l - d]);
					xi[(src ^ 64) + l] = v;
				}
				K2A_FOLD_SYNC();
				src ^= 64;
			}
			for (int x = 0; x < NL; ++x) { const int l = lane0 + x; ent[x] = l > 0 ? k2a_max(carry, xi[src + l - 1]) : carry; }
			carry = k2a_max(carry, xi[src + 63]);
			K2A_FOLD_SYNC();
			/* 3. the rows of every strip, with do_fin_seq's tests; 4. the first strip that froze */
			int tm[NL], tmt[NL], tq[NL], tqt[NL], tmte[NL], tsc[NL], trows[NL];
			bool fr[NL], hmte[NL], hsc[NL];
			uint64_t fmask = 0;
			for (int x = 0; x < NL; ++x) {
				const int s = s0 + lane0 + x;
				int m = ent[x];
				tm[x] = lm[x]; tmt[x] = lmt[x]; tq[x] = lq[x]; tqt[x] = lqt[x]; tmte[x] = tsc[x] = trows[x] = 0;
				fr[x] = hmte[x] = hsc[x] = false;
				if (s < nstrips) {
#pragma unroll
					for (int c = 0; c < C; ++c) {
						const int i = s * C + c;
						if (i < tlen && !fr[x]) {
							const bool reach = i + w >= qlen - 1;
							const int h = H[x][c], he = hend[x][c];
							if (reach && he > tq[x]) { tq[x] = he; tqt[x] = i; }
							if (i == tlen_full - 1) { tmte[x] = h; hmte[x] = true; }
							if (h > m) { m = h; tm[x] = h; tmt[x] = i; }
							else if (zdrop >= 0 && m - h > zdrop) fr[x] = true;
							if (!fr[x] && i == tlen_full - 1 && reach) { tsc[x] = he; hsc[x] = true; }
							trows[x] = i + 1;
						}
					}
				}
				fmask |= K2A_FOLD_BALLOT(fr[x], lane0 + x);
			}
			frozen = fmask != 0;
			const int sfirst = frozen ? s0 + (int)__builtin_ctzll(fmask) : nstrips;
			for (int x = 0; x < NL; ++x) {
				const int s = s0 + lane0 + x;
				if (s < nstrips && s <= sfirst) {
					lm[x] = tm[x]; lmt[x] = tmt[x]; lq[x] = tq[x]; lqt[x] = tqt[x];
					if (hmte[x]) { b->mte = tmte[x]; b->mte_q = 0; }
					if (hsc[x]) b->score = tsc[x];
					if (fr[x]) { b->dropped = 1; b->inexact = 1; b->rows = trows[x]; }
				}
			}
		}
		/* the lane-local bests, merged in lane order; ties to the smaller row */
		K2A_FOLD_SYNC();
		for (int x = 0; x < NL; ++x) { const int l = lane0 + x; xi[4 * l] = lm[x]; xi[4 * l + 1] = lmt[x]; xi[4 * l + 2] = lq[x]; xi[4 * l + 3] = lqt[x]; }
		K2A_FOLD_SYNC();
		for (int x = 0; x < NL; ++x) {
			if (lane0 + x == 0 && !dead) {
				int bm = b->max, bmt = b->max_t, bmq = b->max_q, bq = b->mqe, bqt = b->mqe_t;
				bool qlane = false;                                /* bq is a lane's, not the book's own: only then can a smaller row take a tie */
#pragma nounroll
				for (int l = 0; l < 64; ++l) {
					const int vm = xi[4 * l], vmt = xi[4 * l + 1], vq = xi[4 * l + 2], vqt = xi[4 * l + 3];
					/* (a lane's maximum beat the running one strictly where it was set: no two lanes hold the same) */
					if (vm != none && vm > bm) { bm = vm; bmt = vmt; bmq = 0; }
					if (vq != none && (vq > bq || (qlane && vq == bq && vqt < bqt))) { bq = vq; bqt = vqt; qlane = true; }
				}
				b->max = bm; b->max_t = bmt; b->max_q = bmq; b->mqe = bq; b->mqe_t = bqt;
				if (!frozen) b->rows = tlen;
			}
		}
		K2A_FOLD_SYNC();
	}
}

/* The same for the records of a pair-maximum fill (K2aLanePk PM, K2A_PAIR_MAX): [0, C / 2) = the pairs' maxima, as H - q in the bias of
 * the pair's first row; [C, 2C) = hl as above.  A pair (i, i + 1) with maximum P enters with the running maximum m:
 *   - if zdrop >= 0 and max(m, P) - P + slack > zdrop the book is FROZEN in front of row i: dropped = inexact = 1, rows = i + 1, and
 *     nothing of the pair is folded -- the third pass re-folds the freeze row's strip from its first row with the exact test;
 *   - else mqe / score are taken from the rows' hl as above, mte provisionally (P; the second pass writes the row's own maximum), and
 *     if P > m the maximum moves to the pair: max_t = i provisionally, the second pass finds the row (the first of the strip's rows
 *     in front of a freeze whose maximum is `max`) and its column.
 * slack = delta + q (K2aScoring.pk_pm): adjacent rows' maxima differ by at most delta = max(smax + q + e, -smin, q + e) -- the best cell
 * of a row is reached diagonally (the row above holds at least it - smax; from the border column at least it - smax - q - e), from E
 * (at least it + q + e above), and below it lies a cell of at least it - q - e, or, at the band's left edge, diagonally one of at least
 * it + smin -- so BOTH rows of a pair hold at least P - delta; and a border F may have lifted P by up to q (ksw2_lane_pk.h, PM).  So
 * where this fold does not freeze, the per-row test (max - H > zdrop) fires on neither row: every book it leaves unfrozen is the per-row
 * fold's book (max_t, mte aside), and a frozen one is the exact book in front of a row at or before the per-row form's freeze row.
 * tests/stripmax/stripmax_check.cpp checks the bound and both statements against an int32 recurrence. */
template<int C, int NL>
K2A_FN void k2a_pkfold_task_pm(const K2aScoring &sc, const uint32_t *rec, const K2aCkHead *hd, int nstrips, int qlen, int tlen, int tlen_full, int w,
                               int zdropA, int zdropB, int slack, K2aBook *bkA, K2aBook *bkB, uint32_t *xb, int lane0)
{
	constexpr int CP = C / 2;
	const int hq = k2a_hl_q(sc);
	const int none = (int)0x80000000;
	int *xi = (int*)xb;
#pragma nounroll
	for (int half = 0; half < 2; ++half) {
		K2aBook *b = half ? bkB : bkA;
		const int zdrop = half ? zdropB : zdropA, sh = half ? 16 : 0;
		int lm[NL], lmt[NL], lq[NL], lqt[NL];
		for (int x = 0; x < NL; ++x) { lm[x] = lq[x] = none; lmt[x] = lqt[x] = -1; }
		int carry = b->max;
		const bool dead = b->dropped != 0 || nstrips <= 0;
		bool frozen = false;
		K2A_FOLD_SYNC();
#pragma nounroll
		for (int s0 = 0; s0 < nstrips && !dead && !frozen; s0 += 64) {
			int P[NL][CP], hend[NL][C], ent[NL];
			/* 1. the strips' pairs, un-biased; their maxima into the exchange buffer */
			for (int x = 0; x < NL; ++x) {
				const int l = lane0 + x, s = s0 + l;
				int sm = none;
				if (s < nstrips) {
					const uint32_t *r = rec + (size_t)s * K2A_CK_REC_WORDS(C);
					const int base = half ? hd[s].baseB : hd[s].baseA;
					const bool rs = k2a_pkfold_strip_reaches<C>(s, qlen, tlen, w);
#pragma unroll
					for (int p = 0; p < CP; ++p) {
						const int i = s * C + 2 * p;
						P[x][p] = (int)(int16_t)(k2a_ofs_off(r[p]) >> sh) + hq + base - sc.e * i;
						if (i < tlen) sm = k2a_max(sm, P[x][p]);
					}
#pragma unroll
					for (int c = 0; c < C; ++c)
						hend[x][c] = rs ? (int)(int16_t)(k2a_ofs_off(r[C + c]) >> sh) + hq + base - sc.e * (s * C + c) : none;
				}
				xi[l] = sm;
			}
			K2A_FOLD_SYNC();
			/* 2. inclusive prefix maximum over the lanes */
			int src = 0;
#pragma nounroll
			for (int d = 1; d < 64; d <<= 1) {
				for (int x = 0; x < NL; ++x) {
					const int l = lane0 + x;
					int v = xi[src + l];
					if (l >= d) v = k2a_max(v, xi[src + l - d]);
					xi[(src ^ 64) + l] = v;
				}
				K2A_FOLD_SYNC();
				src ^= 64;
			}
			for (int x = 0; x < NL; ++x) { const int l = lane0 + x; ent[x] = l > 0 ? k2a_max(carry, xi[src + l - 1]) : carry; }
			carry = k2a_max(carry, xi[src + 63]);
			K2A_FOLD_SYNC();
			/* 3. the pairs of every strip; 4. the first strip that froze */
			int tm[NL], tmt[NL], tq[NL], tqt[NL], tmte[NL], tsc[NL], trows[NL];
			bool fr[NL], hmte[NL], hsc[NL];
			uint64_t fmask = 0;
			for (int x = 0; x < NL; ++x) {
				const int s = s0 + lane0 + x;
				int m = ent[x];
				tm[x] = lm[x]; tmt[x] = lmt[x]; tq[x] = lq[x]; tqt[x] = lqt[x]; tmte[x] = tsc[x] = trows[x] = 0;
				fr[x] = hmte[x] = hsc[x] = false;
				if (s < nstrips) {
#pragma unroll
					for (int p = 0; p < CP; ++p) {
						const int i0 = s * C + 2 * p, pv = P[x][p];
						if (i0 < tlen && !fr[x]) {
							if (zdrop >= 0 && k2a_max(m, pv) - pv + slack > zdrop) { fr[x] = true; trows[x] = i0 + 1; }
							else {
#pragma unroll
								for (int c = 2 * p; c < 2 * p + 2; ++c) {
									const int i = s * C + c;
									if (i < tlen) {
										const bool reach = i + w >= qlen - 1;
										const int he = hend[x][c];
										if (reach && he > tq[x]) { tq[x] = he; tqt[x] = i; }
										if (i == tlen_full - 1) { tmte[x] = pv; hmte[x] = true; }
										if (i == tlen_full - 1 && reach) { tsc[x] = he; hsc[x] = true; }
										trows[x] = i + 1;
									}
								}
								if (pv > m) { m = pv; tm[x] = pv; tmt[x] = i0; }
							}
						}
					}
				}
				fmask |= K2A_FOLD_BALLOT(fr[x], lane0 + x);
			}
			frozen = fmask != 0;
			const int sfirst = frozen ? s0 + (int)__builtin_ctzll(fmask) : nstrips;
			for (int x = 0; x < NL; ++x) {
				const int s = s0 + lane0 + x;
				if (s < nstrips && s <= sfirst) {
					lm[x] = tm[x]; lmt[x] = tmt[x]; lq[x] = tq[x]; lqt[x] = tqt[x];
					if (hmte[x]) { b->mte = tmte[x]; b->mte_q = 0; }
					if (hsc[x]) b->score = tsc[x];
					if (fr[x]) { b->dropped = 1; b->inexact = 1; b->rows = trows[x]; }
				}
			}
		}
		/* the lane-local bests, merged in lane order; ties to the smaller row */
		K2A_FOLD_SYNC();
		for (int x = 0; x < NL; ++x) { const int l = lane0 + x; xi[4 * l] = lm[x]; xi[4 * l + 1] = lmt[x]; xi[4 * l + 2] = lq[x]; xi[4 * l + 3] = lqt[x]; }
		K2A_FOLD_SYNC();
		for (int x = 0; x < NL; ++x) {
			if (lane0 + x == 0 && !dead) {
				int bm = b->max, bmt = b->max_t, bmq = b->max_q, bq = b->mqe, bqt = b->mqe_t;
				bool qlane = false;
#pragma nounroll
				for (int l = 0; l < 64; ++l) {
					const int vm = xi[4 * l], vmt = xi[4 * l + 1], vq = xi[4 * l + 2], vqt = xi[4 * l + 3];
					if (vm != none && vm > bm) { bm = vm; bmt = vmt; bmq = 0; }
					if (vq != none && (vq > bq || (qlane && vq == bq && vqt < bqt))) { bq = vq; bqt = vqt; qlane = true; }
				}
				b->max = bm; b->max_t = bmt; b->max_q = bmq; b->mqe = bq; b->mqe_t = bqt;
				if (!frozen) b->rows = tlen;
			}
		}
		K2A_FOLD_SYNC();
	}
}

#endif
