/*
 * stripfold_check.cpp -- host check of the deferred fills' strip-end fold (ksw2_lane_pkfold.h: k2a_pkfold_task) against
 * K2aLanePk::do_fin_seq (its DEFER branch) called on the same strips one by one, in order.
 *
 * The fold's text runs here with NL = 64: its per-lane loops are the wavefront, its exchange buffer an array of exactly
 * K2A_PKFOLD_XB_WORDS words.  Records and headers are synthetic: a case states the true row maxima H and last-column values of both
 * alignment halves and the per-strip, per-half bases, and the records are formed from them as the lanes' registers would hold them
 * (offset form, row bias e * i, relative to the base, the H column less q in the open form).  Compared: every field of both books.
 *
 * Every case is folded twice: from buffers of exactly nstrips records and headers (the address sanitizer sees a read behind them),
 * and from buffers with 70 more records and headers behind, filled with values that would win (the recycled blocks of other plans).
 * Rows behind tlen in a partial last strip hold such values as well.
 *
 * Directed cases state what they are about as an expectation on the reference's book (a case that is not reached fails): ties of the
 * maximum inside a strip, between strips of one round and of two rounds; freezes at the first and the last row of a strip, in lane
 * 0, in lane 63, in the strips just behind a round boundary (63 -> 64, 127 -> 128), in a strip whose earlier row raised the maximum,
 * on a reach row (mqe first, no score); halves frozen at different rows, one half only; zdrop = -1; 1, 63, 64, 65, 129 strips; a
 * partial last strip; tlen < tlen_full; mqe ties inside a strip, between strips and between rounds; bases that differ per strip and
 * half, negative ones included (every case).  Then randomized cases from a fixed seed.  C = 8 and C = 16.
 *
 * A stand-alone program: g++ -O1 -fsanitize=address,undefined -I ksw2_amd/csrc tests/stripfold/stripfold_check.cpp && ./a.out
 * returns 0 when every check held.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "ksw2_lane_pkfold.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
	return (uint32_t)(g_rng >> 32);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++g_fail; } } while (0)

static const int WIN_H = 3000;      /* what stale records and rows behind tlen claim: above every case's values */
static const int STALE = 70;        /* records and headers behind nstrips in the padded run: more than a round */

template<int C>
struct Task {
	std::string name;
	int nstrips, tlen, tlen_full, qlen, w, zd[2];
	std::vector<int> base[2];        /* per strip */
	std::vector<int> H[2], HE[2];    /* per row: the row's maximum, its H at the last column (read on reach rows only) */

	Task(const char *nm, int ns, int cut = 0, int more = 0, int reachrows = 5)
	{
		name = nm; nstrips = ns; tlen = ns * C - cut; tlen_full = tlen + more;
		qlen = tlen_full; w = reachrows - 1;                 /* row i reaches iff i + w >= qlen - 1: the last `reachrows` rows of the full target */
		zd[0] = zd[1] = 50;
		for (int h = 0; h < 2; ++h) {
			base[h].resize(ns); H[h].assign(ns * C, 100); HE[h].assign(ns * C, 90);
			for (int s = 0; s < ns; ++s) base[h][s] = rnd_in(-2000, 2000);
		}
	}
	int row(int s, int c) const { return s * C + c; }
	bool reach(int i) const { return i + w >= qlen - 1; }
};

static K2aScoring scoring()
{
	K2aScoring sc;
	memset(&sc, 0, sizeof(sc));
	sc.q = 4; sc.e = 2; sc.m = 5; sc.pk_smax = 2;
	return sc;
}

static uint32_t half16(int plain)
{
	if (plain < K2A_NEG16 || plain > K2A_PK_VMAX) { printf("FAIL: a case's value %d does not fit the packed range\n", plain); ++g_fail; plain = 0; }
	return (uint32_t)(plain + K2A_OFS16) & 0xffffu;
}

/* the records and headers of a task, `extra` stale ones behind them */
template<int C>
static void build(const K2aScoring &sc, const Task<C> &t, int extra, std::vector<uint32_t> &rec, std::vector<K2aCkHead> &hd)
{
	const int hq = k2a_hl_q(sc), n = t.nstrips + extra;
	rec.assign((size_t)n * K2A_CK_REC_WORDS(C), 0);
	hd.resize(n);
	for (int s = 0; s < n; ++s) {
		const bool stale = s >= t.nstrips;
		const int bA = stale ? 1000 : t.base[0][s], bB = stale ? 1000 : t.base[1][s];
		hd[s].baseA = bA; hd[s].baseB = bB; hd[s].hd0 = 0xdeadbeefu; hd[s].pad = 0;
		for (int c = 0; c < C; ++c) {
			const int i = s * C + c;
			const bool real = !stale && i < t.tlen;
			const int hA = real ? t.H[0][i] : WIN_H, hB = real ? t.H[1][i] : WIN_H;
			/* the H column of a strip without a reach row is not part of its record: whatever lay there before */
			const bool rs = !stale && k2a_pkfold_strip_reaches<C>(s, t.qlen, t.tlen, t.w);
			const int eA = real && rs ? t.HE[0][i] : WIN_H, eB = real && rs ? t.HE[1][i] : WIN_H;
			rec[(size_t)s * K2A_CK_REC_WORDS(C) + c] = half16(hA - bA + sc.e * i) | (half16(hB - bB + sc.e * i) << 16);
			rec[(size_t)s * K2A_CK_REC_WORDS(C) + C + c] = half16(eA - hq - bA + sc.e * i) | (half16(eB - hq - bB + sc.e * i) << 16);
		}
	}
}

/* K2aLanePk::do_fin_seq, DEFER branch, strip by strip */
template<int C>
static void reference(const K2aScoring &sc, const Task<C> &t, const std::vector<uint32_t> &rec, const std::vector<K2aCkHead> &hd, K2aBook *bA, K2aBook *bB)
{
	typedef K2aLanePk<64, C, false, K2A_MODE_SCORE, true, false, 0, true, false> Lane;
	static Lane L;
	k2a_book_reset(bA); k2a_book_reset(bB);
	for (int s = 0; s < t.nstrips; ++s) {
		uint32_t rowbuf[K2A_PK_STAGE(C)];
		L.i0 = s * C; L.tlen = t.tlen; L.tlen_full = t.tlen_full; L.w = t.w; L.qlen = t.qlen;
		L.baseA = hd[s].baseA; L.baseB = hd[s].baseB;
		for (int c = 0; c < C; ++c) {
			rowbuf[c] = k2a_ofs_off(rec[(size_t)s * K2A_CK_REC_WORDS(C) + C + c]);
			rowbuf[C + c] = k2a_ofs_off(rec[(size_t)s * K2A_CK_REC_WORDS(C) + c]);
			rowbuf[2 * C + c] = 0;                             /* the deferred lanes have no arg-max columns (rmj) */
		}
		L.do_fin_seq(sc, bA, bB, t.zd[0], t.zd[1], rowbuf);
	}
}

static bool same_book(const K2aBook &a, const K2aBook &b)
{
	return a.max == b.max && a.max_t == b.max_t && a.max_q == b.max_q && a.mqe == b.mqe && a.mqe_t == b.mqe_t && a.mte == b.mte && a.mte_q == b.mte_q &&
	       a.score == b.score && a.dropped == b.dropped && a.rows == b.rows && a.inexact == b.inexact;
}
static void print_book(const char *who, const K2aBook &b)
{
	printf("  %s: max %d max_t %d max_q %d mqe %d mqe_t %d mte %d mte_q %d score %d dropped %d rows %d inexact %d\n", who, b.max, b.max_t, b.max_q, b.mqe,
	       b.mqe_t, b.mte, b.mte_q, b.score, b.dropped, b.rows, b.inexact);
}

/* folds the task both ways, compares with the reference; returns the reference's books for the case's own expectations */
template<int C>
static void run(const Task<C> &t, K2aBook ref[2])
{
	const K2aScoring sc = scoring();
	for (int pass = 0; pass < 2; ++pass) {
		std::vector<uint32_t> rec;
		std::vector<K2aCkHead> hd;
		build<C>(sc, t, pass ? STALE : 0, rec, hd);
		if (pass == 0) reference<C>(sc, t, rec, hd, &ref[0], &ref[1]);
		std::vector<uint32_t> xb(K2A_PKFOLD_XB_WORDS, 0xa5a5a5a5u);
		K2aBook got[2];
		k2a_book_reset(&got[0]); k2a_book_reset(&got[1]);
		k2a_pkfold_task<C, 64>(sc, rec.data(), hd.data(), t.nstrips, t.qlen, t.tlen, t.tlen_full, t.w, t.zd[0], t.zd[1], &got[0], &got[1], xb.data(), 0);
		for (int h = 0; h < 2; ++h)
			if (!same_book(got[h], ref[h])) {
				printf("FAIL C=%d %s (%s buffers) half %d: nstrips %d tlen %d tlen_full %d w %d zdrop %d\n", C, t.name.c_str(), pass ? "padded" : "exact", h,
				       t.nstrips, t.tlen, t.tlen_full, t.w, t.zd[h]);
				print_book("fold     ", got[h]); print_book("reference", ref[h]);
				++g_fail;
			}
	}
}

template<int C>
static int directed()
{
	int n = 0;
	K2aBook r[2];
#define RUN(t) do { run<C>(t, r); ++n; } while (0)
	/* sizes; nothing special: the flat task's maximum is its first row, no freeze, the last row gives mte and score */
	const int sizes[] = { 1, 63, 64, 65, 129 };
	for (int ns : sizes) {
		Task<C> t("size", ns);
		RUN(t);
		for (int h = 0; h < 2; ++h)
			CHECK(r[h].max == 100 && r[h].max_t == 0 && r[h].max_q == 0 && !r[h].dropped && r[h].rows == ns * C && r[h].mte == 100 && r[h].mte_q == 0 &&
			      r[h].score == 90 && r[h].mqe == 90 && r[h].mqe_t == k2a_max(0, ns * C - 5), "C=%d size %d half %d not as stated", C, ns, h);
	}
	{	/* maximum tied between two rows of one strip */
		Task<C> t("tie-strip", 65);
		t.zd[0] = t.zd[1] = 1000;                               /* (the test is on, and the fall behind the peak does not fire it) */
		for (int h = 0; h < 2; ++h) t.H[h][t.row(2, 1)] = t.H[h][t.row(2, 3)] = 500;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 500 && r[h].max_t == t.row(2, 1) && !r[h].dropped, "C=%d tie-strip", C);
	}
	{	/* ... between two strips of one round */
		Task<C> t("tie-round", 65);
		t.zd[0] = t.zd[1] = 1000;
		for (int h = 0; h < 2; ++h) t.H[h][t.row(3, 2)] = t.H[h][t.row(10, 0)] = 500;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 500 && r[h].max_t == t.row(3, 2) && !r[h].dropped, "C=%d tie-round", C);
	}
	{	/* ... between strips of different rounds; the later one in a lower lane */
		Task<C> t("tie-rounds", 129);
		t.zd[0] = t.zd[1] = 1000;
		for (int h = 0; h < 2; ++h) t.H[h][t.row(5, 1)] = t.H[h][t.row(64 + 2, 0)] = t.H[h][t.row(128, 3)] = 500;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 500 && r[h].max_t == t.row(5, 1) && !r[h].dropped && r[h].rows == t.tlen, "C=%d tie-rounds", C);
	}
	{	/* freezes: first / last row of a strip; lane 0 (strips 0, 64, 128: just behind a round boundary), lane 63 (63, 127) */
		const int at[][2] = { { 7, 0 }, { 7, C - 1 }, { 0, 2 }, { 64, 0 }, { 64, C - 1 }, { 128, 0 }, { 128, 1 }, { 63, 0 }, { 63, C - 1 }, { 127, C - 1 }, { 127, 0 }, { 65, 1 } };
		for (const auto &a : at) {
			Task<C> t("freeze", 129);
			for (int h = 0; h < 2; ++h) t.H[h][t.row(a[0], a[1])] = 49;          /* 100 - 49 > 50 */
			RUN(t);
			for (int h = 0; h < 2; ++h)
				CHECK(r[h].dropped == 1 && r[h].inexact == 1 && r[h].rows == t.row(a[0], a[1]) + 1 && r[h].max == 100 && r[h].max_t == 0 && r[h].mte == K2A_NEG &&
				      r[h].score == K2A_NEG && r[h].mqe == K2A_NEG, "C=%d freeze at strip %d row %d", C, a[0], a[1]);
		}
	}
	{	/* the row in front of a freeze is not one: 100 - 50 = zdrop exactly */
		Task<C> t("no-freeze-at-zdrop", 65);
		for (int h = 0; h < 2; ++h) t.H[h][t.row(64, 0)] = 50;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(!r[h].dropped && r[h].rows == t.tlen, "C=%d no-freeze-at-zdrop", C);
	}
	{	/* freeze in a strip in which an earlier row raised the maximum: 249 would pass against the 100 the strip is entered with */
		Task<C> t("freeze-raised", 129);
		for (int h = 0; h < 2; ++h) { t.H[h][t.row(70, 1)] = 300; t.H[h][t.row(70, 2)] = 260; t.H[h][t.row(70, 3)] = 255; t.H[h][t.row(70, 4)] = 249; }
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].dropped == 1 && r[h].rows == t.row(70, 4) + 1 && r[h].max == 300 && r[h].max_t == t.row(70, 1), "C=%d freeze-raised", C);
	}
	{	/* ... and the maxima of strips behind a freeze do not count, in the same round or a later one */
		Task<C> t("freeze-then-max", 129);
		for (int h = 0; h < 2; ++h) { t.H[h][t.row(20, 3)] = 49; t.H[h][t.row(21, 0)] = 700; t.H[h][t.row(100, 0)] = 800; }
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].dropped == 1 && r[h].rows == t.row(20, 3) + 1 && r[h].max == 100 && r[h].max_t == 0, "C=%d freeze-then-max", C);
	}
	{	/* freeze on a reach row -- the last row: mqe takes the row first, score does not, mte does */
		Task<C> t("freeze-reach", 65);
		const int last = t.tlen - 1;
		for (int h = 0; h < 2; ++h) { t.H[h][last] = 49; t.HE[h][last] = 95; }
		RUN(t);
		for (int h = 0; h < 2; ++h)
			CHECK(r[h].dropped == 1 && r[h].rows == t.tlen && r[h].mqe == 95 && r[h].mqe_t == last && r[h].score == K2A_NEG && r[h].mte == 49, "C=%d freeze-reach", C);
	}
	{	/* the halves frozen at different rows, of different rounds */
		Task<C> t("freeze-halves", 129);
		t.H[0][t.row(4, 1)] = 49; t.H[1][t.row(70, 3)] = 49;
		RUN(t);
		CHECK(r[0].dropped == 1 && r[0].rows == t.row(4, 1) + 1 && r[1].dropped == 1 && r[1].rows == t.row(70, 3) + 1, "C=%d freeze-halves", C);
	}
	{	/* ... of one round, the higher half first */
		Task<C> t("freeze-halves-round", 65);
		t.H[1][t.row(4, 1)] = 49; t.H[0][t.row(40, 3)] = 49; t.H[1][t.row(30, 0)] = 900;
		RUN(t);
		CHECK(r[1].dropped == 1 && r[1].rows == t.row(4, 1) + 1 && r[1].max == 100 && r[0].dropped == 1 && r[0].rows == t.row(40, 3) + 1, "C=%d freeze-halves-round", C);
	}
	for (int fh = 0; fh < 2; ++fh) {	/* one half frozen, the other not */
		Task<C> t("freeze-one-half", 129);
		t.zd[!fh] = 1000;
		t.H[fh][t.row(66, 2)] = 49; t.H[!fh][t.row(90, 2)] = 400;
		RUN(t);
		CHECK(r[fh].dropped == 1 && r[fh].rows == t.row(66, 2) + 1 && !r[!fh].dropped && r[!fh].rows == t.tlen && r[!fh].max == 400 && r[!fh].max_t == t.row(90, 2) &&
		      r[!fh].score == 90, "C=%d freeze-one-half %d", C, fh);
	}
	{	/* zdrop = -1: nothing freezes, whatever the rows do; one half only */
		Task<C> t("zdrop-off", 65);
		t.zd[0] = -1;
		for (int h = 0; h < 2; ++h) t.H[h][t.row(9, 2)] = -400;
		RUN(t);
		CHECK(!r[0].dropped && r[0].rows == t.tlen && r[0].score == 90 && r[1].dropped == 1 && r[1].rows == t.row(9, 2) + 1, "C=%d zdrop-off", C);
	}
	{	/* no row above 0: the book's maximum stays where the reset put it, and the first row that lies zdrop below 0 freezes it */
		Task<C> t("never-positive", 8);
		for (int h = 0; h < 2; ++h) for (int i = 0; i < t.tlen; ++i) t.H[h][i] = -10 - i;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 0 && r[h].max_t == -1 && r[h].max_q == -1 && r[h].dropped == 1 && r[h].rows == 42, "C=%d never-positive", C);
	}
	{	/* a partial last strip: the rows behind tlen hold winners */
		Task<C> t("partial", 65, 3);
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 100 && r[h].rows == 65 * C - 3 && r[h].mte == 100 && r[h].score == 90 && r[h].mqe_t == 65 * C - 3 - 5, "C=%d partial", C);
		Task<C> u("partial-one-row", 129, C - 1);
		RUN(u);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 100 && r[h].rows == 128 * C + 1 && r[h].mte == 100 && r[h].score == 90, "C=%d partial-one-row", C);
	}
	{	/* tlen < tlen_full: the fill stops short of the last target row: no mte, no score; reach rows there may be */
		Task<C> t("short", 65, 2, 3, 6);
		RUN(t);
		for (int h = 0; h < 2; ++h)
			CHECK(r[h].mte == K2A_NEG && r[h].mte_q == -1 && r[h].score == K2A_NEG && r[h].rows == t.tlen && r[h].mqe == 90 && r[h].mqe_t == t.tlen_full - 6 && !r[h].dropped, "C=%d short", C);
	}
	{	/* mqe ties: inside a strip, between strips of a round, between rounds (reach rows over 70 strips) -- the first row wins */
		Task<C> t("mqe-tie-strip", 65, 0, 0, C);
		for (int h = 0; h < 2; ++h) t.HE[h][t.row(64, 2)] = t.HE[h][t.row(64, 5)] = 95;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].mqe == 95 && r[h].mqe_t == t.row(64, 2), "C=%d mqe-tie-strip", C);
		Task<C> u("mqe-tie-rounds", 129, 0, 0, 70 * C);
		for (int h = 0; h < 2; ++h) u.HE[h][u.row(62, 1)] = u.HE[h][u.row(63, 0)] = u.HE[h][u.row(66, 0)] = u.HE[h][u.row(128, 0)] = 95;
		RUN(u);
		for (int h = 0; h < 2; ++h) CHECK(r[h].mqe == 95 && r[h].mqe_t == u.row(62, 1) && u.reach(u.row(62, 1)) && !u.reach(u.row(58, 0)), "C=%d mqe-tie-rounds", C);
		Task<C> v("mqe-later-lower-lane", 129, 0, 0, 70 * C);      /* the winner of a later round sits in a lower lane than an earlier tie */
		for (int h = 0; h < 2; ++h) { v.HE[h][v.row(63, 0)] = 95; v.HE[h][v.row(64, 0)] = 95; v.HE[h][v.row(65, 0)] = 96; v.HE[h][v.row(127, 0)] = 96; }
		RUN(v);
		for (int h = 0; h < 2; ++h) CHECK(r[h].mqe == 96 && r[h].mqe_t == v.row(65, 0), "C=%d mqe-later-lower-lane", C);
	}
	{	/* bases: every case has its own per strip and half; here the extremes, with the same true scores */
		Task<C> t("bases", 129);
		t.zd[0] = t.zd[1] = 1000;
		for (int s = 0; s < t.nstrips; ++s) { t.base[0][s] = (s & 1) ? -4000 : 2500; t.base[1][s] = (s & 1) ? 2500 : -4000; }
		for (int h = 0; h < 2; ++h) t.H[h][t.row(77, 7)] = 640;
		RUN(t);
		for (int h = 0; h < 2; ++h) CHECK(r[h].max == 640 && r[h].max_t == t.row(77, 7) && !r[h].dropped && r[h].score == 90, "C=%d bases", C);
	}
#undef RUN
	return n;
}

template<int C>
static int randomized(int cases)
{
	K2aBook r[2];
	int frozen = 0;
	for (int k = 0; k < cases; ++k) {
		const int ns = (k % 7 == 0) ? rnd_in(1, 3) : rnd_in(1, 140);
		const int cut = rnd_in(0, 2) ? 0 : rnd_in(0, C - 1), more = rnd_in(0, 3) ? 0 : rnd_in(1, 40);
		const int reachrows = rnd_in(0, 3) ? rnd_in(1, 2 * C) : rnd_in(1, 80 * C);
		Task<C> t("random", ns, cut, more, reachrows);
		for (int h = 0; h < 2; ++h) {
			t.zd[h] = rnd_in(0, 4) ? rnd_in(0, 300) : -1;
			/* a walk with few distinct values, so that ties are common, and now and then a fall */
			int v = rnd_in(-50, 200);
			const int step = rnd_in(1, 40), fall = rnd_in(0, 2) ? rnd_in(50, 400) : 0, fallat = rnd_in(0, ns * C - 1);
			for (int i = 0; i < ns * C; ++i) {
				v += (rnd_in(0, 2) - 1) * step;
				v = k2a_min(k2a_max(v, -400), 1500);
				t.H[h][i] = i == fallat ? v - fall : v;
				t.HE[h][i] = t.H[h][i] - rnd_in(0, 3) * step;
			}
		}
		run<C>(t, r);
		frozen += r[0].dropped + r[1].dropped;
	}
	CHECK(frozen > cases / 10 && frozen < 2 * cases - cases / 10, "C=%d: %d of %d random books frozen: the cases do not cover both outcomes", C, frozen, 2 * cases);
	return cases;
}

int main()
{
	const int d8 = directed<8>(), d16 = directed<16>();
	const int r8 = randomized<8>(1500), r16 = randomized<16>(1500);
	printf("C=8: %d directed, %d random cases\nC=16: %d directed, %d random cases\n", d8, r8, d16, r16);
	if (g_fail) { printf("stripfold check FAILED: %d\n", g_fail); return 1; }
	printf("stripfold check ok\n");
	return 0;
}
