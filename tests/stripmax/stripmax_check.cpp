/*
 * stripmax_check.cpp -- host check of the deferred fills' pair-maximum form (K2aLanePk PM, ksw2_lane_pk.h; the fold
 * k2a_pkfold_task_pm, ksw2_lane_pkfold.h) against the per-row form and against a plain int32 recurrence written here.
 *
 * Two groups of 64 lanes -- K2aLanePk<64, C, .., DEFER> with one running maximum per row, and the same with PM: one per pair of rows --
 * run whole alignments in lock step through the loop of k2a_fill_pk_body (ksw2_shim_hip.hip; same order of events), two alignments of
 * one shape per lane, and store a record per strip as the kernel does.  The recurrence is the textbook affine one with the
 * reference's borders on the band |i - j| <= w; it knows nothing of row bias, bases, offset form, or F registers.  Checked:
 *   (a) every pair's maximum, un-biased, is the larger of its rows' maxima in the recurrence over i < tlen (and the per-row form's
 *       rmax[c] are those) -- but for an odd row that starts at column 0, whose border F may stand in: then the pair's value is at most
 *       q above the true one and stands for a negative H;
 *   (b) |M_i - M_(i+1)| <= delta = max(smax + q + e, -smin, q + e) for every adjacent row pair of the recurrence; the cases hold
 *       rows whose best cell lies at column 0, on the left and on the right band edge (counted, and required);
 *   (c) for a set of Z-drop thresholds: where neither fold freezes, k2a_pkfold_task_pm's book is K2aLanePk::do_fin_seq's on the
 *       per-row strips in order, field for field -- max_t names the pair's first row and mte the pair's maximum, and what the second
 *       pass does with them (first row of the strip, in front of a freeze, whose own maximum is the book's; the last row's own
 *       maximum) gives the reference's;
 *   (d) where the new fold freezes, its freeze row is at or before the per-row form's, and the book is the exact book in front of
 *       that row (folded here from the recurrence);
 *   (e) where the per-row form freezes, the new one has frozen too.
 * Cases: C = 16 with targets of 1 025 and 2 053 rows, C = 8 with 513 and 1 029, a partial last strip, qlen + w < tlen; bands 0, C,
 * C + 1 and the widest the geometry admits; plain and re-based; similar reads, reads with random tails that leave in the first, a
 * middle and the last strip, reads shifted onto either band edge, reads that match nothing, a maximum that is reached again two rows
 * on and a strip on, target and query wildcards (the TN build); the 2 / -4 preset, a transition / transversion matrix, and mismatch -7
 * (profile bytes short of pk_base).
 *
 * A stand-alone program: g++ -O1 -fsanitize=address,undefined -I ksw2_amd/csrc tests/stripmax/stripmax_check.cpp && ./a.out
 * returns 0 when every check held.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "ksw2_lane_pkfold.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
	return (uint32_t)(g_rng >> 32);
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 40) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++g_fail; } } while (0)

enum { NEGI = -(1 << 28) };
static inline int imax2(int a, int b) { return a > b ? a : b; }
static inline int imin2(int a, int b) { return a < b ? a : b; }

/* a scoring as the host builds it (ksw2_host_plan.c::pk_scoring) from a 5 x 5 matrix mat[t * 5 + q]; target wildcard rows on */
struct Scoring {
	K2aScoring sc;
	int8_t mat[25];
	int smax, smin, delta;
};
static Scoring scoring(int match, int ts, int tv, int wild, int q, int e)
{
	Scoring s;
	memset(&s, 0, sizeof(s));
	for (int t = 0; t < 5; ++t)
		for (int c = 0; c < 5; ++c)
			s.mat[t * 5 + c] = (int8_t)((t == 4 || c == 4) ? wild : t == c ? match : ((t ^ c) == 2) ? ts : tv);      /* 0 <-> 2, 1 <-> 3: transitions */
	s.smax = s.smin = s.mat[0];
	for (int x = 0; x < 25; ++x) { s.smax = imax2(s.smax, s.mat[x]); s.smin = imin2(s.smin, s.mat[x]); }
	K2aScoring &sc = s.sc;
	sc.q = q; sc.e = e; sc.m = 5; sc.pk_smax = s.smax;
	int lo = 1 << 30, hi = -(1 << 30);
	for (int c = 0; c < 5; ++c)
		for (int t = 0; t < 4; ++t) { const int v = q + e + s.mat[t * 5 + c]; lo = imin2(lo, v); hi = imax2(hi, v); }
	sc.pk_base = lo < 0 ? lo : hi > 255 ? hi - 255 : 0;
	for (int c = 0; c < 5; ++c)
		for (int t = 0; t < 4; ++t) sc.cp[c] |= (uint32_t)(q + e + s.mat[t * 5 + c] - sc.pk_base) << (8 * t);
	sc.pk_tn1 = s.smax - wild + 1; sc.pk_tnc = q + e + wild - sc.pk_base;
	s.delta = imax2(imax2(s.smax + q + e, -s.smin), q + e);
	sc.pk_pm = s.delta + q;
	return s;
}

/* the recurrence: per row its maximum, the first column that holds it, and its H at the last column where the row reaches it */
struct Scalar { std::vector<int> rmax, rcol, hend; };
static void scalar_fill(const Scoring &s, const uint8_t *q, const uint8_t *t, int qlen, int tlen, int w, Scalar &o)
{
	const K2aScoring &sc = s.sc;
	std::vector<int> Hp(qlen, NEGI), Ep(qlen, NEGI), Hc(qlen, NEGI), Ec(qlen, NEGI);
	o.rmax.assign(tlen, NEGI); o.rcol.assign(tlen, -1); o.hend.assign(tlen, NEGI);
	for (int i = 0; i < tlen; ++i) {
		const int jlo = imax2(0, i - w), jhi = imin2(i + w, qlen - 1);
		int F = NEGI, Hleft = NEGI;
		for (int j = jlo; j <= jhi; ++j) {
			const int diag = i == 0 ? k2a_border<false>(sc, j) : j == 0 ? k2a_border<false>(sc, i) : Hp[j - 1];
			int E;
			if (i == 0) E = k2a_border<false>(sc, j + 1) - (sc.q + sc.e);
			else if (j - (i - 1) <= w) E = imax2(Ep[j], Hp[j] - sc.q) - sc.e;
			else E = NEGI;
			if (j == 0) F = k2a_border<false>(sc, i + 1) - (sc.q + sc.e);
			else if (i - (j - 1) <= w) F = imax2(F, Hleft - sc.q) - sc.e;
			else F = NEGI;
			const int H = imax2(imax2(diag + s.mat[t[i] * 5 + q[j]], E), F);
			Hc[j] = H; Ec[j] = E; Hleft = H;
			if (H > o.rmax[i]) { o.rmax[i] = H; o.rcol[i] = j; }
			if (j == qlen - 1) o.hend[i] = H;
		}
		Hp.swap(Hc); Ep.swap(Ec);
	}
}

struct Shape { int qlen, tlen_full, w; };
/* what the two halves' reads look like */
enum Kind { SIMILAR, TAIL_FIRST, TAIL_MID, TAIL_LAST, EDGE_LEFT, EDGE_RIGHT, NOTHING, AGAIN, WILD, NKIND };

static void make_pair(Kind kind, const Shape &s, int C, bool wild_ok, std::vector<uint8_t> &q, std::vector<uint8_t> &t)
{
	const int ql = s.qlen, tl = s.tlen_full;
	t.resize(tl); q.resize(ql);
	for (int x = 0; x < tl; ++x) t[x] = (uint8_t)(rnd() & 3);
	const int shift = kind == EDGE_LEFT ? s.w : kind == EDGE_RIGHT ? -s.w : 0;       /* q[j] = t[j + shift]: the diagonal j = i - shift */
	for (int j = 0; j < ql; ++j) {
		const int i = j + shift;
		q[j] = (i >= 0 && i < tl && rnd() % 100 >= 4) ? t[i] : (uint8_t)(rnd() & 3);
	}
	if (kind == TAIL_FIRST || kind == TAIL_MID || kind == TAIL_LAST) {
		const int at = kind == TAIL_FIRST ? imin2(C / 2, ql - 1) : kind == TAIL_MID ? ql / 2 : imax2(0, imin2(ql, tl) - C - C / 2);
		for (int j = at; j < ql; ++j) q[j] = (uint8_t)(rnd() & 3);
	}
	if (kind == NOTHING) { for (int x = 0; x < tl; ++x) t[x] = (uint8_t)(x & 1 ? 0 : 2); for (int j = 0; j < ql; ++j) q[j] = (uint8_t)(j % 3 == 0 ? 3 : 1); }
	if (kind == AGAIN) {
		/* clean matches up to a best cell, then per block: a mismatch and two matches (the maximum is reached again two rows on),
		 * and the same one strip later; random behind */
		const int n = imin2(ql, tl), peak = imin2(n - 1, 5 * C + 3);
		for (int j = 0; j < n; ++j) q[j] = t[j];
		for (int b = 0; b < 2 && peak + b * C + 3 < n; ++b) { const int x = peak + b * C + 1; q[x] = (uint8_t)((t[x] + 1) & 3); }
		for (int j = peak + C + 4; j < ql; ++j) q[j] = (uint8_t)(rnd() & 3);
	}
	if (kind == WILD && wild_ok) {
		for (int x = 0; x < tl; ++x) if (rnd() % 40 == 0) t[x] = 4;
		for (int j = 0; j < ql; ++j) if (rnd() % 40 == 0) q[j] = 4;
	}
}

static long g_cases, g_pairs, g_border_pairs, g_col0, g_left, g_right, g_books, g_frozen_new, g_frozen_ref, g_frozen_early, g_resolved;

template<int C, bool PM, bool RB, bool TN>
struct Group {
	typedef K2aLanePk<64, C, false, K2A_MODE_SCORE, RB, false, 0, true, TN, PM> Lane;
	std::vector<Lane> L;
	std::vector<uint32_t> rec;
	std::vector<K2aCkHead> hd;
	std::vector<uint32_t> qpa, qpb;
	std::vector<k2a_pk> hin, ein;
	std::vector<int> bsA, bsB;
	void run(const K2aScoring &sc, const K2aPair pr[2], const uint8_t *seq)
	{
		const int G = 64;
		L.resize(G); qpa.resize(G); qpb.resize(G); hin.resize(G); ein.resize(G); bsA.resize(G); bsB.resize(G);
		for (int l = 0; l < G; ++l) {
			L[l].lrow = 0;
			L[l].setup(pr[0], pr[1], seq, l, true, sc.cp);
			L[l].load_query_group(0, L[l].knext == 0 ? L[l].koff_next : L[l].koff, L[l].qwA, L[l].qwB);
		}
		const int ns = L[0].nstrips, tlen = pr[0].tlen;
		rec.assign((size_t)ns * K2A_CK_REC_WORDS(C), 0xffffffffu);      /* what no lane stored stays a value that would win */
		hd.resize(ns);
		const int kmax = L[0].last_step();
		const int ktop = k2a_min(pr[0].qlen - 1, k2a_min(C - 1, tlen - 1) + pr[0].w);
		for (int k = 0; k <= kmax; ++k) {
			for (int l = 0; l < G; ++l) {
				const int src = (l + G - 1) % G;
				hin[l] = L[src].hout; ein[l] = L[src].eout; bsA[l] = L[src].baseA; bsB[l] = L[src].baseB;
			}
			for (int l = 0; l < G; ++l) {
				if (L[l].need_init(k)) {
					L[l].do_init(sc, RB ? bsA[l] : 0, RB ? bsB[l] : 0);
					if (k & 3) L[l].reload_query_group(k);
					K2aCkHead h; h.baseA = L[l].baseA; h.baseB = L[l].baseB; h.hd0 = L[l].hd0; h.pad = 0; hd[L[l].S] = h;
				}
				L[l].hu_prev = hin[l];
				if (RB) { hin[l] = k2a_pk_add(hin[l], L[l].delta); ein[l] = k2a_pk_add(ein[l], L[l].delta); }
				if ((k & 3) == 0) L[l].load_query_group(k + 4, L[l].knext <= k + 4 ? L[l].koff_next : L[l].koff, qpa[l], qpb[l]);
				L[l].set_qb(Lane::query_pick(L[l].qwA, L[l].qwB, k & 3));
				k2a_pk e2 = 0;
				if (k <= ktop) L[l].top_inputs(sc, k, hin[l], ein[l], e2);
			}
			bool wn = false;                                                   /* K2A_SYNC_WN */
			for (int l = 0; l < G; ++l) wn |= L[l].hasn != 0;
			for (int l = 0; l < G; ++l) L[l].wn = wn;
			for (int l = 0; l < G; ++l) { uint32_t tw[Lane::TBWORDS + 1]; L[l].step(sc, k, hin[l], ein[l], 0u, tw); }
			for (int l = 0; l < G; ++l) {
				if (!L[l].need_fin(k)) continue;
				uint32_t *r = &rec[(size_t)L[l].S * K2A_CK_REC_WORDS(C)];          /* the record, as k2a_fill_pk_body stores it */
				if (PM) { for (int p = 0; p < C / 2; ++p) r[p] = L[l].rmax(2 * p); }
				else for (int c = 0; c < C; ++c) r[c] = L[l].rmax(c);
				if (k2a_pkfold_strip_reaches<C>(L[l].S, L[l].qlen, L[l].tlen, L[l].w)) for (int c = 0; c < C; ++c) r[C + c] = L[l].hl[c];
				L[l].end_strip();
			}
			if ((k & 3) == 3)
				for (int l = 0; l < G; ++l) { L[l].qwA = qpa[l]; L[l].qwB = qpb[l]; }
		}
	}
};

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

template<int C, bool RB, bool TN>
static void run_case(const Scoring &s, const Shape &sh, Kind kA, Kind kB)
{
	const K2aScoring &sc = s.sc;
	K2aPair pr[2];
	std::vector<uint8_t> seq;
	for (int h = 0; h < 2; ++h) {
		std::vector<uint8_t> q, t;
		make_pair(h ? kB : kA, sh, C, TN, q, t);
		K2aPair &p = pr[h];
		memset(&p, 0, sizeof(p));
		p.qlen = sh.qlen; p.tlen_full = sh.tlen_full; p.w = sh.w;
		p.tlen = imin2(sh.qlen + sh.w, sh.tlen_full);                            /* rows that own an in-band cell */
		p.zdrop = -1;
		p.qoff = (uint32_t)seq.size(); seq.insert(seq.end(), q.begin(), q.end()); seq.resize(seq.size() + 8, 0);
		p.toff = (uint32_t)seq.size(); seq.insert(seq.end(), t.begin(), t.end()); seq.resize(seq.size() + C + 8, 0);
	}
	seq.resize(seq.size() + 64, 0);
	const int tlen = pr[0].tlen, tlen_full = sh.tlen_full, qlen = sh.qlen, w = sh.w, ns = (tlen + C - 1) / C, hq = k2a_hl_q(sc);
	Scalar ref[2];
	for (int h = 0; h < 2; ++h) scalar_fill(s, seq.data() + pr[h].qoff, seq.data() + pr[h].toff, qlen, tlen, w, ref[h]);

	static Group<C, false, RB, TN> R;
	static Group<C, true, RB, TN> P;
	R.run(sc, pr, seq.data());
	P.run(sc, pr, seq.data());
	++g_cases;

	/* (a), (b) */
	for (int h = 0; h < 2; ++h) {
		const int shf = h ? 16 : 0;
		for (int i = 0; i < tlen; ++i) {
			const int st = i / C, c = i % C, base = h ? R.hd[st].baseB : R.hd[st].baseA;
			const int got = (int)(int16_t)(k2a_ofs_off(R.rec[(size_t)st * K2A_CK_REC_WORDS(C) + c]) >> shf) + base - sc.e * i;
			CHECK(got == ref[h].rmax[i], "C=%d half %d row %d: per-row form %d, the recurrence %d", C, h, i, got, ref[h].rmax[i]);
			if (ref[h].rcol[i] == 0) ++g_col0;
			else if (ref[h].rcol[i] == i - w) ++g_left;
			if (ref[h].rcol[i] == i + w && ref[h].rcol[i] > 0) ++g_right;
			if (i + 1 < tlen) {
				const int d = ref[h].rmax[i] - ref[h].rmax[i + 1];
				CHECK(d <= s.delta && -d <= s.delta, "C=%d half %d rows %d / %d: maxima %d and %d differ by more than delta = %d (columns %d, %d; w %d)", C, h, i, i + 1,
				      ref[h].rmax[i], ref[h].rmax[i + 1], s.delta, ref[h].rcol[i], ref[h].rcol[i + 1], w);
			}
		}
		for (int st = 0; st < ns; ++st) {
			const int baseR = h ? R.hd[st].baseB : R.hd[st].baseA, baseP = h ? P.hd[st].baseB : P.hd[st].baseA;
			CHECK(baseR == baseP && R.hd[st].hd0 == P.hd[st].hd0, "C=%d half %d strip %d: the forms' headers differ", C, h, st);
			for (int p = 0; p < C / 2 && st * C + 2 * p < tlen; ++p) {
				const int i = st * C + 2 * p;
				const int want = i + 1 < tlen ? imax2(ref[h].rmax[i], ref[h].rmax[i + 1]) : ref[h].rmax[i];
				const int got = (int)(int16_t)(k2a_ofs_off(P.rec[(size_t)st * K2A_CK_REC_WORDS(C) + p]) >> shf) + hq + baseP - sc.e * i;
				++g_pairs;
				if (got != want) {
					/* only a border F: the odd row starts at column 0, at most q above, and it stands for a negative H */
					CHECK(got > want && got - want <= sc.q && i + 1 < tlen && i + 1 <= w && got < 0, "C=%d half %d strip %d pair %d (row %d): pair maximum %d, the rows' %d", C, h, st, p, i, got, want);
					++g_border_pairs;
				}
			}
			/* the records' hl parts are the same registers in both forms */
			if (k2a_pkfold_strip_reaches<C>(st, qlen, tlen, w))
				for (int c = 0; c < C; ++c)
					CHECK(R.rec[(size_t)st * K2A_CK_REC_WORDS(C) + C + c] == P.rec[(size_t)st * K2A_CK_REC_WORDS(C) + C + c], "C=%d strip %d row %d: hl differs between the forms", C, st, c);
		}
	}

	/* (c), (d), (e) */
	const int zds[] = { -1, 0, s.delta, 2 * sc.pk_pm - 1, 2 * sc.pk_pm, 50, 100, 400 };
	for (int zd : zds) {
		K2aBook want[2], got[2], old[2];
		{	/* K2aLanePk::do_fin_seq, DEFER branch, strip by strip (as tests/stripfold/stripfold_check.cpp) */
			typedef K2aLanePk<64, C, false, K2A_MODE_SCORE, true, false, 0, true, false> Lane;
			static Lane L;
			k2a_book_reset(&want[0]); k2a_book_reset(&want[1]);
			for (int st = 0; st < ns; ++st) {
				uint32_t rowbuf[K2A_PK_STAGE(C)];
				L.i0 = st * C; L.tlen = tlen; L.tlen_full = tlen_full; L.w = w; L.qlen = qlen;
				L.baseA = R.hd[st].baseA; L.baseB = R.hd[st].baseB;
				for (int c = 0; c < C; ++c) {
					rowbuf[c] = k2a_ofs_off(R.rec[(size_t)st * K2A_CK_REC_WORDS(C) + C + c]);
					rowbuf[C + c] = k2a_ofs_off(R.rec[(size_t)st * K2A_CK_REC_WORDS(C) + c]);
					rowbuf[2 * C + c] = 0;
				}
				L.do_fin_seq(sc, &want[0], &want[1], zd, zd, rowbuf);
			}
		}
		std::vector<uint32_t> xb(K2A_PKFOLD_XB_WORDS, 0xa5a5a5a5u);
		k2a_book_reset(&old[0]); k2a_book_reset(&old[1]);
		k2a_pkfold_task<C, 64>(sc, R.rec.data(), R.hd.data(), ns, qlen, tlen, tlen_full, w, zd, zd, &old[0], &old[1], xb.data(), 0);
		k2a_book_reset(&got[0]); k2a_book_reset(&got[1]);
		k2a_pkfold_task_pm<C, 64>(sc, P.rec.data(), P.hd.data(), ns, qlen, tlen, tlen_full, w, zd, zd, sc.pk_pm, &got[0], &got[1], xb.data(), 0);
		for (int h = 0; h < 2; ++h) {
			++g_books;
			CHECK(same_book(old[h], want[h]), "C=%d zdrop %d half %d: the per-row fold and do_fin_seq differ", C, zd, h);
			const K2aBook &g = got[h], &x = want[h];
			K2aBook e = x;                                          /* what the new fold should have left */
			int lim = tlen;
			g_frozen_ref += x.dropped;
			if (g.dropped) {
				++g_frozen_new;
				const int fr = g.rows - 1;                          /* (d): at or before the per-row form's freeze row; an even row of its strip */
				CHECK(g.inexact == 1 && fr >= 0 && fr < tlen && ((fr % C) & 1) == 0 && (!x.dropped || fr <= x.rows - 1), "C=%d zdrop %d half %d: froze at row %d, the per-row form %s at %d",
				      C, zd, h, fr, x.dropped ? "froze" : "did not freeze: rows", x.rows - 1);
				if (!x.dropped || fr < x.rows - 1) ++g_frozen_early;
				k2a_book_reset(&e);                                 /* the exact book in front of row fr */
				for (int i = 0; i < fr; ++i) {
					if (i + w >= qlen - 1 && ref[h].hend[i] > e.mqe) { e.mqe = ref[h].hend[i]; e.mqe_t = i; }
					if (ref[h].rmax[i] > e.max) { e.max = ref[h].rmax[i]; e.max_t = i; e.max_q = 0; }
				}
				e.dropped = e.inexact = 1; e.rows = fr + 1;
				lim = fr;
			} else CHECK(!x.dropped, "C=%d zdrop %d half %d: the per-row form froze at row %d, the pair form did not", C, zd, h, x.rows - 1);      /* (e) */
			/* max_t: the pair's first row; mte: the pair's maximum (an unfrozen book has folded the last row) */
			K2aBook prov = e;
			if (e.max_t >= 0) prov.max_t = e.max_t - ((e.max_t % C) & 1);
			if (!g.dropped && tlen == tlen_full) {                  /* (the record's value: checked against the rows' maxima under (a)) */
				const int i = (tlen - 1) - (((tlen - 1) % C) & 1), st = i / C;
				prov.mte = (int)(int16_t)(k2a_ofs_off(P.rec[(size_t)st * K2A_CK_REC_WORDS(C) + (i % C) / 2]) >> (h ? 16 : 0)) + hq + (h ? P.hd[st].baseB : P.hd[st].baseA) - sc.e * i;
			}
			if (!same_book(g, prov)) {
				CHECK(false, "C=%d RB %d zdrop %d half %d (qlen %d tlen %d w %d, kinds %d %d): the pair fold's book", C, (int)RB, zd, h, qlen, tlen, w, (int)kA, (int)kB);
				if (g_fail < 40) { print_book("pair fold", g); print_book("expected ", prov); print_book("per-row  ", x); }
			}
			/* the second pass: the first row of max_t's strip, in front of the freeze row, whose maximum is the strip's largest */
			if (g.max_t >= 0) {
				const int st = g.max_t / C;
				int best = NEGI, arg = -1;
				for (int c = 0; c < C; ++c) { const int i = st * C + c; if (i < lim && ref[h].rmax[i] > best) { best = ref[h].rmax[i]; arg = i; } }
				CHECK(arg == e.max_t && best == e.max, "C=%d zdrop %d half %d: the second pass would name row %d (%d), the exact book has %d (%d)", C, zd, h, arg, best, e.max_t, e.max);
				++g_resolved;
			}
		}
	}
}

template<int C>
static void run_geom(const std::vector<Scoring> &scs)
{
	const int wmax = (64 * (C + 1) - C) / 2, tl1 = 64 * C + 1, tl2 = 2 * 64 * C + 5;
	const Shape shapes[] = {
		{ tl1, tl1, 0 }, { tl1, tl1, C }, { tl1 + C + 1, tl1, C + 1 }, { tl1, tl1, wmax }, { tl2, tl2, wmax }, { tl2, tl2, C + 1 }, { tl2 - 30, tl2, C },
		{ tl1 - 100, tl1, C },                                  /* qlen + w < tlen: rows the band never reaches */
		{ 63 * C + 20, 63 * C + C / 2 + 1, C + 1 },             /* a partial last strip */
		{ 45, 37, 5 }, { 3 * C, 3 * C, 3 * C },                 /* a few strips; every row starts at column 0 */
	};
	int n = 0;
	for (const Shape &sh : shapes) {
		for (int k = 0; k < (int)NKIND; ++k, ++n) {
			const Kind kA = (Kind)k, kB = (Kind)((k + 1 + n % 3) % NKIND);
			const Scoring &s = scs[n % scs.size()];
			const bool wild = kA == WILD || kB == WILD, big = sh.tlen_full > tl1;
			if (big && (k % 3) != (n / NKIND) % 3) continue;          /* the long shapes: a third of the kinds each */
			if (s.sc.pk_base != 0 || wild) { if (n & 1) run_case<C, true, true>(s, sh, kA, kB); else run_case<C, false, true>(s, sh, kA, kB); }
			else { if (n & 1) run_case<C, true, false>(s, sh, kA, kB); else run_case<C, false, false>(s, sh, kA, kB); }
		}
	}
}

int main()
{
	std::vector<Scoring> scs;
	scs.push_back(scoring(2, -4, -4, -1, 4, 2));                  /* the preset */
	scs.push_back(scoring(2, -2, -4, -1, 4, 2));                  /* transitions cost less than transversions */
	scs.push_back(scoring(2, -7, -7, -1, 4, 2));                  /* a score below -(q + e): pk_base != 0, the TN build */
	scs.push_back(scoring(1, -3, -3, 0, 5, 1));
	run_geom<8>(scs);
	const long c8 = g_cases;
	run_geom<16>(scs);
	printf("C=8: %ld cases\nC=16: %ld cases\n", c8, g_cases - c8);
	printf("%ld pair maxima (%ld lifted by a border F), best cells: %ld at column 0, %ld on the left band edge, %ld on the right\n", g_pairs, g_border_pairs, g_col0, g_left, g_right);
	printf("%ld books: the pair fold froze %ld (%ld of them before the per-row form, or where it never does), the per-row fold %ld; %ld rows resolved as the second pass does\n",
	       g_books, g_frozen_new, g_frozen_early, g_frozen_ref, g_resolved);
	CHECK(g_col0 > 0 && g_left > 0 && g_right > 0, "the cases do not hold best cells at column 0 and on both band edges");
	CHECK(g_frozen_new > g_books / 20 && g_frozen_new < g_books - g_books / 20 && g_frozen_ref > 0 && g_frozen_early > 0, "the cases do not cover frozen and unfrozen books in both forms");
	if (g_fail) { printf("stripmax check FAILED: %d\n", g_fail); return 1; }
	printf("stripmax check ok\n");
	return 0;
}
