/*
 * hlopen_check.cpp -- host check of what the packed lanes' row registers hold (K2A_HL_OPEN, ksw2_lane_pk.h "Open form": hl[] and the
 * ports hout / hin / hd0 / hu_prev carry H - q, the column profiles q + e + s) against a plain int32 recurrence written here.
 *
 * One group of G K2aLanePk<G, C, DUAL, MODE, RB> lanes runs whole small alignments in lock step through the loop of k2a_fill_pk_body
 * (ksw2_shim_hip.hip; same order of events: strip start, rotate, re-base shift, query pick, top inputs, step, strip end), two
 * alignments of one shape per lane.  Compared with the recurrence, for both alignments:
 *   - every row's maximum, and its H at the query's last column where the row reaches it, as the strip epilogue sees them (stage_rows);
 *   - H of the last target row at every in-band column, read from the row register after each step;
 *   - the books behind do_fin_seq: max, mqe and score.
 * The recurrence is the textbook affine one with the reference's borders (ksw2_extz.c:32-44, ksw2_extd.c:33-52) on the band
 * |i - j| <= w, cells outside it -infinity; it knows nothing of row bias, bases, offset form or what a register holds.
 *
 * Cases: (8, 18) and (16, 8) at targets of up to three rounds of strips, (64, 16) at 64 * 16 + 17 rows; plain and re-based, single
 * and two-piece gaps, score only and left-aligned traceback; bands 0, C and the widest the geometry admits.  Two scorings: the 2 / -4
 * / N -1 preset (every profile byte fits: the plain build of the lane), and mismatch -7 under q = 4, e = 2 (a score below -(q + e):
 * bytes less K2aScoring.pk_base, the TN build of the lane, whose slow path adds the constant).
 *
 * A stand-alone program: g++ -O1 -fsanitize=address,undefined -pthread -I ksw2_amd/csrc tests/hlopen/hlopen_check.cpp && ./a.out
 * returns 0 when every check held.  usage: a.out [threads]     (-DHLOPEN_GEOM=0 / 1 / 2: one of the three geometries only)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "ksw2_lane_pk.h"

struct Shape { int qlen, tlen_full, w; };

static thread_local uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
	return (uint32_t)(g_rng >> 32);
}

static int score_of(int mis, int t, int q) { return (t > 3 || q > 3) ? -1 : t == q ? 2 : mis; }

/* the table as the host builds it (ksw2_host_plan.c::pk_scoring) for match 2 / mismatch `mis` / wildcard -1, q = 4, e = 2 (24 / 1) */
static K2aScoring scoring(int mis, bool dual)
{
	K2aScoring sc;
	memset(&sc, 0, sizeof(sc));
	sc.q = 4; sc.e = 2; sc.q2 = dual ? 24 : 0; sc.e2 = dual ? 1 : 0; sc.m = 5; sc.pk_smax = 2;
#if K2A_HL_OPEN
	int lo = 1 << 30, hi = -(1 << 30);
	for (int q = 0; q < 5; ++q)
		for (int t = 0; t < 4; ++t) { const int v = sc.q + sc.e + score_of(mis, t, q); lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
	sc.pk_base = lo < 0 ? lo : hi > 255 ? hi - 255 : 0;
	for (int q = 0; q < 5; ++q)
		for (int t = 0; t < 4; ++t) sc.cp[q] |= (uint32_t)(sc.q + sc.e + score_of(mis, t, q) - sc.pk_base) << (8 * t);
#else
	for (int q = 0; q < 5; ++q)
		for (int t = 0; t < 4; ++t) sc.cp[q] |= (uint32_t)(2 - score_of(mis, t, q)) << (8 * t);
#endif
	return sc;
}

enum { NEGI = -(1 << 28) };
static inline int imax2(int a, int b) { return a > b ? a : b; }

/* the recurrence: per row its H at the last in-band column and its maximum; the last row's H per column */
struct Scalar {
	std::vector<int> hend, rmax, lastrow;
};
template<bool DUAL>
static void scalar_fill(const K2aScoring &sc, int mis, const uint8_t *q, const uint8_t *t, int qlen, int tlen, int w, Scalar &o)
{
	std::vector<int> Hp(qlen, NEGI), Ep(qlen, NEGI), E2p(qlen, NEGI), Hc(qlen, NEGI), Ec(qlen, NEGI), E2c(qlen, NEGI);
	o.hend.assign(tlen, NEGI); o.rmax.assign(tlen, NEGI); o.lastrow.assign(qlen, NEGI);
	for (int i = 0; i < tlen; ++i) {
		const int jlo = imax2(0, i - w), jhi = i + w < qlen - 1 ? i + w : qlen - 1;
		int F = NEGI, F2 = NEGI, Hleft = NEGI;
		for (int j = jlo; j <= jhi; ++j) {
			const int diag = i == 0 ? k2a_border<DUAL>(sc, j) : j == 0 ? k2a_border<DUAL>(sc, i) : Hp[j - 1];
			int E, E2;
			if (i == 0) { E = k2a_border<DUAL>(sc, j + 1) - (sc.q + sc.e); E2 = k2a_border<DUAL>(sc, j + 1) - (sc.q2 + sc.e2); }
			else if (j - (i - 1) <= w) { E = imax2(Ep[j], Hp[j] - sc.q) - sc.e; E2 = imax2(E2p[j], Hp[j] - sc.q2) - sc.e2; }
			else E = E2 = NEGI;
			if (j == 0) { F = k2a_border<DUAL>(sc, i + 1) - (sc.q + sc.e); F2 = k2a_border<DUAL>(sc, i + 1) - (sc.q2 + sc.e2); }
			else if (i - (j - 1) <= w) { F = imax2(F, Hleft - sc.q) - sc.e; F2 = imax2(F2, Hleft - sc.q2) - sc.e2; }
			else F = F2 = NEGI;
			int H = imax2(imax2(diag + score_of(mis, t[i], q[j]), E), F);
			if (DUAL) H = imax2(imax2(H, E2), F2);
			Hc[j] = H; Ec[j] = E; E2c[j] = E2; Hleft = H;
			o.rmax[i] = imax2(o.rmax[i], H);
			if (j == jhi) o.hend[i] = H;
			if (i == tlen - 1) o.lastrow[j] = H;
		}
		Hp.swap(Hc); Ep.swap(Ec); E2p.swap(E2c);
	}
}

static std::atomic<long> g_cases, g_rows, g_lastcells;

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return false; } while (0)

template<int G, int C, bool DUAL, int MODE, bool RB, bool TN>
static bool run_case(const Shape &s, int mis)
{
	typedef K2aLanePk<G, C, DUAL, MODE, RB, false, 0, false, TN> Lane;
	const K2aScoring sc = scoring(mis, DUAL);
	if ((sc.pk_base != 0) != TN) FAIL("scoring with mismatch %d: pk_base %d, TN %d", mis, sc.pk_base, (int)TN);
	std::vector<Lane> L(G);
	K2aPair pr[2];
	std::vector<uint8_t> seq;
	for (int h = 0; h < 2; ++h) {
		K2aPair &p = pr[h];
		memset(&p, 0, sizeof(p));
		p.qlen = s.qlen; p.tlen_full = s.tlen_full; p.w = s.w;
		p.tlen = s.qlen + s.w < s.tlen_full ? s.qlen + s.w : s.tlen_full;       /* rows that own an in-band cell (ksw2_host_single.c) */
		p.zdrop = -1;
		p.qoff = (uint32_t)seq.size();
		for (int x = 0; x < s.qlen; ++x) seq.push_back((uint8_t)(rnd() % 100 < 2 ? 4 : rnd() & 3));
		seq.resize(seq.size() + 8, 0);
		p.toff = (uint32_t)seq.size();
		const uint32_t base = p.qoff;
		for (int x = 0; x < s.tlen_full; ++x) {                                  /* mostly the query again, with an indel now and then */
			const uint32_t r = rnd() % 100;
			const int src = x + (x > s.tlen_full / 2 ? 2 : 0);
			const bool follow = src < s.qlen && r >= 8;
			const uint8_t c = follow ? seq[base + src] : (uint8_t)(rnd() & 3);
			seq.push_back(c > 3 ? 0 : c);
		}
		seq.resize(seq.size() + C + 8, 0);
	}
	seq.resize(seq.size() + 64, 0);
	const int tlen = pr[0].tlen;
	Scalar ref[2];
	for (int h = 0; h < 2; ++h) scalar_fill<DUAL>(sc, mis, seq.data() + pr[h].qoff, seq.data() + pr[h].toff, s.qlen, tlen, s.w, ref[h]);

	K2aBook bk[2];
	uint32_t stage[K2A_PK_STAGE(C)];
	for (int l = 0; l < G; ++l) {
		L[l].lrow = 0;
		L[l].setup(pr[0], pr[1], seq.data(), l, true, sc.cp);
		L[l].load_query_group(0, L[l].knext == 0 ? L[l].koff_next : L[l].koff, L[l].qwA, L[l].qwB);
	}
	for (int h = 0; h < 2; ++h) k2a_book_reset(&bk[h]);
	const int kmax = L[0].last_step();
	const int ktop = k2a_min(s.qlen - 1, k2a_min(C - 1, tlen - 1) + s.w);
	const int hq = k2a_hl_q(sc);
	std::vector<uint32_t> qpa(G), qpb(G);
	std::vector<k2a_pk> hin(G), ein(G), e2in(G);
	std::vector<int> bsA(G), bsB(G);
	std::vector<char> rowseen(tlen, 0), lastseen(s.qlen, 0);
	for (int k = 0; k <= kmax; ++k) {
		for (int l = 0; l < G; ++l) {
			const int src = (l + G - 1) % G;
			hin[l] = L[src].hout; ein[l] = L[src].eout; e2in[l] = DUAL ? L[src].e2out : 0u; bsA[l] = L[src].baseA; bsB[l] = L[src].baseB;
		}
		for (int l = 0; l < G; ++l) {
			if (L[l].need_init(k)) { L[l].do_init(sc, RB ? bsA[l] : 0, RB ? bsB[l] : 0); if (k & 3) L[l].reload_query_group(k); }
			L[l].hu_prev = hin[l];
			if (RB) { hin[l] = k2a_pk_add(hin[l], L[l].delta); ein[l] = k2a_pk_add(ein[l], L[l].delta); if (DUAL) e2in[l] = k2a_pk_add(e2in[l], L[l].delta); }
			if ((k & 3) == 0) L[l].load_query_group(k + 4, L[l].knext <= k + 4 ? L[l].koff_next : L[l].koff, qpa[l], qpb[l]);
			L[l].set_qb(Lane::query_pick(L[l].qwA, L[l].qwB, k & 3));
			if (k <= ktop) L[l].top_inputs(sc, k, hin[l], ein[l], e2in[l]);
		}
		bool wn = false;                                                   /* K2A_SYNC_WN */
		for (int l = 0; l < G; ++l) wn |= L[l].hasn != 0;
		for (int l = 0; l < G; ++l) L[l].wn = wn;
		for (int l = 0; l < G; ++l) {
			uint32_t tw[Lane::TBWORDS];
			L[l].step(sc, k, hin[l], ein[l], e2in[l], tw);
			/* the last target row, column by column, out of the row register */
			if (L[l].S >= 0 && L[l].i0 <= tlen - 1 && tlen - 1 < L[l].i0 + C) {
				const int i = tlen - 1, j = k - L[l].koff, c = i - L[l].i0;
				if (j >= 0 && j < s.qlen && j >= i - s.w && j <= i + s.w) {
					const k2a_pk v = k2a_ofs_off(L[l].hl[c]);
					const int gA = k2a_pk_lo(v) + hq + (RB ? L[l].baseA : 0) - sc.e * i, gB = k2a_pk_hi(v) + hq + (RB ? L[l].baseB : 0) - sc.e * i;
					if (gA != ref[0].lastrow[j] || gB != ref[1].lastrow[j])
						FAIL("last row: column %d: %d / %d, the recurrence has %d / %d", j, gA, gB, ref[0].lastrow[j], ref[1].lastrow[j]);
					lastseen[j] = 1; ++g_lastcells;
				}
			}
		}
		for (int l = 0; l < G; ++l) {
			if (!L[l].need_fin(k)) continue;
			const int i0 = L[l].i0, bA = RB ? L[l].baseA : 0, bB = RB ? L[l].baseB : 0;
			L[l].stage_rows(stage);
			for (int c = 0; c < C && i0 + c < tlen; ++c) {
				const int i = i0 + c;
				const int hA = (int)(int16_t)(stage[c] & 0xffffu) + hq + bA - sc.e * i, hB = (int)(int16_t)(stage[c] >> 16) + hq + bB - sc.e * i;
				const int mA = (int)(int16_t)(stage[C + c] & 0xffffu) + bA - sc.e * i, mB = (int)(int16_t)(stage[C + c] >> 16) + bB - sc.e * i;
				/* (a row that ends before the query does is dead at the strip's last step: its register then holds -infinity) */
				if (i + s.w >= s.qlen - 1 && (hA != ref[0].hend[i] || hB != ref[1].hend[i])) FAIL("row %d: H at its last column %d / %d, the recurrence has %d / %d", i, hA, hB, ref[0].hend[i], ref[1].hend[i]);
				if (mA != ref[0].rmax[i] || mB != ref[1].rmax[i]) FAIL("row %d: maximum %d / %d, the recurrence has %d / %d", i, mA, mB, ref[0].rmax[i], ref[1].rmax[i]);
				rowseen[i] = 1; ++g_rows;
			}
			L[l].do_fin_seq(sc, &bk[0], &bk[1], -1, -1, stage);
		}
		if ((k & 3) == 3)
			for (int l = 0; l < G; ++l) { L[l].qwA = qpa[l]; L[l].qwB = qpb[l]; }
	}
	for (int i = 0; i < tlen; ++i) if (!rowseen[i]) FAIL("row %d never reached a strip end", i);
	for (int j = imax2(0, tlen - 1 - s.w); j < s.qlen && j <= tlen - 1 + s.w; ++j) if (!lastseen[j]) FAIL("last row: column %d never seen", j);
	for (int h = 0; h < 2; ++h) {
		int mx = 0, mqe = K2A_NEG;
		for (int i = 0; i < tlen; ++i) { mx = imax2(mx, ref[h].rmax[i]); if (i + s.w >= s.qlen - 1) mqe = imax2(mqe, ref[h].hend[i]); }
		const bool corner = tlen == s.tlen_full && tlen - 1 + s.w >= s.qlen - 1;
		if (bk[h].max != mx || bk[h].mqe != mqe || bk[h].score != (corner ? ref[h].hend[tlen - 1] : K2A_NEG) || bk[h].rows != tlen)
			FAIL("book %d: max %d mqe %d score %d rows %d, the recurrence has %d %d %d %d", h, bk[h].max, bk[h].mqe, bk[h].score, bk[h].rows, mx, mqe,
			     corner ? ref[h].hend[tlen - 1] : K2A_NEG, tlen);
	}
	++g_cases;
	return true;
}

static int g_threads = 1;

/* what the plan admits for the (G, C) array (geom_fits, ksw2_host_plan.c); the band as the host resolves it */
template<int G, int C>
static bool admit(Shape &s)
{
	if (s.qlen < 1 || s.tlen_full < 1 || s.w < 0) return false;
	const int mx = s.qlen > s.tlen_full ? s.qlen : s.tlen_full;
	if (s.w > mx) s.w = mx;
	const int tlen = s.qlen + s.w < s.tlen_full ? s.qlen + s.w : s.tlen_full;
	const int nstrips = (tlen + C - 1) / C;
	return nstrips <= G || 2 * (long)s.w < (long)G * (C + 1) - C + 1;
}

template<int G, int C, bool DUAL, int MODE, bool RB>
static bool run_form(const std::vector<int> &tls)
{
	const int wmax = (G * (C + 1) - C) / 2;
	const int ws[] = { 0, C, wmax };
	std::vector<Shape> shapes;
	for (int w : ws)
		for (int tl : tls) {
			const int qls[] = { tl, tl - w, tl + w + 3 };
			for (int ql : qls) {
				Shape s = { ql, tl, w };
				if (!admit<G, C>(s)) continue;
				bool dup = false;
				for (const Shape &o : shapes) dup |= o.qlen == s.qlen && o.tlen_full == s.tlen_full && o.w == s.w;
				if (!dup) shapes.push_back(s);
			}
		}
	const long c0 = g_cases;
	std::atomic<size_t> next(0);
	std::atomic<bool> ok(true);
	auto work = [&]() {
		for (size_t x; ok && (x = next++) < 2 * shapes.size(); ) {
			g_rng = 0x9E3779B97F4A7C15ull * (x + 1) + (uint64_t)(G * 1000 + C * 10 + (DUAL ? 4 : 0) + MODE * 2 + (RB ? 1 : 0));
			const Shape &s = shapes[x / 2];
			const bool good = (x & 1) ? run_case<G, C, DUAL, MODE, RB, true>(s, -7) : run_case<G, C, DUAL, MODE, RB, false>(s, -4);
			if (!good) {
				fprintf(stderr, "  in (%d,%d) dual %d mode %d RB %d mismatch %d: qlen %d tlen %d w %d\n", G, C, (int)DUAL, MODE, (int)RB, (x & 1) ? -7 : -4, s.qlen, s.tlen_full, s.w);
				ok = false;
			}
		}
	};
	std::vector<std::thread> th;
	for (int t = 1; t < g_threads; ++t) th.emplace_back(work);
	work();
	for (std::thread &t : th) t.join();
	if (!ok) return false;
	printf("(%d,%d) dual %d mode %d RB %d: %ld cases\n", G, C, (int)DUAL, MODE, (int)RB, g_cases - c0);
	return true;
}

template<int G, int C>
static bool run_geom(const std::vector<int> &tls)
{
	return run_form<G, C, false, K2A_MODE_SCORE, false>(tls) && run_form<G, C, false, K2A_MODE_SCORE, true>(tls) &&
	       run_form<G, C, true, K2A_MODE_SCORE, false>(tls) && run_form<G, C, true, K2A_MODE_SCORE, true>(tls) &&
	       run_form<G, C, false, K2A_MODE_LEFT, false>(tls) && run_form<G, C, false, K2A_MODE_LEFT, true>(tls) &&
	       run_form<G, C, true, K2A_MODE_LEFT, false>(tls) && run_form<G, C, true, K2A_MODE_LEFT, true>(tls);
}

int main(int argc, char **argv)
{
	const int hw = (int)std::thread::hardware_concurrency();
	g_threads = argc > 1 ? atoi(argv[1]) : hw < 1 ? 1 : hw > 16 ? 16 : hw;
	/* one row; one strip and a bit; one, two and three rounds of strips, each a bit over or under.  -DHLOPEN_GEOM=0/1/2 builds one
	 * geometry only (tests/test_hlopen_cpu.py compiles the three side by side) */
#ifndef HLOPEN_GEOM
#define HLOPEN_GEOM -1
#endif
	bool ok = true;
	if (HLOPEN_GEOM < 0 || HLOPEN_GEOM == 0) ok = ok && run_geom<8, 18>({ 1, 18, 19, 8 * 18 + 1, 2 * 8 * 18 + 5, 3 * 8 * 18 - 1 });
	if (HLOPEN_GEOM < 0 || HLOPEN_GEOM == 1) ok = ok && run_geom<16, 8>({ 1, 8, 9, 16 * 8 + 1, 2 * 16 * 8 + 5, 3 * 16 * 8 - 1 });
	if (HLOPEN_GEOM < 0 || HLOPEN_GEOM == 2) ok = ok && run_geom<64, 16>({ 64 * 16 + 17 });
	if (!ok) return 1;
	printf("K2A_HL_OPEN %d: %ld cases, %ld rows at strip ends, %ld cells of last rows agree with the recurrence\n", (int)K2A_HL_OPEN, g_cases.load(), g_rows.load(), g_lastcells.load());
	printf("hlopen check ok\n");
	return 0;
}
