/*
 * initflag_check.cpp -- host check of K2aLanePk::do_init's wavefront-uniform "some new strip has column-0 rows" flag
 * (do_init<true>(.., col0_any), what k2a_fill_pk_body passes with K2A_INIT_COL0_UNIFORM) against the plain do_init.
 *
 * 64 K2aLanePk<64, 16, false, SCORE, RB, false, 2, true> lanes (the headline fill's lane: deferred arg-max, row selectors in LDS) run
 * in lock step through the loop of k2a_fill_pk_body (ksw2_shim_hip.hip; same order of events), twice on two copies of the lane
 * state and of the two books:
 *   copy X: do_init as every other caller uses it;
 *   copy Y: do_init<true> with the flag as the kernel forms it -- the OR over the lanes that start a strip at this step of
 *           Snext * C <= w, taken BEFORE do_init sets i0 -- so that the border rows are skipped whenever no such lane has one.
 * Both end their strips as the kernel does (fin_fast, else stage_rows + do_fin_seq).  The lane state of X and Y is compared after
 * every step -- rows, ports, bases, schedule and the row selectors in LDS -- and the books after every strip and at the end.
 *
 * The flag is formed HERE, by this program, in the way the kernel's comment describes; the kernel's own ballot (where it is taken, what
 * it covers) is not host code and is tied to the results only by the GPU parity tests (tests/test_gpu_strip_events.py, and every
 * other packed score-only test).  What this program establishes is the lane method: do_init<true> with a flag formed that way leaves
 * every lane exactly as do_init does.
 *
 * Shapes: the (w, tlen, qlen) grid of tests/rowmask/rowmask_check.cpp for (64, 16) with targets of more than one, two and three
 * rounds of strips added (GC + 1, GC + C + 1, 2GC + 5, 3GC + C - 1), without a Z-drop and with one on either or both alignments,
 * re-based and not.  The program prints how many steps with a strip start ran with the flag off and on; tests/test_initflag_cpu.py
 * asserts that both occurred.
 *
 * A stand-alone program: g++ -O1 -fsanitize=address,undefined -pthread -I ksw2_amd/csrc tests/stripev/initflag_check.cpp && ./a.out
 * returns 0 when every check held.  usage: a.out [threads]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "ksw2_lane_pk.h"

enum { G = 64, C = 16, GC = G * C };

struct Shape { int qlen, tlen_full, w; };
struct Case { Shape sh; int zdropA, zdropB; };

static thread_local uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
	return (uint32_t)(g_rng >> 32);
}

static K2aScoring scoring()
{
	K2aScoring sc;
	memset(&sc, 0, sizeof(sc));
	sc.q = 4; sc.e = 2; sc.m = 5; sc.pk_smax = 2;                  /* match 2, mismatch -4, wildcard -1 */
	for (int q = 0; q < 5; ++q)
		for (int t = 0; t < 4; ++t) sc.cp[q] |= (uint32_t)(q == 4 ? 3 : q == t ? 0 : 6) << (8 * t);
	return sc;
}

static std::atomic<long> g_init_off, g_init_on, g_steps, g_cases, g_dropped;

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return false; } while (0)

static bool same_book(const K2aBook &a, const K2aBook &b)
{
	return a.max == b.max && a.max_t == b.max_t && a.max_q == b.max_q && a.mqe == b.mqe && a.mqe_t == b.mqe_t && a.mte == b.mte &&
	       a.mte_q == b.mte_q && a.score == b.score && a.rows == b.rows && a.dropped == b.dropped && a.inexact == b.inexact;
}

template<bool RB>
static bool run_case(const Case &cs)
{
	typedef K2aLanePk<G, C, false, K2A_MODE_SCORE, RB, false, 2, true, false> Lane;
	const K2aScoring sc = scoring();
	const Shape s = cs.sh;
	std::vector<Lane> X(64), Y(64);
	std::vector<uint32_t> lrowX(C * 64, 0), lrowY(C * 64, 0);
	K2aPair pr[2];
	std::vector<uint8_t> seq;
	for (int h = 0; h < 2; ++h) {
		K2aPair &p = pr[h];
		memset(&p, 0, sizeof(p));
		p.qlen = s.qlen; p.tlen_full = s.tlen_full; p.w = s.w;
		p.tlen = s.qlen + s.w < s.tlen_full ? s.qlen + s.w : s.tlen_full;       /* rows that own an in-band cell (ksw2_host_single.c) */
		p.zdrop = h ? cs.zdropB : cs.zdropA;
		p.qoff = (uint32_t)seq.size();
		for (int x = 0; x < s.qlen; ++x) seq.push_back((uint8_t)(rnd() % 100 < 3 ? 4 : rnd() & 3));
		seq.resize(seq.size() + 8, 0);
		p.toff = (uint32_t)seq.size();
		const uint32_t base = p.qoff;
		for (int x = 0; x < s.tlen_full; ++x) {                                  /* mostly the query again: real scores, not all -inf */
			const uint32_t r = rnd() % 100;
			const bool follow = x < s.qlen && r >= 10;
			const uint8_t c = follow ? seq[base + x] : (uint8_t)(rnd() & 3);
			seq.push_back(c > 3 ? 0 : c);
		}
		seq.resize(seq.size() + C + 8, 0);
	}
	seq.resize(seq.size() + 64, 0);
	const int zdropA = pr[0].zdrop, zdropB = pr[1].zdrop;

	K2aBook bX[2], bY[2];
	uint32_t stage[K2A_PK_STAGE(C)];
	for (int l = 0; l < 64; ++l) {
		X[l].lrow = &lrowX[l];
		X[l].setup(pr[0], pr[1], seq.data(), l, true, sc.cp);
		X[l].load_query_group(0, X[l].knext == 0 ? X[l].koff_next : X[l].koff, X[l].qwA, X[l].qwB);
		Y[l] = X[l];
		Y[l].lrow = &lrowY[l];
	}
	memcpy(lrowY.data(), lrowX.data(), lrowX.size() * sizeof(uint32_t));
	for (int h = 0; h < 2; ++h) { k2a_book_reset(&bX[h]); k2a_book_reset(&bY[h]); }
	const int kmax = X[0].last_step();
	const int ktop = k2a_min(pr[0].qlen - 1, k2a_min(C - 1, pr[0].tlen - 1) + pr[0].w);
	uint32_t qpaX[64], qpbX[64], qpaY[64], qpbY[64];
	long init_off = 0, init_on = 0;
	for (int k = 0; k <= kmax; ++k) {
		k2a_pk hinX[64], einX[64], hinY[64], einY[64];
		int bsAX[64], bsBX[64], bsAY[64], bsBY[64];
		for (int l = 0; l < 64; ++l) {
			const int src = (l + 63) % 64;
			hinX[l] = X[src].hout; einX[l] = X[src].eout; bsAX[l] = X[src].baseA; bsBX[l] = X[src].baseB;
			hinY[l] = Y[src].hout; einY[l] = Y[src].eout; bsAY[l] = Y[src].baseA; bsBY[l] = Y[src].baseB;
		}
		/* strips that start at this step; the kernel's flag = its ballot of (ninit && Snext * C <= w) */
		bool col0_any = false, any_init = false;
		for (int l = 0; l < 64; ++l) if (Y[l].need_init(k)) { any_init = true; col0_any |= Y[l].Snext * C <= Y[l].w; }
		for (int l = 0; l < 64; ++l) {
			if (X[l].need_init(k) != Y[l].need_init(k)) FAIL("step %d lane %d: the copies disagree on need_init", k, l);
			if (!X[l].need_init(k)) continue;
			X[l].do_init(sc, RB ? bsAX[l] : 0, RB ? bsBX[l] : 0); if (k & 3) X[l].reload_query_group(k);
			Y[l].template do_init<true>(sc, RB ? bsAY[l] : 0, RB ? bsBY[l] : 0, 0, col0_any); if (k & 3) Y[l].reload_query_group(k);
		}
		if (any_init) { if (col0_any) ++init_on; else ++init_off; }
		uint64_t finmask = 0;
		for (int l = 0; l < 64; ++l) {
			uint32_t tw[Lane::TBWORDS];
			k2a_pk e2 = 0;
			X[l].hu_prev = hinX[l]; Y[l].hu_prev = hinY[l];
			if (RB) {
				hinX[l] = k2a_pk_add(hinX[l], X[l].delta); einX[l] = k2a_pk_add(einX[l], X[l].delta);
				hinY[l] = k2a_pk_add(hinY[l], Y[l].delta); einY[l] = k2a_pk_add(einY[l], Y[l].delta);
			}
			if ((k & 3) == 0) {
				X[l].load_query_group(k + 4, X[l].knext <= k + 4 ? X[l].koff_next : X[l].koff, qpaX[l], qpbX[l]);
				Y[l].load_query_group(k + 4, Y[l].knext <= k + 4 ? Y[l].koff_next : Y[l].koff, qpaY[l], qpbY[l]);
			}
			X[l].set_qb(Lane::query_pick(X[l].qwA, X[l].qwB, k & 3));
			Y[l].set_qb(Lane::query_pick(Y[l].qwA, Y[l].qwB, k & 3));
			if (k <= ktop) { X[l].top_inputs(sc, k, hinX[l], einX[l], e2); Y[l].top_inputs(sc, k, hinY[l], einY[l], e2); }
			X[l].step(sc, k, hinX[l], einX[l], 0u, tw);
			Y[l].step(sc, k, hinY[l], einY[l], 0u, tw);
			if (Y[l].need_fin(k)) finmask |= 1ull << l;
		}
		/* the lane state, bit for bit */
		for (int l = 0; l < 64; ++l) {
			const Lane &a = X[l], &b = Y[l];
			bool same = !memcmp(a.hl, b.hl, sizeof(a.hl)) && !memcmp(a.f, b.f, sizeof(a.f)) && !memcmp(a.rmax_, b.rmax_, sizeof(a.rmax_)) &&
			            a.hout == b.hout && a.eout == b.eout && a.hd0 == b.hd0 && a.baseA == b.baseA && a.baseB == b.baseB && a.delta == b.delta &&
			            a.S == b.S && a.i0 == b.i0 && a.kfin == b.kfin && a.rows_m1 == b.rows_m1 && a.Snext == b.Snext && a.knext == b.knext;
			for (int c = 0; c < C; ++c) same = same && lrowX[c * 64 + l] == lrowY[c * 64 + l];
			if (!same) FAIL("state: step %d lane %d differs  (RB %d; qlen %d tlen %d w %d; S %d i0 %d)", k, l, (int)RB, a.qlen, a.tlen, a.w, a.S, a.i0);
		}
		if (finmask != 0) {
			if (finmask & (finmask - 1)) FAIL("step %d: two strips end at once", k);
			const int l = __builtin_ctzll(finmask);
			const int S = X[l].S;
			if (S % 64 != l) FAIL("step %d: strip %d ends in lane %d", k, S, l);
			if (!X[l].fin_fast(sc, &bX[0], &bX[1], zdropA, zdropB)) { X[l].stage_rows(stage); X[l].do_fin_seq(sc, &bX[0], &bX[1], zdropA, zdropB, stage); }
			if (!Y[l].fin_fast(sc, &bY[0], &bY[1], zdropA, zdropB)) { Y[l].stage_rows(stage); Y[l].do_fin_seq(sc, &bY[0], &bY[1], zdropA, zdropB, stage); }
			for (int h = 0; h < 2; ++h)
				if (!same_book(bX[h], bY[h])) FAIL("book %d differs behind strip %d (RB %d; qlen %d tlen %d w %d)", h, S, (int)RB, s.qlen, s.tlen_full, s.w);
		}
		if ((k & 3) == 3)
			for (int l = 0; l < 64; ++l) { X[l].qwA = qpaX[l]; X[l].qwB = qpbX[l]; Y[l].qwA = qpaY[l]; Y[l].qwB = qpbY[l]; }
	}
	for (int h = 0; h < 2; ++h) {
		if (!same_book(bX[h], bY[h])) FAIL("book %d differs at the end (RB %d; qlen %d tlen %d w %d)", h, (int)RB, s.qlen, s.tlen_full, s.w);
		if (!bX[h].dropped && bX[h].rows != pr[0].tlen) FAIL("book %d saw %d rows of %d", h, bX[h].rows, pr[0].tlen);
		if (bX[h].dropped) ++g_dropped;
	}
	g_init_off += init_off; g_init_on += init_on; g_steps += kmax + 1; ++g_cases;
	return true;
}

/* what the plan admits for the (G, C) array (geom_fits, ksw2_host_plan.c); the band as the host resolves it */
static bool admit(Shape &s)
{
	if (s.qlen < 1 || s.tlen_full < 1 || s.w < 0) return false;
	const int mx = s.qlen > s.tlen_full ? s.qlen : s.tlen_full;
	if (s.w > mx) s.w = mx;
	const int tlen = s.qlen + s.w < s.tlen_full ? s.qlen + s.w : s.tlen_full;
	const int nstrips = (tlen + C - 1) / C;
	return nstrips <= G || 2 * (long)s.w < (long)G * (C + 1) - C + 1;
}

static int g_threads = 1;

template<bool RB>
static bool run_all()
{
	const int wmax = (G * (C + 1) - C) / 2;
	const int ws[] = { 0, 1, C - 1, C, C + 1, 2 * C, wmax / 2, wmax - 1, wmax };
	const int tls[] = { 1, C - 1, C, C + 1, 2 * C + 3, GC - 1, GC, GC + 1, GC + C + 1, 2 * GC + 5, 3 * GC + C - 1 };
	std::vector<Case> cases;
	std::vector<Shape> shapes;
	for (int w : ws)
		for (int tl : tls) {
			const int qls[] = { 1, 2, C, tl, tl - w, tl / 3, tl + w + 3, 2 * tl + 7 };
			for (int ql : qls) {
				Shape s = { ql, tl, w };
				if (tl > 2 * GC && ql != tl && ql != tl - w && ql != tl + w + 3) continue;      /* (the long targets: around the diagonal only) */
				if (!admit(s)) continue;
				bool dup = false;
				for (const Shape &o : shapes) dup |= o.qlen == s.qlen && o.tlen_full == s.tlen_full && o.w == s.w;
				if (dup) continue;
				shapes.push_back(s);
				/* no Z-drop; one that fires here and there on the 10 % mutated pairs, on either alignment or both */
				const size_t n = shapes.size();
				const Case plain = { s, -1, -1 }, z = { s, n % 3 == 1 ? -1 : 24, n % 3 == 2 ? -1 : 24 };
				cases.push_back(plain);
				if (n % 2 == 0 || tl < GC - 1) cases.push_back(z);
			}
		}
	g_steps = 0; g_init_off = 0; g_init_on = 0; g_dropped = 0;
	std::atomic<size_t> next(0);
	std::atomic<bool> ok(true);
	auto work = [&]() {
		for (size_t x; ok && (x = next++) < cases.size(); ) {
			g_rng = 0x9E3779B97F4A7C15ull * (x + 1) + (uint64_t)(RB ? 77 : 0);
			if (!run_case<RB>(cases[x])) ok = false;
		}
	};
	std::vector<std::thread> th;
	for (int t = 1; t < g_threads; ++t) th.emplace_back(work);
	work();
	for (std::thread &t : th) t.join();
	if (!ok) return false;
	printf("RB %d: %zu cases, %ld steps, %ld frozen books; steps with a strip start: %ld with the flag off, %ld on; lane state and books agree\n",
	       (int)RB, cases.size(), g_steps.load(), g_dropped.load(), g_init_off.load(), g_init_on.load());
	return true;
}

int main(int argc, char **argv)
{
	const int hw = (int)std::thread::hardware_concurrency();
	g_threads = argc > 1 ? atoi(argv[1]) : hw < 1 ? 1 : hw > 16 ? 16 : hw;
	const bool ok = run_all<true>() && run_all<false>();
	if (!ok) return 1;
	printf("initflag check ok\n");
	return 0;
}
