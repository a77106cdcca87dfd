/*
 * rowmask_check.cpp -- host check of the wavefront-uniform row masks (ksw2_amd/csrc/ksw2_lane_rowmask.h) against the per-lane
 * band test of K2aLanePk::step.
 *
 * 64 K2aLanePk lanes run in lock step through the loop of k2a_fill_pk_body (ksw2_shim_hip.hip; same order of events: rotate the
 * ports, start strips, advance the masks, step, end strips), twice on two copies of the lane state: copy A with the per-lane row
 * predicate (K2aRowPredLane = K2aLanePk::step), copy B with the uniform one (K2aRowPredUniform over K2aRowMasks), the masks fed
 * with "ballots" assembled lane by lane.  At every step
 *   (a) bit l of m[c] must equal lane l's own live bit of row c, for every row and lane (and the masks' lane sets `active` and
 *       `partial` must be the lanes that hold a strip / a strip of fewer than C rows);
 *   (b) every lane's hl[], f[], row maxima and arg-max columns, hout, eout (and the strip bookkeeping) must be equal bit for bit.
 * Shapes: the grid of (w, tlen, qlen) around every boundary of the schedule for each packed geometry -- bands from 0 to the
 * largest one geom_fits admits once lanes take a second strip (a lane's next strip then starts one step after its last one ends),
 * targets of one row to two rounds of strips and a bit, queries shorter, equal and longer --, groups of different shapes in one
 * wavefront where G < 64, and random shapes on top.
 *
 * A stand-alone program: g++ -O1 -fsanitize=address,undefined -pthread -I ksw2_amd/csrc tests/rowmask/rowmask_check.cpp && ./a.out
 * prints one line per geometry and returns 0 when every check held.  usage: a.out [random shapes per geometry] [threads]; the
 * wavefronts of a geometry are independent and are spread over the threads (each draws its sequences from its own index).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>
#include "ksw2_lane_pk.h"
#include "ksw2_lane_rowmask.h"

struct Shape { int qlen, tlen_full, w; };

static thread_local uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
	g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
	return (uint32_t)(g_rng >> 32);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

static K2aScoring scoring()
{
	K2aScoring sc;
	memset(&sc, 0, sizeof(sc));
	sc.q = 4; sc.e = 2; sc.m = 5; sc.pk_smax = 2;                  /* match 2, mismatch -4, wildcard -1 */
	for (int q = 0; q < 5; ++q)
		for (int t = 0; t < 4; ++t) sc.cp[q] |= (uint32_t)(q == 4 ? 3 : q == t ? 0 : 6) << (8 * t);
	return sc;
}

static std::atomic<long> g_steps, g_usteps, g_rowbits, g_edge_steps;
static int g_threads = 1;

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return false; } while (0)

/* one wavefront: group g of 64 / G runs the pair of shape sh[g] (both alignments of a packed task share the shape) */
template<int G, int C>
static bool run_wave(const Shape *sh, int ngroups)
{
	constexpr int NG = 64 / G;
	typedef K2aLanePk<G, C, false, K2A_MODE_SCORE, true, false, 0, false, false> Lane;
	const K2aScoring sc = scoring();
	std::vector<Lane> A(64), B(64);
	K2aPair pr[NG][2];
	std::vector<uint8_t> seq;
	for (int g = 0; g < NG; ++g) {
		const Shape s = sh[g < ngroups ? g : 0];
		for (int h = 0; h < 2; ++h) {
			K2aPair &p = pr[g][h];
			memset(&p, 0, sizeof(p));
			p.qlen = s.qlen; p.tlen_full = s.tlen_full; p.w = s.w;
			p.tlen = s.qlen + s.w < s.tlen_full ? s.qlen + s.w : s.tlen_full;       /* rows that own an in-band cell (ksw2_host_single.c) */
			p.zdrop = -1;
			p.qoff = (uint32_t)seq.size();
			for (int x = 0; x < s.qlen; ++x) seq.push_back((uint8_t)(rnd() % 100 < 3 ? 4 : rnd() & 3));
			seq.resize(seq.size() + 8, 0);
			p.toff = (uint32_t)seq.size();
			uint32_t base = p.qoff;
			for (int x = 0; x < s.tlen_full; ++x) {                                  /* mostly the query again: real scores, not all -inf */
				const uint32_t r = rnd() % 100;
				uint8_t c = (x < s.qlen && r >= 10) ? seq[base + x] : (uint8_t)(rnd() & 3);
				seq.push_back(c > 3 ? 0 : c);
			}
			seq.resize(seq.size() + C + 8, 0);
		}
	}
	seq.resize(seq.size() + 64, 0);

	K2aBook bookA[NG][2], bookB[NG][2];
	uint32_t stage[K2A_PK_STAGE(C)];
	int kmax = -1, ktop = -1;
	bool valid[64];
	for (int l = 0; l < 64; ++l) {
		const int g = l / G, gl = l % G;
		valid[l] = g < ngroups;
		A[l].lrow = 0;
		A[l].setup(pr[g][0], pr[g][1], seq.data(), gl, valid[l], sc.cp);
		A[l].load_query_group(0, A[l].knext == 0 ? A[l].koff_next : A[l].koff, A[l].qwA, A[l].qwB);
		B[l] = A[l];
		if (gl == 0) { k2a_book_reset(&bookA[g][0]); k2a_book_reset(&bookA[g][1]); k2a_book_reset(&bookB[g][0]); k2a_book_reset(&bookB[g][1]); }
		if (A[l].last_step() > kmax) kmax = A[l].last_step();
		if (valid[l]) {
			const int kt = k2a_min(pr[g][0].qlen - 1, k2a_min(C - 1, pr[g][0].tlen - 1) + pr[g][0].w);
			if (kt > ktop) ktop = kt;
		}
	}
	K2aRowMasks<C> RM;
	RM.reset();
	uint32_t qpaA[64], qpbA[64], qpaB[64], qpbB[64];
	long steps = 0, refreshed = 0, rowbits = 0, edge_steps = 0;
	for (int k = 0; k <= kmax; ++k) {
		k2a_pk hinA[64], einA[64], hinB[64], einB[64];
		int bsAA[64], bsBA[64], bsAB[64], bsBB[64];
		for (int l = 0; l < 64; ++l) {
			const int src = (l / G) * G + (l % G + G - 1) % G;
			hinA[l] = A[src].hout; einA[l] = A[src].eout; bsAA[l] = A[src].baseA; bsBA[l] = A[src].baseB;
			hinB[l] = B[src].hout; einB[l] = B[src].eout; bsAB[l] = B[src].baseA; bsBB[l] = B[src].baseB;
		}
		/* strips that start at this step */
		uint64_t initmask = 0;
		for (int l = 0; l < 64; ++l) {
			if (A[l].need_init(k) != B[l].need_init(k)) FAIL("step %d lane %d: the copies disagree on need_init", k, l);
			if (!B[l].need_init(k)) continue;
			initmask |= 1ull << l;
			A[l].do_init(sc, bsAA[l], bsBA[l]); if (k & 3) A[l].reload_query_group(k);
			B[l].do_init(sc, bsAB[l], bsBB[l]); if (k & 3) B[l].reload_query_group(k);
		}
		/* the masks, as k2a_fill_pk_body feeds them */
		{
			uint64_t inband = 0, partmask = 0, col0mask = 0;
			for (int l = 0; l < 64; ++l) {
				const int dd = k - B[l].kd;
				if ((uint32_t)(dd + B[l].w) <= (uint32_t)(2 * B[l].w)) inband |= 1ull << l;
				if (((initmask >> l) & 1) && B[l].rows_m1 != C - 1) partmask |= 1ull << l;
				if (((initmask >> l) & 1) && B[l].i0 <= B[l].w) col0mask |= 1ull << l;
			}
			if (initmask != 0) RM.on_init(initmask, partmask, col0mask);
			RM.advance(inband);
			if (RM.needs_refresh()) {
				uint64_t lv[C];
				for (int c = 0; c < C; ++c) {
					lv[c] = 0;
					for (int l = 0; l < 64; ++l) {
						const int dd = k - B[l].kd, lo = k2a_max(0, dd - B[l].w), hi = k2a_min(B[l].rows_m1, dd + B[l].w);
						if (lo <= c && c <= hi) lv[c] |= 1ull << l;
					}
				}
				RM.refresh(lv);
				++refreshed;
			}
		}
		/* (a) the masks against every lane's own band test, and the lane sets against the lanes */
		bool edge = false;
		for (int l = 0; l < 64; ++l) {
			const bool lact = A[l].rows_m1 >= 0, lpart = lact && A[l].rows_m1 != C - 1;
			if (((RM.active >> l) & 1) != (uint64_t)lact || ((RM.partial >> l) & 1) != (uint64_t)lpart)
				FAIL("step %d lane %d: active %d partial %d, rows_m1 %d", k, l, (int)((RM.active >> l) & 1), (int)((RM.partial >> l) & 1), A[l].rows_m1);
			K2aRowPredLane rp;
			rp.begin(k - A[l].kd, A[l].w, A[l].rows_m1);
			for (int c = 0; c < C; ++c) {
				const uint32_t want = (rp.live >> c) & 1u, got = (uint32_t)((RM.m[c] >> l) & 1u);
				if (want != got)
					FAIL("mask: step %d lane %d row %d: per-lane %u, uniform %u  (G %d C %d; qlen %d tlen %d w %d; S %d i0 %d kd %d rows_m1 %d)",
					     k, l, c, want, got, G, C, A[l].qlen, A[l].tlen, A[l].w, A[l].S, A[l].i0, A[l].kd, A[l].rows_m1);
			}
			rowbits += C;
			edge |= rp.live != 0 && rp.live != (C >= 32 ? ~0u : (1u << C) - 1u);
		}
		edge_steps += edge;
		++steps;
		/* the step, both forms */
		uint64_t finmask = 0;
		for (int l = 0; l < 64; ++l) {
			uint32_t tw[Lane::TBWORDS];
			k2a_pk e2 = 0;
			A[l].hu_prev = hinA[l]; hinA[l] = k2a_pk_add(hinA[l], A[l].delta); einA[l] = k2a_pk_add(einA[l], A[l].delta);
			B[l].hu_prev = hinB[l]; hinB[l] = k2a_pk_add(hinB[l], B[l].delta); einB[l] = k2a_pk_add(einB[l], B[l].delta);
			if ((k & 3) == 0) {
				A[l].load_query_group(k + 4, A[l].knext <= k + 4 ? A[l].koff_next : A[l].koff, qpaA[l], qpbA[l]);
				B[l].load_query_group(k + 4, B[l].knext <= k + 4 ? B[l].koff_next : B[l].koff, qpaB[l], qpbB[l]);
			}
			A[l].set_qb(Lane::query_pick(A[l].qwA, A[l].qwB, k & 3));
			B[l].set_qb(Lane::query_pick(B[l].qwA, B[l].qwB, k & 3));
			if (k <= ktop) { A[l].top_inputs(sc, k, hinA[l], einA[l], e2); B[l].top_inputs(sc, k, hinB[l], einB[l], e2); }
			const bool liveA = A[l].step(sc, k, hinA[l], einA[l], 0u, tw);
			K2aRowPredUniform<C> rp(RM, l);
			const bool liveB = B[l].step_rows(sc, k, hinB[l], einB[l], 0u, tw, rp);
			if (liveA != liveB) FAIL("step %d lane %d: live %d / %d", k, l, (int)liveA, (int)liveB);
			if (B[l].need_fin(k)) finmask |= 1ull << l;
		}
		/* (b) the lane state, bit for bit */
		for (int l = 0; l < 64; ++l) {
			const Lane &a = A[l], &b = B[l];
			const bool same = !memcmp(a.hl, b.hl, sizeof(a.hl)) && !memcmp(a.f, b.f, sizeof(a.f)) && !memcmp(a.rmax_, b.rmax_, sizeof(a.rmax_)) &&
			                  !memcmp(a.rmj_, b.rmj_, sizeof(a.rmj_)) && a.hout == b.hout && a.eout == b.eout && a.hd0 == b.hd0 &&
			                  a.baseA == b.baseA && a.baseB == b.baseB && a.delta == b.delta && a.S == b.S && a.kfin == b.kfin && a.rows_m1 == b.rows_m1;
			if (!same)
				FAIL("state: step %d lane %d differs  (G %d C %d; qlen %d tlen %d w %d; S %d i0 %d)", k, l, G, C, a.qlen, a.tlen, a.w, a.S, a.i0);
		}
		/* strips that end at this step: the sequential epilogue of the re-based kernels */
		if (finmask != 0) {
			bool gfin[NG];
			for (int g = 0; g < NG; ++g) gfin[g] = false;
			RM.on_fin(finmask);
			for (int l = 0; l < 64; ++l) {
				if (!((finmask >> l) & 1)) continue;
				const int g = l / G;
				if (gfin[g]) FAIL("step %d: two strips of group %d end at once", k, g);
				gfin[g] = true;
				if (!A[l].fin_fast(sc, &bookA[g][0], &bookA[g][1], -1, -1)) { A[l].stage_rows(stage); A[l].do_fin_seq(sc, &bookA[g][0], &bookA[g][1], -1, -1, stage); }
				if (!B[l].fin_fast(sc, &bookB[g][0], &bookB[g][1], -1, -1)) { B[l].stage_rows(stage); B[l].do_fin_seq(sc, &bookB[g][0], &bookB[g][1], -1, -1, stage); }
			}
		}
		if ((k & 3) == 3)
			for (int l = 0; l < 64; ++l) { A[l].qwA = qpaA[l]; A[l].qwB = qpbA[l]; B[l].qwA = qpaB[l]; B[l].qwB = qpbB[l]; }
	}
	for (int g = 0; g < ngroups; ++g)
		for (int h = 0; h < 2; ++h) {
			const K2aBook &a = bookA[g][h], &b = bookB[g][h];
			if (a.max != b.max || a.max_t != b.max_t || a.max_q != b.max_q || a.mqe != b.mqe || a.mqe_t != b.mqe_t || a.mte != b.mte ||
			    a.mte_q != b.mte_q || a.score != b.score || a.rows != b.rows)
				FAIL("book: group %d half %d differs (G %d C %d; qlen %d tlen %d w %d)", g, h, G, C, sh[g].qlen, sh[g].tlen_full, sh[g].w);
			if (a.rows != pr[g][0].tlen) FAIL("book: group %d saw %d rows of %d", g, a.rows, pr[g][0].tlen);
		}
	g_steps += steps; g_usteps += steps - refreshed; g_rowbits += rowbits; g_edge_steps += edge_steps;
	return true;
}

/* what the plan admits for a (G, C) array: every strip resident at once, or a lane is done with strip S before strip S + G starts
 * (geom_fits, ksw2_host_plan.c); the band as the host resolves it (ksw2_host_single.c) */
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

template<int G, int C>
static bool run_geometry(int nrandom)
{
	constexpr int NG = 64 / G;
	const int wmax = (G * (C + 1) - C) / 2, GC = G * C;
	const int ws[] = { 0, 1, C - 1, C, C + 1, 2 * C, wmax / 2, wmax - 1, wmax };
	const int tls[] = { 1, C - 1, C, C + 1, 2 * C + 3, GC - 1, GC, GC + 1, 2 * GC + 5 };
	std::vector<Shape> shapes;
	for (int w : ws)
		for (int tl : tls) {
			const int qls[] = { 1, 2, C, tl, tl - w, tl / 3, tl + w + 3, 2 * tl + 7 };
			for (int ql : qls) {
				Shape s = { ql, tl, w };
				if (!admit<G, C>(s)) continue;
				bool dup = false;                                   /* (w = 0: tl - w is tl again; a band wider than both sequences is clamped) */
				for (const Shape &o : shapes) dup |= o.qlen == s.qlen && o.tlen_full == s.tlen_full && o.w == s.w;
				if (!dup) shapes.push_back(s);
			}
		}
	const size_t ngrid = shapes.size();
	for (int x = 0; x < nrandom; ++x) {
		Shape s;
		s.tlen_full = rnd() % 4 == 0 ? rnd_in(1, 3 * C) : rnd_in(1, 2 * GC + 5);
		s.qlen = rnd() % 4 == 0 ? rnd_in(1, 2 * C) : rnd_in(1, 2 * s.tlen_full + 7);
		s.w = rnd() % 3 == 0 ? rnd_in(0, 2 * C) : rnd() % 3 == 0 ? rnd_in(wmax - 3, wmax) : rnd_in(0, s.tlen_full + s.qlen);
		if (admit<G, C>(s)) shapes.push_back(s);
	}
	g_steps = 0; g_usteps = 0; g_rowbits = 0; g_edge_steps = 0;
	/* G = 64: one shape per wavefront.  G < 64: NG different shapes per wavefront, twice -- neighbours in the list, and the list
	 * against itself in strides of 37 (a short pair next to a long one) */
	std::vector<std::vector<Shape> > waves;
	if (NG == 1)
		for (const Shape &s : shapes) waves.push_back(std::vector<Shape>(1, s));
	else
		for (int stride = 1; stride <= 37; stride += 36)
			for (size_t at = 0; at < shapes.size(); at += NG) {
				std::vector<Shape> sh;
				for (int g = 0; g < NG && (stride > 1 || at + g < shapes.size()); ++g) sh.push_back(shapes[(at + (size_t)g * stride) % shapes.size()]);
				waves.push_back(sh);
			}
	std::atomic<size_t> next(0);
	std::atomic<bool> ok(true);
	auto work = [&]() {
		for (size_t x; ok && (x = next++) < waves.size(); ) {
			g_rng = 0x9E3779B97F4A7C15ull * (x + 1) + (uint64_t)(G * 131 + C);
			if (!run_wave<G, C>(waves[x].data(), (int)waves[x].size())) ok = false;
		}
	};
	std::vector<std::thread> th;
	for (int t = 1; t < g_threads; ++t) th.emplace_back(work);
	work();
	for (std::thread &t : th) t.join();
	if (!ok) return false;
	printf("(%d,%d): %zu grid shapes + %zu random, %zu wavefronts, %ld steps (%ld on shifted masks alone, %ld with a lane at a band edge), %ld row bits: masks and lane state agree\n",
	       G, C, ngrid, shapes.size() - ngrid, waves.size(), g_steps.load(), g_usteps.load(), g_edge_steps.load(), g_rowbits.load());
	return true;
}

int main(int argc, char **argv)
{
	const int nrandom = argc > 1 ? atoi(argv[1]) : 24;
	const int hw = (int)std::thread::hardware_concurrency();
	g_threads = argc > 2 ? atoi(argv[2]) : hw < 1 ? 1 : hw > 16 ? 16 : hw;
	bool ok = run_geometry<64, 16>(nrandom) && run_geometry<8, 18>(8 * nrandom) && run_geometry<16, 8>(4 * nrandom) && run_geometry<64, 8>(nrandom);
	if (ok) printf("rowmask check ok\n");
	return ok ? 0 : 1;
}
