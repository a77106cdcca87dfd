"""GPU: the deferred one-group fills in the pair-maximum form (K2aLanePk PM, ksw2_lane_pk.h: one running maximum per pair of rows, the
row and its column resolved by the second pass; k2a_pkfold_task_pm, ksw2_lane_pkfold.h) against the oracle on all fields.

A class takes the form iff each of its pairs has zdrop < 0 or zdrop >= 4 * slack, slack = delta + q, delta = max(smax + q + e, -smin,
q + e) over the matrix with its wildcard entries (ksw2_host_plan.c): 48 under the preset scoring, 216 under the "deep" one.  Per
geometry -- (64, 16) with targets of 1 025 and 2 053 rows, (64, 8) with 513 and 1 029; bands 0, C, C + 1 and the widest the geometry
admits -- and scoring -- the preset, the preset with wildcard runs in the targets (the TN build), "deep" (re-based; bands up to 100, the
widest does not fit the 16-bit window there) -- one batch at
the threshold and without a Z-drop (the form: asserted from describe()) and one a unit below it (the per-row form: asserted).  Per shape
eight pairs, four tasks:
  - a healthy read without a Z-drop and one under it;
  - a read whose maximum is reached again two rows on, again and again over more than a strip (a mismatch and two matches behind the
    best cell, repeated), with and without a Z-drop: the first row wins;
  - reads that leave their target in the first strip, in a middle strip and 2 * zdrop rows before the end (the last six or twelve strips), under the Z-drop;
  - a read with a run of mismatches that takes it further than zdrop - slack and no further than zdrop below its maximum (the run
    is long enough that a pair of gaps around it costs as much): the new fold freezes its book, nothing drops (asserted on the result).
Every ksw_extz_t field is compared, and the plan is run a second time on its recycled buffers: the same records."""
import numpy as np
import pytest

import ksw2_amd as ka
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import hlopen_util as hu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

G = 64
ENV = {"KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": 1}
GEOMS = {16: 3, 8: 2}                                   # C -> KSW2AMD_PK_FIRST index


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                                    # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def slack_of(scoring):
    mat, m, q, e = hu.SCORINGS[scoring][:4]
    mat = np.asarray(mat, dtype=np.int64)
    return max(int(mat.max()) + q + e, -int(mat.min()), q + e) + q


def read_of(rng, t, ql, kind, C, mis, slack, zd, gq, ge):
    """A query of ql bases off target t (3 % substitutions; cut, or padded with random bases)."""
    sub = rng.random(len(t)) < 0.03
    q = np.where(sub, (t + rng.integers(1, 4, len(t))) & 3, t).astype(np.uint8)
    if len(q) < ql:
        q = np.concatenate([q, rng.integers(0, 4, ql - len(q), dtype=np.uint8)])
    q = np.ascontiguousarray(q[:ql])
    n = min(ql, len(t))
    if kind == "again":
        # clean up to the best cell, then (mismatch, match, match) over a strip and a half -- back at the maximum every third row,
        # never above it (2 + 2 = 4; under another scoring just a repeat structure) --, random behind
        peak = min(n - 1, 5 * C + 3)
        q[:n] = t[:n]
        end = min(n, peak + 1 + 3 * ((3 * C // 2 + 2) // 3))
        for x in range(peak + 1, end, 3):
            q[x] = (t[x] + 1) & 3
        q[end:] = rng.integers(0, 4, ql - end, dtype=np.uint8)
    elif kind in ("first", "middle", "last"):
        at = {"first": min(C // 2, ql - 1), "middle": ql // 2, "last": max(0, n - max(2 * C + C // 2, 2 * zd))}[kind]
        q[at:] = rng.integers(0, 4, ql - at, dtype=np.uint8)
        if kind == "last":                              # ... 2 * zdrop rows of certain mismatches on the diagonal: the drop comes in the last strips
            q[at:n] = (t[at:n] + 2) & 3
    elif kind == "dip":
        # clean, with one run of mismatches in the middle: crossing it, or going round it with a gap on either side, costs more than
        # zd - slack and no more than zd
        cost = lambda k: min(mis * k, 2 * (gq + ge * k))
        nm = next(k for k in range(1, 400) if cost(k) > zd - slack)
        assert zd - slack < cost(nm) <= zd
        q[:n] = t[:n]
        at = n // 2
        q[at:at + nm] = (t[at:at + nm] + 1) & 3
    return q


KINDS = [("healthy", 0), ("healthy", 1), ("again", 0), ("again", 1), ("first", 1), ("middle", 1), ("last", 1), ("dip", 1)]


def batch(seed, C, scoring, shapes, zd, wild):
    mat, m, q, e = hu.SCORINGS[scoring][:4]
    mis, slack = -int(np.asarray(mat).min()), slack_of(scoring)
    rng = np.random.Generator(np.random.PCG64(seed))
    qs, ts, ws, zs, kinds = [], [], [], [], []
    for ql, tl, w in shapes:
        for kind, z in KINDS:
            t = rng.integers(0, 4, tl, dtype=np.uint8)
            qs.append(read_of(rng, t, ql, kind, C, mis, slack, zd, q, e)); ts.append(t); ws.append(w); zs.append(zd if z else -1); kinds.append(kind)
    if wild:
        ts = pu.sprinkle_target_wildcards(rng, ts, every=2, runs=(1, 50))
    return qs, ts, np.array(ws), np.array(zs), kinds


def run(lib, setenv, delenv, C, scoring, shapes, zd, wild, want_pm, seed):
    mat, m, q, e = hu.SCORINGS[scoring][:4]
    qs, ts, ws, zs, kinds = batch(seed, C, scoring, shapes, zd, wild)
    eu.set_env(setenv, delenv, dict(ENV, KSW2AMD_PK_FIRST=GEOMS[C]))
    p = lib.make_batch(qs, ts, mat, q, e, 0, 0, w=ws, zdrop=zs, flag=po.SCORE_ONLY, m=m).plan(False)
    try:
        d, npk = p.describe(), p.packed_pairs()
        assert d and npk == len(qs) and all(c["kernel"] == "pk" and (c["G"], c["C"]) == (G, C) and c["mode"] == "score" and c["form"] == "defer" and
                                             c["nomax"] == 0 and c["pairmax"] == want_pm for c in d), (scoring, zd, npk, len(qs), d)
        if scoring == "deep":
            assert all(c["rebased"] == 1 for c in d), d
        if wild:
            assert all(c["tn"] == 1 for c in d), d
        p.run()
        got, raw1 = p.fetch(), p.fetch_raw().copy()
        p.run()                                         # ... again, on the buffers the first run left behind
        raw2 = p.fetch_raw().copy()
    finally:
        p.close()
    assert (raw1 == raw2).all(), np.flatnonzero((raw1 != raw2).any(axis=1))[:8]
    ndrop = 0
    for i in range(len(qs)):
        exp = po.align("oracle", "extz2", qs[i], ts[i], mat, q, e, 0, 0, w=int(ws[i]), zdrop=int(zs[i]), flag=po.SCORE_ONLY, m=m)
        bad = pu.diff(exp, got[i], pu.CMP_FIELDS)
        assert not bad, ("pair %d (%s) C=%d %s w=%d zdrop=%d qlen=%d tlen=%d" % (i, kinds[i], C, scoring, ws[i], zs[i], len(qs[i]), len(ts[i])),
                         {k: (exp[k], got[i][k]) for k in bad})
        ndrop += exp["zdropped"]
        # (under "deep" the run is 64 long and cheaper to go round: only a band that admits the two gaps keeps the read alive)
        if kinds[i] == "dip" and not wild and (ws[i] > 0 if scoring == "preset" else ws[i] >= 100) and len(qs[i]) == len(ts[i]):
            assert exp["zdropped"] == 0, (i, exp)        # frozen by the new fold's rule at most: the read recovers
        # (under "deep" a long gap costs 1 per base: the last strips alone do not take a read 216 below its maximum)
        if kinds[i] in ("first", "middle", "last") and not wild and len(qs[i]) >= len(ts[i]) and not (kinds[i] == "last" and scoring == "deep"):
            assert exp["zdropped"] == 1, (i, kinds[i], exp)
    assert ndrop >= len(shapes), (ndrop, len(shapes))


def shapes_of(C, long_too):
    wmax = (G * (C + 1) - C) // 2
    tl1, tl2 = G * C + 1, 2 * G * C + 5
    s = [(tl1, tl1, 0), (tl1, tl1, C), (tl1 + 3, tl1, C + 1), (tl1, tl1, wmax)]
    if long_too:
        s += [(tl2, tl2, C + 1), (tl2 - 20, tl2, wmax)]
    return s


@pytest.mark.parametrize("C", [16, 8])
@pytest.mark.parametrize("scoring,wild", [("preset", False), ("preset", True)])
def test_stripmax_preset(lib, monkeypatch, C, scoring, wild):
    thr = 4 * slack_of(scoring)
    assert thr == 48
    run(lib, monkeypatch.setenv, monkeypatch.delenv, C, scoring, shapes_of(C, True), thr, wild, thr // 4, 9600 + C + wild)
    run(lib, monkeypatch.setenv, monkeypatch.delenv, C, scoring, shapes_of(C, False)[1:3], thr - 1, wild, 0, 9650 + C + wild)


@pytest.mark.parametrize("C", [16, 8])
def test_stripmax_rebased(lib, monkeypatch, C):
    thr = 4 * slack_of("deep")
    assert thr == 216
    # the widest band of the geometry does not fit the 16-bit window under this scoring (the plan sends it to the int32 kernels): bands 0,
    # C, C + 1 and 100 on the short target, C + 1 and 100 on the long one
    tl1, tl2 = G * C + 1, 2 * G * C + 5
    shapes = [(tl1, tl1, 0), (tl1, tl1, C), (tl1 + 3, tl1, C + 1), (tl1, tl1, 100), (tl2, tl2, C + 1), (tl2 - 20, tl2, 100)]
    run(lib, monkeypatch.setenv, monkeypatch.delenv, C, "deep", shapes, thr, False, thr // 4, 9700 + C)
    run(lib, monkeypatch.setenv, monkeypatch.delenv, C, "deep", [shapes[2], shapes[5]], thr - 1, False, 0, 9750 + C)
