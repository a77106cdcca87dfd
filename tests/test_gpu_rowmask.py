"""GPU: the score-only packed fills with wavefront-uniform row masks (ksw2_amd/csrc/ksw2_lane_rowmask.h) against the oracle, on the
shape grid of tests/rowmask/rowmask_check.cpp -- (w, tlen, qlen) around every boundary of the strip schedule -- for each packed
geometry, forced through KSW2AMD_PK_FIRST and asserted from the plan's description, under every form of the fill: deferred arg-max or
not, row selectors in LDS or registers, exact and KSW_EZ_APPROX_MAX, without a Z-drop and with one that fires (which sends pairs of a
uniform-mask fill through the per-lane second and third passes), plus one uniform streamed plan and one flat batch.

Every pair is compared on all fields (tests/parity_util.check_batch).  The oracle's records depend on the pair and its parameters
only, not on the form that ran, so they are computed once per (pair, w, zdrop, flag) and shared by the forms (a memo around
oracle.pyoracle.align for the time of a test)."""
import numpy as np
import pytest

import ksw2_amd as ka
from ksw2_amd import synth
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

GEOMS = [(8, 18), (16, 8), (64, 8), (64, 16)]        # KSW2AMD_PK_FIRST = index
LDSCODE_GEOMS = {(64, 16), (8, 18), (16, 8)}         # K2A_PK_LDSCODES (ksw2_lane_pk.h)
MAT = synth.simple_mat(5, 2, 4, -1)
GQ, GE = 4, 2
ZDROP_GRID = 50                                      # grid pairs carry 5 % substitutions and 6 % indels: fires on some, not on all


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def grid_shapes(G, C):
    """The grid of tests/rowmask/rowmask_check.cpp (run_geometry / admit): (qlen, tlen, w) with the band clamped as the host does and
    kept where the (G, C) array holds it."""
    wmax, GC, out = (G * (C + 1) - C) // 2, G * C, []
    for w in (0, 1, C - 1, C, C + 1, 2 * C, wmax // 2, wmax - 1, wmax):
        for tl in (1, C - 1, C, C + 1, 2 * C + 3, GC - 1, GC, GC + 1, 2 * GC + 5):
            for ql in (1, 2, C, tl, tl - w, tl // 3, tl + w + 3, 2 * tl + 7):
                if ql < 1:
                    continue
                ww = min(w, max(ql, tl))
                nstrips = (min(tl, ql + ww) + C - 1) // C
                if (nstrips <= G or 2 * ww < G * (C + 1) - C + 1) and (ql, tl, ww) not in out:
                    out.append((ql, tl, ww))
    return out


def mutated(rng, t, ql):
    """A query of ql bases off target t: 5 % substitutions, 6 % indels (half each), cut or padded with random bases."""
    u = rng.random(len(t))
    keep = np.where(u < 0.03, 0, 1)                                   # deletions
    ins = (u >= 0.03) & (u < 0.06)                                    # an inserted base behind the position
    sub = (u >= 0.06) & (u < 0.11)
    b = np.where(sub, (t + rng.integers(1, 4, len(t))) & 3, t).astype(np.uint8)
    rep = keep + ins
    q = np.repeat(b, rep)
    first = np.cumsum(rep) - rep                                      # a doubled position: the second copy is the insertion
    extra = first[ins & (keep == 1)] + 1
    q[extra] = rng.integers(0, 4, len(extra), dtype=np.uint8)
    if len(q) < ql:
        q = np.concatenate([q, rng.integers(0, 4, ql - len(q), dtype=np.uint8)])
    return np.ascontiguousarray(q[:ql])


_BATCH = {}


def grid_batch(gi):
    """Every grid shape of geometry gi twice (a packed task is two pairs of one shape), then a few edge_util.zdrop_pairs pairs of one
    square shape with their own critical Z-drop minus one: (queries, targets, w per pair, zdrop per pair for the Z-drop runs)."""
    if gi in _BATCH:
        return _BATCH[gi]
    G, C = GEOMS[gi]
    rng = np.random.Generator(np.random.PCG64(9100 + gi))
    qs, ts, ws, zs = [], [], [], []
    for ql, tl, w in grid_shapes(G, C):
        for _ in range(2):
            t = rng.integers(0, 4, tl, dtype=np.uint8)
            qs.append(mutated(rng, t, ql)); ts.append(t); ws.append(w); zs.append(ZDROP_GRID)
    ngrid = len(qs)
    wz = min(40, (G * (C + 1) - C) // 2)
    zq, zt = eu.same_shape(*eu.zdrop_pairs(9200 + gi, 8, 0.5))
    fired = 0
    for i in range(len(zq)):
        z = eu.critical_zdrop(lambda zz: po.align("oracle", "extz2", zq[i], zt[i], MAT, GQ, GE, w=wz, zdrop=zz, flag=po.SCORE_ONLY)["zdropped"] == 1)
        qs.append(zq[i]); ts.append(zt[i]); ws.append(wz); zs.append(z - 1 if z else 0)
        fired += 1 if z else 0
    assert fired >= 2, fired                                          # "a zdrop that fires on a few pairs"
    _BATCH[gi] = (qs, ts, np.array(ws), np.array(zs), ngrid)
    return _BATCH[gi]


_MEMO = {}


@pytest.fixture
def shared_oracle(monkeypatch):
    """oracle.pyoracle.align with a memo per (sequences, every argument): one reference per pair and parameter set for all forms"""
    real = po.align

    def align(impl, func, q, t, *a, **kw):
        key = (impl, func, np.asarray(q).tobytes(), np.asarray(t).tobytes(), tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in a),
               tuple(sorted(kw.items())))
        if key not in _MEMO:
            _MEMO[key] = real(impl, func, q, t, *a, **kw)
        return _MEMO[key]

    monkeypatch.setattr(po, "align", align)


def expected_form(G, C, defer, ldscodes, approx):
    if defer and not approx:
        return "defer"
    return "ldscodes" if ldscodes and (G, C) in LDSCODE_GEOMS else "registers"


def run_forced(lib, monkeypatch, gi, defer, ldscodes, approx, zdrop_on):
    G, C = GEOMS[gi]
    qs, ts, ws, zs, _ = grid_batch(gi)
    flag = po.SCORE_ONLY | (po.APPROX_MAX if approx else 0)
    zd = zs if zdrop_on else -1
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_PK_FIRST": gi, "KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": defer,
                                                       "KSW2AMD_LDSCODES": ldscodes})
    p = lib.make_batch(qs, ts, MAT, GQ, GE, w=ws, zdrop=zd, flag=flag).plan(False)
    d, npk = p.describe(), p.packed_pairs()
    p.close()
    want = expected_form(G, C, defer, ldscodes, approx)
    assert d and npk == len(qs) and all(c["kernel"] == "pk" and (c["G"], c["C"]) == (G, C) and c["mode"] == "score" and c["form"] == want and
                                         c["nomax"] == int(approx) for c in d), ((G, C), defer, ldscodes, approx, zdrop_on, npk, len(qs), d)
    n, res = pu.check_batch(lib, False, qs, ts, MAT, GQ, GE, 0, 0, w=ws, zdrop=zd, flag=flag)
    assert n == len(qs)
    return res


@pytest.mark.parametrize("approx", [False, True], ids=["exact", "approx"])
@pytest.mark.parametrize("gi", range(4), ids=["G%dC%d" % g for g in GEOMS])
def test_rowmask_grid_forms(lib, monkeypatch, shared_oracle, gi, approx):
    nz = 0
    for zdrop_on in (False, True):
        for defer in ((0,) if approx else (0, 1)):                    # (the kernels without maximum tracking have no deferred form)
            for ldscodes in (0, 1):
                res = run_forced(lib, monkeypatch, gi, defer, ldscodes, approx, zdrop_on)
                if zdrop_on:
                    nz = sum(r["zdropped"] for r in res)
    qs, _, _, _, ngrid = grid_batch(gi)
    if not approx:                                                    # the Z-drop fired on grid pairs and on the pairs built for it
        assert nz >= 3 and nz < len(qs), nz


def test_rowmask_uniform_streamed_and_flat(lib, monkeypatch, shared_oracle):
    """One shape, 128 pairs, through a uniform streamed plan (the QUEUE build of the fill) and the same pairs as a flat batch."""
    G, C = 64, 16
    ql, tl, w = G * C + 1, G * C + 1, C + 1
    rng = np.random.Generator(np.random.PCG64(9300))
    ts = rng.integers(0, 4, (8, tl), dtype=np.uint8)
    qs = np.stack([mutated(rng, t, ql) for t in ts])
    QS, TS = np.tile(qs, (16, 1)), np.tile(ts, (16, 1))
    flag = po.SCORE_ONLY
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_UNIFORM": 1, "KSW2AMD_STREAM": 1, "KSW2AMD_STREAM_PIECE_KB": 64, "KSW2AMD_SIMDS": 0,
                                                       "KSW2AMD_SOLO": 0})
    s0 = lib.stream_stats()
    n, _ = pu.check_batch(lib, False, QS, TS, MAT, GQ, GE, 0, 0, w=w, zdrop=ZDROP_GRID, flag=flag)
    assert n == len(QS) and lib.stream_stats()["streamed_plans"] - s0["streamed_plans"] == 1, "the uniform streamed plan did not run"
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0})
    fres = lib.make_flat_batch(QS, TS, MAT, GQ, GE, 0, 0, w=w, zdrop=ZDROP_GRID, end_bonus=0, flag=flag).run_oneshot(False)
    exp = pu.oracle_batch(False, QS, TS, MAT, GQ, GE, 0, 0, w, ZDROP_GRID, 0, flag)
    bad = [(i, pu.diff(exp[i], fres[i])) for i in range(len(QS)) if pu.diff(exp[i], fres[i])]
    assert not bad, ("flat", bad[:3])
