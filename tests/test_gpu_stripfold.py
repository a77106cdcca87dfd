"""GPU: the deferred fills' strip ends folded behind the step loop (ksw2_lane_pkfold.h) -- one record per strip in the checkpoint
block, the books folded from them once per task -- against the oracle on all fields.

tests/test_gpu_strip_events.py drives the deferred (64, 16) fill through drops in every place a strip can have; here are the cases
that lie beside it:
  - the deferred (64, 8) geometry (records of half the size), forced and asserted from the plan's description: targets of one and of
    two rounds of 64 strips and a bit, bands 0, C and the widest the geometry admits, half the pairs with a Z-drop that fires and
    half with none;
  - one non-uniform plan whose tasks have different strip counts, so that the blocks -- stream, headers, records -- differ in size
    from task to task (the per-task layout of plan_create_ex);
  - recycled buffers: in one process a batch of a long shape, then one of a shorter shape with drops: the shorter tasks' blocks are
    followed by the longer ones' records, which a fold that reads past its own strips would take up (they hold higher maxima)."""
import numpy as np
import pytest

import ksw2_amd as ka
from ksw2_amd import synth
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

G = 64
MAT = synth.simple_mat(5, 2, 4, -1)
GQ, GE = 4, 2
ZD = 50


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def mutated(rng, t, ql):
    """A query of ql bases off target t: 3 % substitutions, cut or padded with random bases."""
    sub = rng.random(len(t)) < 0.03
    q = np.where(sub, (t + rng.integers(1, 4, len(t))) & 3, t).astype(np.uint8)
    if len(q) < ql:
        q = np.concatenate([q, rng.integers(0, 4, ql - len(q), dtype=np.uint8)])
    return np.ascontiguousarray(q[:ql])


def leaving(rng, t, ql, at):
    """... that leaves its target at column `at`: random from there on, so a Z-drop of ZD fires some rows behind it."""
    q = mutated(rng, t, ql)
    q[at:] = rng.integers(0, 4, ql - at, dtype=np.uint8)
    return q


def shape_pairs(rng, shapes):
    """Per shape (ql, tl, w) four pairs -- two tasks --: two that leave their target under Z-drop ZD, at different places, two without a Z-drop."""
    qs, ts, ws, zs = [], [], [], []
    for ql, tl, w in shapes:
        for i in range(4):
            t = rng.integers(0, 4, tl, dtype=np.uint8)
            ts.append(t); ws.append(w)
            if i < 2:
                qs.append(leaving(rng, t, ql, (ql // 3, ql - ql // 5)[i])); zs.append(ZD)
            else:
                qs.append(mutated(rng, t, ql)); zs.append(-1)
    return qs, ts, np.array(ws), np.array(zs)


def check(lib, qs, ts, ws, zs, want_drops):
    n, res = pu.check_batch(lib, False, qs, ts, MAT, GQ, GE, 0, 0, w=ws, zdrop=zs, flag=po.SCORE_ONLY)
    assert n == len(qs)
    nz = sum(r["zdropped"] for r in res)
    assert nz >= want_drops and any(r["zdropped"] == 0 for r in res), (nz, want_drops)
    return res


def describe(lib, qs, ts, ws, zs):
    p = lib.make_batch(qs, ts, MAT, GQ, GE, w=ws, zdrop=zs, flag=po.SCORE_ONLY).plan(False)
    d, npk = p.describe(), p.packed_pairs()
    p.close()
    return d, npk


def test_stripfold_64x8(lib, monkeypatch):
    C, GI = 8, 2                                         # KSW2AMD_PK_FIRST index of (64, 8)
    wmax = (G * (C + 1) - C) // 2
    rng = np.random.Generator(np.random.PCG64(9500))
    shapes = [(tl, tl, w) for tl in (G * C + 1, 2 * G * C + 5) for w in (0, C, wmax)]
    qs, ts, ws, zs = shape_pairs(rng, shapes)
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_PK_FIRST": GI, "KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": 1})
    d, npk = describe(lib, qs, ts, ws, zs)
    assert d and npk == len(qs) and all(c["kernel"] == "pk" and (c["G"], c["C"]) == (G, C) and c["mode"] == "score" and c["form"] == "defer" and
                                         c["nomax"] == 0 for c in d), (npk, len(qs), d)
    check(lib, qs, ts, ws, zs, len(qs) // 2)            # every pair that leaves its target drops


def test_stripfold_mixed_shapes(lib, monkeypatch):
    C, GI = 16, 3
    rng = np.random.Generator(np.random.PCG64(9510))
    # strip counts 1, 2, 19, 65, 129 and 193 (partial last strips among them), query shorter, equal and longer than the target
    shapes = [(9, 7, 3), (40, 30, 5), (300, 290, 20), (G * C + 1, G * C + 1, C + 1), (2 * G * C - 40, 2 * G * C + 5, 60), (3 * G * C + 30, 3 * G * C + C - 1, 33)]
    qs, ts, ws, zs = shape_pairs(rng, shapes)
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_PK_FIRST": GI, "KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": 1})
    d, npk = describe(lib, qs, ts, ws, zs)
    assert d and npk == len(qs) and all(c["kernel"] == "pk" and (c["G"], c["C"]) == (G, C) and c["form"] == "defer" for c in d), (npk, len(qs), d)
    check(lib, qs, ts, ws, zs, 4)


def test_stripfold_recycled_buffers(lib, monkeypatch):
    C, GI = 16, 3
    rng = np.random.Generator(np.random.PCG64(9520))
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_PK_FIRST": GI, "KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": 1})
    # the longest shape first: clean matches, so every strip's record holds maxima far above anything the second batch reaches
    tl = 3 * G * C + C - 1
    ts = [rng.integers(0, 4, tl, dtype=np.uint8) for _ in range(8)]
    qs = [mutated(rng, t, tl) for t in ts]
    n, res = pu.check_batch(lib, False, qs, ts, MAT, GQ, GE, 0, 0, w=40, zdrop=ZD, flag=po.SCORE_ONLY)
    assert n == len(qs) and all(r["zdropped"] == 0 for r in res)
    # then a shorter shape, half of its pairs dropping: its blocks are carved out of the same buffer
    sl = G * C + 5
    qs2, ts2, ws2, zs2 = shape_pairs(rng, [(sl, sl, 40), (sl, sl, 40)])
    d, npk = describe(lib, qs2, ts2, ws2, zs2)
    assert d and npk == len(qs2) and all(c["form"] == "defer" and (c["G"], c["C"]) == (G, C) for c in d), d
    check(lib, qs2, ts2, ws2, zs2, len(qs2) // 2)
