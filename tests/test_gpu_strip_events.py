"""GPU: the strip events of the packed (64, 16) score-only fill -- strip starts behind the wavefront-uniform column-0 flag
(K2aLanePk::do_init<true>), the rotates without a zeroed destination, the deferred fill's step without its early-stop test -- against
the oracle on all fields.

The geometry is forced through KSW2AMD_PK_FIRST and asserted from the plan's description, with the deferred arg-max on and off and
the row selectors in LDS and in registers.  Shapes: targets of more than one, more than two and more than three rounds of 64 strips,
bands from 0 (no strip but the first has a row at column 0) to the widest the geometry admits (the first 34 strips have one); the
longest shape does not fit the plain 16-bit window and runs re-based, the others run plain.  Z-drop pairs come from
tests/edge_util.zdrop_pairs between a matching prefix, which moves the row at which the oracle drops to a chosen place, and a
matching suffix, each at its own critical Z-drop minus one (drops) and at the critical one (does not).  The row at which the oracle
drops is found from the oracle alone: the scalar recurrence works row by row, so it is the shortest target prefix that still drops
(with the query cut where that prefix's band ends).  The rows are spread over the places a strip can have in a (64, 16) fill: the
first strip of a round of 64 (lane 0), a middle one, the last one (lane 63), the last, incomplete round in front of the strips that
take the row-by-row epilogue, and such a strip (it holds the last target row or reaches the query end); tests/test_strip_events_cpu.py
asserts, without a GPU, that the construction reaches each of them.  Only "takes the row-by-row epilogue or not" is a distinction
the kernel's strip-end code makes today: the others name lanes and rounds, not code paths, and are there to spread the rows.  In a
deferred fill an alignment that drops has its book frozen at or before that row and goes through the second and third passes.

The oracle's records depend on the pair and its parameters only, so they are computed once and shared by the forms."""
import numpy as np
import pytest

import ksw2_amd as ka
from ksw2_amd import synth
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import parity_util as pu

pytestmark = pytest.mark.gpu

G, C = 64, 16
GI = 3                                               # KSW2AMD_PK_FIRST index of (64, 16)
GC = G * C
WMAX = (G * (C + 1) - C) // 2
MAT = synth.simple_mat(5, 2, 4, -1)
GQ, GE = 4, 2
ZLEN, ZW = 3 * GC + C - 1, 40                        # the Z-drop pairs' square shape and band
CLASSES = ("first", "middle", "last", "partial", "immediate")


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


def shape_list():
    out = []
    for tl in (GC + 1, GC + C + 1, 2 * GC + 5, 3 * GC + C - 1):
        for w in (0, C - 1, C, C + 1, 2 * C, WMAX - 1, WMAX):
            for ql in (tl, tl - w, tl + w + 3):
                if ql >= 1 and (ql, tl, w) not in out:
                    out.append((ql, tl, w))
    return out


def strip_class(row, qlen, tlen_full, w):
    """Where the strip of target row `row` stands among the strip ends of a (64, 16) fill of this shape."""
    tlen = min(tlen_full, qlen + w)                                   # rows that own an in-band cell
    imm = lambda s: s * C + C >= tlen or s * C + C - 1 + w >= qlen - 1      # noqa: E731  (fin_fast's first test fails)
    s = row // C
    if imm(s):
        return "immediate"
    if any(imm(x) for x in range(s, (s // G) * G + G)):                # its round does not complete before the first immediate strip
        return "partial"
    return "first" if s % G == 0 else "last" if s % G == G - 1 else "middle"


def oracle_drops(q, t, w, z):
    return po.align("oracle", "extz2", q, t, MAT, GQ, GE, w=w, zdrop=z, flag=po.SCORE_ONLY)["zdropped"] == 1


def drop_row(q, t, w, z):
    """The target row at which the oracle drops (it does, at zdrop z): one less than the shortest target prefix that still drops.
    (A prefix of n rows reads the first n + w columns only; cut there, the band still reaches the corner.)"""
    lo, hi = 0, len(t)                                                # does not drop on lo rows, drops on hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if oracle_drops(q[:mid + w], t[:mid], w, z):
            hi = mid
        else:
            lo = mid
    return hi - 1


_Z = {}


def zdrop_batch():
    """Pairs of tests/edge_util.zdrop_pairs between a matching prefix and a matching suffix, one square shape: (queries, targets,
    zdrop per pair, class of the drop row per pair or None).  Every pair with a critical Z-drop Z* comes twice: at Z* - 1 (drops) and at Z* (does not)."""
    if _Z:
        return _Z["v"]
    rng = np.random.Generator(np.random.PCG64(9400))
    zq, zt = eu.zdrop_pairs(9401, 6, 0.5)
    # rows at which a drop is wanted: the first and the last strip of the second round, the middle of the first, the incomplete
    # third round, the row-by-row strips at the end
    wanted = [64 * C + 5, 127 * C + 9, 30 * C + 3, 150 * C + 7, ZLEN - 30]
    qs, ts, zs, cls = [], [], [], []
    for k in range(len(zq)):
        for want in wanted:
            def build(pre):
                # a matching prefix, the pair cut to one length, a matching suffix: the score recovers behind the pair, so the
                # deepest dip -- the row that decides at the critical Z-drop -- lies inside it
                n = min(len(zq[k]), len(zt[k]), ZLEN - pre)
                p, sfx = rng.integers(0, 4, pre, dtype=np.uint8), rng.integers(0, 4, ZLEN - pre - n, dtype=np.uint8)
                return np.concatenate([p, zq[k][:n], sfx]), np.concatenate([p, zt[k][:n], sfx])
            # the pair alone drops some rows in; move it so that the row lands where it is wanted
            q0, t0 = build(0)
            z0 = eu.critical_zdrop(lambda zz: oracle_drops(q0, t0, ZW, zz))
            if not z0:
                continue
            pre = want - drop_row(q0, t0, ZW, z0 - 1)
            if pre < 0 or pre > ZLEN - 2 * C:
                continue
            q, t = build(pre)
            z = eu.critical_zdrop(lambda zz: oracle_drops(q, t, ZW, zz))
            if not z:
                continue
            r = drop_row(q, t, ZW, z - 1)
            qs += [q, q]; ts += [t, t]; zs += [z - 1, z]; cls += [strip_class(r, ZLEN, ZLEN, ZW), None]
    _Z["v"] = (qs, ts, zs, cls)
    return _Z["v"]


_B = {}


def batch():
    """(queries, targets, w per pair, zdrop per pair, class of the oracle's drop row per pair)"""
    if _B:
        return _B["v"]
    rng = np.random.Generator(np.random.PCG64(9410))
    qs, ts, ws, zs, cls = [], [], [], [], []
    for ql, tl, w in shape_list():
        for i in range(2):                                            # a packed task is two pairs of one shape
            t = rng.integers(0, 4, tl, dtype=np.uint8)
            qs.append(mutated(rng, t, ql)); ts.append(t); ws.append(w); zs.append(-1 if i == 0 else 60); cls.append(None)
    zq, zt, zz, zc = zdrop_batch()
    qs += zq; ts += zt; ws += [ZW] * len(zq); zs += zz; cls += zc
    _B["v"] = (qs, ts, np.array(ws), np.array(zs), cls)
    return _B["v"]


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


@pytest.mark.parametrize("ldscodes", [1, 0], ids=["ldscodes", "registers"])
@pytest.mark.parametrize("defer", [1, 0], ids=["defer", "nodefer"])
def test_strip_events_forms(lib, monkeypatch, shared_oracle, defer, ldscodes):
    qs, ts, ws, zs, _ = batch()
    flag = po.SCORE_ONLY
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_PK_FIRST": GI, "KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": defer,
                                                       "KSW2AMD_LDSCODES": ldscodes})
    p = lib.make_batch(qs, ts, MAT, GQ, GE, w=ws, zdrop=zs, flag=flag).plan(False)
    d, npk = p.describe(), p.packed_pairs()
    p.close()
    want = "defer" if defer else "ldscodes" if ldscodes else "registers"
    assert d and npk == len(qs) and all(c["kernel"] == "pk" and (c["G"], c["C"]) == (G, C) and c["mode"] == "score" and c["form"] == want and
                                         c["nomax"] == 0 for c in d), (defer, ldscodes, npk, len(qs), d)
    assert {c["rebased"] for c in d} == {0, 1}, d                     # the longest shape runs re-based, the others plain
    n, res = pu.check_batch(lib, False, qs, ts, MAT, GQ, GE, 0, 0, w=ws, zdrop=zs, flag=flag)
    assert n == len(qs)
    nz = sum(r["zdropped"] for r in res)
    assert 0 < nz < len(qs), nz


def test_strip_events_uniform_streamed_and_flat(lib, monkeypatch, shared_oracle):
    """One shape of three rounds and a bit, 128 pairs, through a uniform streamed plan (the QUEUE build of the fill) and the same pairs
    as a flat batch."""
    ql = tl = ZLEN
    w = C + 1
    rng = np.random.Generator(np.random.PCG64(9420))
    ts = rng.integers(0, 4, (8, tl), dtype=np.uint8)
    qs = np.stack([mutated(rng, t, ql) for t in ts])
    qs[1, 20 * C:] = rng.integers(0, 4, ql - 20 * C, dtype=np.uint8)  # two queries that leave their target: these drop
    qs[5, 130 * C:] = rng.integers(0, 4, ql - 130 * C, dtype=np.uint8)
    QS, TS = np.tile(qs, (16, 1)), np.tile(ts, (16, 1))
    flag, zd = po.SCORE_ONLY, 50
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_UNIFORM": 1, "KSW2AMD_STREAM": 1, "KSW2AMD_STREAM_PIECE_KB": 64, "KSW2AMD_SIMDS": 0,
                                                       "KSW2AMD_SOLO": 0})
    s0 = lib.stream_stats()
    n, res = pu.check_batch(lib, False, QS, TS, MAT, GQ, GE, 0, 0, w=w, zdrop=zd, flag=flag)
    assert n == len(QS) and lib.stream_stats()["streamed_plans"] - s0["streamed_plans"] == 1, "the uniform streamed plan did not run"
    assert 0 < sum(r["zdropped"] for r in res) < len(QS)
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {"KSW2AMD_SIMDS": 0, "KSW2AMD_SOLO": 0})
    fres = lib.make_flat_batch(QS, TS, MAT, GQ, GE, 0, 0, w=w, zdrop=zd, end_bonus=0, flag=flag).run_oneshot(False)
    exp = pu.oracle_batch(False, QS, TS, MAT, GQ, GE, 0, 0, w, zd, 0, flag)
    bad = [(i, pu.diff(exp[i], fres[i])) for i in range(len(QS)) if pu.diff(exp[i], fres[i])]
    assert not bad, ("flat", bad[:3])
