"""CPU: local alignment under the two-piece gap cost (ksw2amd_lld_batch / ksw2amd_lld_align_batch and their flat forms; include/ksw2_amd.h,
DESIGN.md section 3.18).  The contract's formula (tests/lld_oracle.c) is pinned to a brute-force statement of the definition and to the
compiled reference's scalar ksw_extd; the product's host code and lane code (K2aLaneLL<.., DUAL = true>, forward and REV, both number
formats and both score lookups) run on a test-local lock-step simulator build against that formula; a C caller compiled against
include/ksw2_amd.h prints the formula's answers; the golden file of the GPU tier is checked against the formula here too."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import lla_util as la
from tests import llf_util as lf
from tests import lld_util as d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ksw2amd_lld_batch", "ksw2amd_lld_align_batch", "ksw2amd_lld_batch_flat", "ksw2amd_lld_align_batch_flat")
EXTZ_ONLY = 0x40
_i8p = ctypes.POINTER(ctypes.c_int8)


@pytest.fixture(scope="module")
def simso(tmp_path_factory):
    return d.sim_library(str(tmp_path_factory.mktemp("lldsim") / "libksw2_amd.so"))


@pytest.fixture(scope="module")
def sim(simso):
    return ksw2_amd.Library(simso)


@pytest.fixture(autouse=True)
def _env():
    keys = ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS", "KSW2AMD_TRACE")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 3)
    return mat.reshape(-1)


def _cells(alns):
    return np.array([[r["score"], r["qe"], r["te"]] for r in alns], dtype=np.int32).reshape(-1, 3)


def _four_entries(lib, q, t, mat, costs, m, flag=0, dev=False):
    """(lld_batch, lld_align_batch, lld_batch_flat, lld_align_batch_flat) on the same pairs; the flat ones from a host arena (dev: the
    simulator's "device" arena, which is host memory used in place)"""
    a = lf.arena(q, t, lead=3, gap=2)
    db = a[0].ctypes.data if dev else None
    return (lib.lld_batch(q, t, mat, *costs, m=m), lib.lld_align_batch(q, t, mat, *costs, flag=flag, m=m),
            lib.lld_batch_flat(*a, mat, *costs, m=m, device_base=db), lib.lld_align_batch_flat(*a, mat, *costs, flag=flag, m=m, device_base=db))


def _check_four(lib, q, t, mat, costs, m, exp=None, flag=0, dev=False, msg=""):
    exp = d.expected(q, t, mat, costs, m, flag) if exp is None else exp
    fwd = np.array([[e["score"], e["qe"], e["te"]] for e in exp], dtype=np.int32).reshape(-1, 3)
    b, al, fb, fal = _four_entries(lib, q, t, mat, costs, m, flag, dev)
    np.testing.assert_array_equal(b, fwd, str(msg))
    np.testing.assert_array_equal(fb, fwd, str(msg))
    d.assert_same(al, exp, (msg, "align"))
    d.assert_same(fal, exp, (msg, "align flat"))
    return al


# ---------------------------------------------------------------- the oracle itself

def _tie_heavy(rng, k):
    """tiny pairs (<= 12 x 12): homopolymers, short repeats, random two- and three-letter strings"""
    kind = k % 4
    if kind == 0:
        return np.zeros(int(rng.integers(1, 13)), np.uint8), np.zeros(int(rng.integers(1, 13)), np.uint8)
    if kind == 1:
        unit = rng.integers(0, 2, int(rng.integers(1, 4)), dtype=np.uint8)
        return np.tile(unit, 4)[:int(rng.integers(1, 13))], np.tile(unit, 4)[:12]
    a = 2 if kind == 2 else 3
    return rng.integers(0, a, int(rng.integers(1, 13)), dtype=np.uint8), rng.integers(0, a, int(rng.integers(1, 13)), dtype=np.uint8)


COST_SETS = ((4, 2, 24, 1), (1, 1, 3, 0), (0, 1, 2, 0), (0, 0, 0, 0), (3, 2, 1, 1), (2, 1, 2, 1), (1, 0, 0, 1), (5, 1, 0, 3))


def test_oracle_is_the_definition_brute_force(sim):
    """tests/lld_oracle.c against every cell's H in plain Python with unclamped gap states and the tie rule on the set of maxima; the
    library (simulator build, clamped states, packed and int32) returns the same."""
    rng = np.random.default_rng(5)
    mat = np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)
    for ci, costs in enumerate(COST_SETS):
        qs, ts = zip(*[_tie_heavy(rng, k) for k in range(60)])
        exp = np.array([d.brute(q, t, mat, costs, 3) for q, t in zip(qs, ts)], dtype=np.int32)
        np.testing.assert_array_equal(d.oracle_batch(qs, ts, mat, costs, 3), exp, str(costs))
        os.environ["KSW2AMD_LL_FORM"] = str(ci % 3)
        np.testing.assert_array_equal(sim.lld_batch(list(qs), list(ts), mat, *costs, m=3), exp, str(costs))


def _pin_sets(rng):
    m5 = u.simple_mat(5, 2, 4, -1)
    m20 = u.random_mat(rng, 20)
    out = []
    q, t = u.ragged(rng, 500, 5, 1, 140, related=0.4)
    out.append((q, t, m5, 5, (4, 2, 24, 1)))
    q, t = u.ragged(rng, 400, 20, 1, 100, related=0.4)
    out.append((q, t, m20, 20, (6, 2, 10, 1)))
    q = [rng.integers(0, 4, int(rng.integers(40, 200)), dtype=np.uint8) for _ in range(400)]
    out.append((q, [u.mutate(rng, x, 4, 0.03, 0.04) for x in q], m5, 5, (4, 2, 8, 1)))
    q, t = u.ragged(rng, 400, 5, 1, 100, related=0.5)
    out.append((q, t, m5, 5, (0, 2, 3, 1)))                       # gapo = 0
    q, t = u.ragged(rng, 400, 5, 1, 100, related=0.5)
    out.append((q, t, m5, 5, (6, 3, 2, 1)))                       # the second piece is cheaper everywhere
    return out


def test_contract_pinned_to_reference():
    """For the oracle's best cell the reference's scalar ksw_extd (extension only, unbanded, no Z-drop) on the reversed prefixes reaches
    exactly the local score as ez.max, and its global score on [qb..qe] x [tb..te] equals the local score; the CIGAR covers the
    interval, re-scores to it under the two-piece cost and begins and ends with M when a gap costs."""
    if not la.have_ref():
        pytest.skip("oracle/_ref/libksw2ref.so not built (build() makes it where the reference's sources exist)")
    from oracle import pyoracle as po
    rng = np.random.default_rng(11)
    total = 0
    for q, t, mat, m, costs in _pin_sets(rng):
        exp = d.expected(q, t, mat, costs, m, which="ref")
        exp_own = d.expected(q, t, mat, costs, m, which="oracle")
        for i, e in enumerate(exp):
            total += 1
            if e["score"] == 0:
                assert (e["qb"], e["qe"], e["tb"], e["te"], e["n_cigar"]) == (-1, -1, -1, -1, 0)
                continue
            assert e["rscore"] == e["score"] and e["gscore"] == e["score"], (costs, i, e)
            assert e["cigar"] == exp_own[i]["cigar"], (costs, i)                       # the project's restatement of ksw_extd agrees
            r = po.align("ref", "extd", q[i][:e["qe"] + 1][::-1], t[i][:e["te"] + 1][::-1], mat, *costs, w=-1, zdrop=-1, flag=EXTZ_ONLY, m=m)
            assert r["max"] == e["score"], (costs, i, r["max"], e)
        d.check_cigars(exp, q, t, mat, m, costs)
    assert total >= 2000


# ---------------------------------------------------------------- the simulator twin through the four public entries

def _new_ground(rng, m):
    """what the second piece adds: the crossover gaps (lane hand-over, generation boundary, column 0), start-cell ground of
    tests/lla_util.py (halves ending in different cells, a zero half, rows above one generation), tie-heavy repeats"""
    q, t, lns = d.crossover_pairs(rng, m, big=True)
    q2, t2 = la.new_ground(rng, m, small=True)
    return q + q2, t + t2, lns


@pytest.mark.parametrize("m", [5, 20])
def test_sim_every_forced_form(sim, monkeypatch, capfd, m):
    rng = np.random.default_rng(300 + m)
    mat = d.cross_mat(m)
    q, t, lns = _new_ground(rng, m)
    exp = d.expected(q, t, mat, d.CROSS, m)
    single = u.oracle_batch(q, t, mat, 4, 2, m)
    for i, ln in enumerate(lns):                                   # the cases test what they are built for
        assert (exp[i]["score"] != single[i][0]) == (ln > 20), (i, ln)
    assert any(e["te"] - e["tb"] > 1024 or e["qe"] - e["qb"] > 1024 for e in exp) or any(e["tb"] < 1024 <= e["te"] or e["qb"] < 1024 <= e["qe"] for e in exp)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form in ("0", "1", "2"):
        for lds in ("0", "1"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
            capfd.readouterr()
            _check_four(sim, q, t, mat, d.CROSS, m, exp, msg=(form, lds))
            err = capfd.readouterr().err
            line = re.search(r"lld-rev: pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
            fwd = re.search(r"lld: pairs=(\d+) pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
            assert line and fwd and "ll:" not in err and "ll-rev:" not in err, err
            assert (int(line.group(1)) == 0) if form == "0" else (int(line.group(1)) >= 12), (form, err)
            assert line.group(3) == ("lds" if lds == "1" or m > 5 else "registers"), err
            assert ("pk_profile=lds" in err) == (lds == "0" and m <= 5), err        # packed two-piece tasks never take the register profile
    _check_four(sim, q[:30], t[:30], mat, d.CROSS, m, exp[:30], dev=True, msg="device arena")


@pytest.mark.parametrize("costs", [(6, 3, 2, 1), (0, 0, 0, 0), (127, 127, 127, 127), (0, 127, 127, 0), (3, 1, 40, 0)])
def test_sim_cost_shapes(sim, costs):
    """second piece cheaper everywhere, all four costs 0, all 127, and mixed extremes: every stage exact, m 5 and an arbitrary m = 11"""
    rng = np.random.default_rng(sum(costs) + 1)
    for m, mat in ((5, u.simple_mat(5, 2, 4, -1)), (11, u.random_mat(rng, 11, -9, 9)), (127, u.random_mat(rng, 127, -128, 128))):
        q, t = u.ragged(rng, 30, m, 1, 120, related=0.7)
        al = _check_four(sim, q, t, mat, costs, m, msg=(costs, m))
        d.check_cigars(al, q, t, mat, m, costs)


def test_sim_flags_and_cigar_rescoring(sim):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    costs = (4, 2, 8, 1)
    q, t = u.ragged(rng, 50, 5, 1, 300, related=0.8)
    q += [np.tile(np.array([0, 1], np.uint8), 30)] * 4                       # gaps whose placement RIGHT changes
    t += [np.concatenate([np.tile(np.array([0, 1], np.uint8), 20), [0, 0], np.tile(np.array([0, 1], np.uint8), 20)]).astype(np.uint8)] * 4
    base = d.expected(q, t, mat, costs, 5)
    differs = 0
    for flag in (0, d.RIGHT, d.REV_CIGAR, d.RIGHT | d.REV_CIGAR, d.SCORE_ONLY, d.SCORE_ONLY | d.RIGHT):
        got = _check_four(sim, q, t, mat, costs, 5, flag=flag, msg=flag)
        d.check_cigars(got, q, t, mat, 5, costs, flag)
        for g, b in zip(got, base):
            assert all(g[f] == b[f] for f in ("score", "qb", "qe", "tb", "te"))
            if flag & d.SCORE_ONLY:
                assert g["n_cigar"] == 0 and g["cigar"] == []
            differs += g["cigar"] != b["cigar"] and not flag & d.SCORE_ONLY
    assert differs > 0


@pytest.mark.parametrize("m", [5, 20])
def test_degenerate_costs_equal_the_single_piece_entries(sim, monkeypatch, m):
    """(gapo2, gape2) = (gapo, gape), and gapo2 >= gapo with gape2 >= gape: bit for bit the ll_* entries' res and aln, CIGARs included"""
    rng = np.random.default_rng(17 + m)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else _m20(rng)
    q, t = la.new_ground(rng, m, small=True)
    a = lf.arena(q, t, lead=1, gap=1)
    for form in ("1", "0"):
        monkeypatch.setenv("KSW2AMD_LL_FORM", form)
        res1, aln1 = sim.ll_batch(q, t, mat, 4, 2, m=m), sim.ll_align_batch(q, t, mat, 4, 2, m=m)
        for go2, ge2 in ((4, 2), (4, 3), (9, 2), (127, 127)):
            costs = (4, 2, go2, ge2)
            b, al, fb, fal = _four_entries(sim, q, t, mat, costs, m)
            np.testing.assert_array_equal(b, res1)
            np.testing.assert_array_equal(fb, res1)
            assert al == aln1 and fal == aln1, costs
    assert sim.ll_align_batch_flat(*a, mat, 4, 2, m=m) == aln1            # (the single-piece flat entry through the shared code)


def _raw_align(sim, q, t, mat, costs, flag, aln, m=5, km=None):
    pairs, keep = sim.local_pairs(q, t)
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    return sim.lib.ksw2amd_lld_align_batch(km, m, mat.ctypes.data_as(_i8p), *costs, flag, len(q), pairs, aln)


def test_bad_arguments_launch_nothing(sim, monkeypatch, capfd):
    mat = u.simple_mat(5, 2, 4, -1)
    x = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    bad = np.array([0, 5], np.uint8)
    a_ok, a_bad = lf.arena([x], [x]), lf.arena([x], [bad])
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    cases = [dict(costs=c) for k in range(4) for c in (tuple(-1 if j == k else 2 for j in range(4)), tuple(128 if j == k else 2 for j in range(4)))]
    cases += [dict(flag=0x40), dict(flag=0x800), dict(flag=0x04), dict(t=bad), dict(m=0), dict(m=128)]
    for kw in cases:
        costs, flag, tt, m = kw.get("costs", (4, 2, 24, 1)), kw.get("flag", 0), kw.get("t", x), kw.get("m", 5)
        arena = a_bad if "t" in kw else a_ok
        d.launches(sim, reset=True)
        capfd.readouterr()
        calls = [lambda: sim.lld_align_batch([x], [tt], mat, *costs, flag=flag, m=m), lambda: sim.lld_align_batch_flat(*arena, mat, *costs, flag=flag, m=m)]
        if "flag" not in kw:
            calls += [lambda: sim.lld_batch([x], [tt], mat, *costs, m=m), lambda: sim.lld_batch_flat(*arena, mat, *costs, m=m)]
        for call in calls:
            with pytest.raises(ksw2_amd.Ksw2Error, match="error -2"):
                call()
        err = capfd.readouterr().err
        n_lld, n_ll, n_chk = d.launches(sim)
        assert n_lld == 0 and n_ll == 0, (kw, err)                # no alignment kernel; a flat entry's code check may have run
        assert n_chk == (2 if "t" in kw else 0), kw
        if "t" not in kw:
            assert "lld:" not in err and "lld-rev:" not in err, err          # nothing was staged either
    # the flat entries name the lowest offending pair and leave the reset values
    qs, ts = [x, x, x, x], [x, bad, x, bad]
    out = np.full((4, 3), 7, np.int32)
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 1: residue code >= m"):
        sim.lld_batch_flat(*lf.arena(qs, ts), mat, 4, 2, 24, 1, out=out)
    assert (out == np.array([0, -1, -1])).all()
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 1: residue code >= m"):
        sim.lld_batch(qs, ts, mat, 4, 2, 24, 1)
    # the corner the CIGAR stage cannot take: m = 1 in the align entries (the score entries accept it)
    one, z = np.array([3], np.int8), np.zeros(9, np.uint8)
    d.launches(sim, reset=True)
    for call in (lambda: sim.lld_align_batch([z], [z], one, 1, 1, 2, 0, m=1), lambda: sim.lld_align_batch([z], [z], one, 1, 1, 2, 0, flag=d.SCORE_ONLY, m=1),
                 lambda: sim.lld_align_batch_flat(*lf.arena([z], [z]), one, 1, 1, 2, 0, m=1)):
        with pytest.raises(ksw2_amd.Ksw2Error, match="error -2"):
            call()
    assert d.launches(sim) == (0, 0, 0)
    assert sim.lld_batch([z], [z], one, 1, 1, 2, 0, m=1).tolist() == [[27, 8, 8]]
    # a NULL sequence with a positive length
    aln = (ksw2_amd.LocalAln * 1)()
    pairs = (ksw2_amd.LocalPair * 1)()
    pairs[0].query, pairs[0].target, pairs[0].qlen, pairs[0].tlen = None, x.ctypes.data, 3, 6
    assert sim.lib.ksw2amd_lld_align_batch(None, 5, mat.ctypes.data_as(_i8p), 4, 2, 24, 1, 0, 1, pairs, aln) == -2
    # n = 0, empty sequences, a matrix without a positive entry: the reset results, nothing launched
    d.launches(sim, reset=True)
    assert sim.lld_align_batch([], [], mat, 4, 2, 24, 1) == [] and len(sim.lld_batch([], [], mat, 4, 2, 24, 1)) == 0
    e = np.zeros(0, np.uint8)
    r = sim.lld_align_batch([x, e, x], [x, x, e], -np.abs(mat), 4, 2, 24, 1)
    assert all((g["score"], g["qb"], g["qe"], g["tb"], g["te"], g["n_cigar"]) == (0, -1, -1, -1, -1, 0) for g in r)
    assert (sim.lld_batch([x, e, x], [x, x, e], -np.abs(mat), 4, 2, 24, 1) == np.array([0, -1, -1])).all()
    assert d.launches(sim)[:2] == (0, 0)
    r = sim.lld_align_batch([e, x], [x, x], mat, 4, 2, 24, 1)
    assert r[0]["score"] == 0 and r[0]["qb"] == -1 and r[1]["score"] == 12 and r[1]["cigar"] == [6 << 4]


def test_cigar_buffer_reuse_without_a_pool(sim):
    rng = np.random.default_rng(41)
    mat = u.simple_mat(5, 2, 4, -1)
    costs = (4, 2, 8, 1)
    q, t = u.ragged(rng, 12, 5, 40, 200, related=1.0)
    exp = d.expected(q, t, mat, costs, 5)
    aln = (ksw2_amd.LocalAln * len(q))()
    assert _raw_align(sim, q, t, mat, costs, 0, aln) == 0
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    assert all(p and mc >= x.n_cigar > 0 for (p, mc), x in zip(first, aln))
    assert _raw_align(sim, q[::-1], t[::-1], mat, costs, 0, aln) == 0         # other alignments into the same buffers
    for k, x in enumerate(aln):
        e = exp[len(q) - 1 - k]
        assert [int(x.cigar[j]) for j in range(x.n_cigar)] == e["cigar"] and x.score == e["score"]
        if x.n_cigar <= first[k][1]:
            assert (ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) == first[k]
    assert _raw_align(sim, q[::-1], t[::-1], mat, costs, d.SCORE_ONLY, aln) == 0
    assert all(x.n_cigar == 0 and x.m_cigar > 0 for x in aln)
    for x in aln:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


def test_flat_chunks_and_reset(sim, monkeypatch):
    """chunking, and the reset semantics of the single-piece flat entries: a bad code in a later chunk leaves earlier chunks' res[] and
    resets every aln[]"""
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 40, 5, 30, 200, related=0.8)
    exp = d.oracle_batch(q, t, mat, d.CROSS, 5)
    monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "4000")
    a = lf.arena(q, t, rng, lead=2, gap=5)
    np.testing.assert_array_equal(sim.lld_batch_flat(*a, mat, *d.CROSS), exp)
    t[30] = t[30].copy()
    t[30][3] = 9
    a = lf.arena(q, t, rng, lead=2, gap=5)
    out = np.full((40, 3), 7, np.int32)
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
        sim.lld_batch_flat(*a, mat, *d.CROSS, out=out)
    assert (out[:8] == exp[:8]).all() and (out[30:] == np.array([0, -1, -1])).all()
    aln = (ksw2_amd.LocalAln * 40)()
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30"):
        sim.lld_align_batch_flat(*a, mat, *d.CROSS, aln=aln)
    assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)


# ---------------------------------------------------------------- header, ABI, golden file

def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ksw2_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ksw2_amd.EXPORTS
    if not os.path.exists(ksw2_amd.DEFAULT_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ksw2_amd", "csrc")], check=True, capture_output=True)
    lib = ctypes.CDLL(ksw2_amd.DEFAULT_SO)
    for name in NAMES:
        assert hasattr(lib, name), name
    for name in ("lld_batch", "lld_align_batch", "lld_batch_flat", "lld_align_batch_flat"):
        assert callable(getattr(ksw2_amd.Library, name))
    # ksw2_host_ll.o names no new launch symbol: the older simulator builds keep linking
    for obj in ("ll", "lla", "llf", "lls"):
        o = os.path.join(ROOT, "ksw2_amd", "csrc", "ksw2_host_%s.o" % obj)
        if os.path.exists(o):
            assert "k2a_shim_launch_lld" not in subprocess.run(["nm", "-u", o], capture_output=True, text=True, check=True).stdout, obj


def _write_input(path, q, t, mat, m, costs, flag):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n%s\n%d\n" % ((m,) + tuple(costs) + (flag, " ".join(str(int(x)) for x in mat), len(q))))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))


@pytest.mark.parametrize("pool", [False, True])
def test_c_caller_with_and_without_pool(simso, tmp_path, pool):
    exe = str(tmp_path / "lld_caller")
    libdir = os.path.dirname(simso)
    subprocess.run(["gcc", "-O1", "-Wall", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "lld_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    costs = (4, 2, 8, 1)
    q, t = u.ragged(rng, 14, 5, 1, 500, related=0.8)
    q.append(np.zeros(3, np.uint8)); t.append(np.ones(4, np.uint8))          # a score of 0 among them
    for flag in (0, d.RIGHT | d.REV_CIGAR):
        inp = str(tmp_path / "pairs.txt")
        _write_input(inp, q, t, mat, 5, costs, flag)
        out = subprocess.run([exe, inp] + (["pool"] if pool else []), check=True, capture_output=True, text=True).stdout
        out = out.replace("\nflat\n", "\nsingle\n")
        batch, flat, reallocs = la.parse_caller(out)
        exp = d.expected(q, t, mat, costs, 5, flag)
        d.assert_same(batch, exp, "batch")
        d.assert_same(flat, exp, "flat")
        assert (reallocs is not None and reallocs >= 2 * sum(e["score"] > 0 for e in exp)) if pool else reallocs is None      # the CIGARs really came from the pool


def test_golden_file_is_the_formula(sim):
    """tests/golden/lld_cases.npz (the GPU tier's expected values, from tests/lld_oracle.c and the compiled reference's ksw_extd) against
    this checkout's formula with the project's own ksw_extd, and through the simulator build"""
    cases = d.load_golden()
    gen = d.golden_inputs()
    assert [c[0] for c in cases] == [g[0] for g in gen]
    for (name, m, mat, costs, q, t, exp), g in zip(cases, gen):
        assert m == g[1] and costs == tuple(g[3]) and (np.asarray(mat) == g[2]).all() and len(q) == len(g[4])
        assert all((a == b).all() for a, b in zip(q + t, list(g[4]) + list(g[5])))
        d.assert_same(d.expected(q, t, mat, costs, m), exp, name)
        d.check_cigars(exp, q, t, mat, m, costs)
        d.assert_same(sim.lld_align_batch(q, t, mat, *costs, m=m), exp, name)
