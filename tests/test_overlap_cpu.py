"""CPU: overlap alignment (ksw2amd_ov_batch / ksw2amd_ovd_batch, their flat forms and the single-pair entries; include/ksw2_amd.h, DESIGN.md
section 3.23).  The contract's formula (tests/ov_oracle.c) is pinned to the compiled reference's scalar ksw_extz / ksw_extd through
tests/golden/ov_cases.npz and to a brute-force statement of the candidates and the tie rule; the product's host code and lane code
(K2aLaneLL<.., FIT, OV>, both number formats, both score lookups, both gap costs) run on a test-local lock-step simulator build against that
formula; a C caller compiled against include/ksw2_amd.h prints the formula's answers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import llf_util as lf
from tests import ov_util as o
from tests import sg_util as s
from tests import sgd_util as d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (0, 0), (4, 2, 24, 1), (24, 1, 4, 2))
FORMS = [(f, l) for f in ("0", "1", "2") for l in ("0", "1")]


@pytest.fixture(scope="module")
def simso(tmp_path_factory):
    return o.sim_library(str(tmp_path_factory.mktemp("ovsim") / "libksw2_amd.so"))


@pytest.fixture(scope="module")
def sim(simso):
    return ksw2_amd.Library(simso)


@pytest.fixture(autouse=True)
def _env():
    keys = ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS", "KSW2AMD_TRACE", "KSW2AMD_ABORT_ON_ERROR")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _form(form, lds):
    os.environ["KSW2AMD_LL_FORM"] = form
    os.environ["KSW2AMD_LL_LDS"] = lds


def _both(lib, q, t, mat, costs, ends, m, exp=None, msg="", flat=True):
    """the pointer entry and the flat entry (host arena with bytes that no matrix admits between the sequences) against the formula"""
    exp = o.oracle_batch(q, t, mat, costs, ends, m) if exp is None else exp
    np.testing.assert_array_equal(o.call(lib, q, t, mat, costs, ends, m), exp, str((msg, costs, ends)))
    if flat:
        np.testing.assert_array_equal(o.call_flat(lib, lf.arena(q, t, lead=3, gap=2), mat, costs, ends, m), exp, str((msg, costs, ends, "flat")))
    return exp


# ---------------------------------------------------------------- 1. the oracle itself

def test_oracle_equals_the_golden_file_of_the_compiled_reference():
    total = 0
    for name, m, mat, c2, c4, q, t, exp, expd in o.load_golden():
        for e in o.ENDS:
            np.testing.assert_array_equal(o.oracle_batch(q, t, mat, c2, e, m), exp[e], str((name, e)))
            np.testing.assert_array_equal(o.oracle_batch(q, t, mat, c4, e, m), expd[e], str((name, e, "two-piece")))
        total += len(q)
    assert total == 324
    g = o.load_golden()
    nq = [np.array([len(x) - 1 for x in c[5]]) for c in g]
    assert sum(int((c[7][3][:, 1] < n).sum()) for c, n in zip(g, nq)) > 50          # best cells in the last row off the corner
    assert sum(int((c[7][3][:, 0] < 0).sum()) for c in g) > 20                      # negative optima with both ends free
    assert any((c[7][1] != c[7][3]).any() for c in g) and any((c[7][2] != c[7][3]).any() for c in g)


def test_ends_0_of_the_oracle_is_the_semiglobal_golden_file():
    for g, gd in zip(s.load_golden(), d.load_golden()):
        name, m, mat, gapo, gape, q, t, exp = g
        np.testing.assert_array_equal(o.oracle_batch(q, t, mat, (gapo, gape), 0, m), exp, name)
        np.testing.assert_array_equal(o.oracle_batch(q, t, mat, gd[3], 0, m), gd[6][:, [0, 2, 4]], name)


def test_oracle_is_the_formula_brute_force(sim):
    """tests/ov_oracle.c against full matrices in plain Python with the candidate cells listed one by one; costs with 0, matrices without a
    positive entry, every ends; the library (simulator build) returns the same."""
    rng = np.random.default_rng(5)
    seen_row = seen_neg = 0
    for ci, costs in enumerate(((4, 2), (0, 1), (3, 0), (0, 0), (1, 1), (4, 2, 24, 1), (24, 1, 4, 2), (0, 1, 5, 0), (5, 0, 2, 1))):
        for m, mat in ((3, np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)), (4, u.random_mat(rng, 4, -6, 1)), (2, u.random_mat(rng, 2))):
            qs, ts = [], []
            for k in range(30):
                a = 1 if k % 5 == 0 else m                                   # homopolymers: everything ties
                q = rng.integers(0, a, int(rng.integers(1, 13)), dtype=np.uint8)
                t = rng.integers(0, a, int(rng.integers(1, 25)), dtype=np.uint8)
                if k % 3 == 0:
                    p = int(rng.integers(1, len(q) + 1))
                    t = np.concatenate([q[len(q) - p:], t, q[:p]]).astype(np.uint8)      # a suffix at the head, a prefix at the tail
                qs.append(q); ts.append(t)
            for ends in range(4):
                exp = np.array([o.brute(q, t, mat, costs, ends, m) for q, t in zip(qs, ts)], dtype=np.int32)
                np.testing.assert_array_equal(o.oracle_batch(qs, ts, mat, costs, ends, m), exp, str((costs, m, ends)))
                _form(str(ci % 3), str(ci % 2))
                np.testing.assert_array_equal(o.call(sim, qs, ts, mat, costs, ends, m), exp, str((costs, m, ends)))
                if ends == 3:
                    seen_row += int((exp[:, 1] < np.array([len(q) - 1 for q in qs])).sum())
                    seen_neg += int((exp[:, 0] < 0).sum())
    assert seen_row > 50 and seen_neg > 20


# ---------------------------------------------------------------- 2. the library on the simulator

@pytest.mark.parametrize("form,lds", FORMS)
def test_ragged_batch_every_form(sim, form, lds):
    rng = np.random.default_rng(11 + int(form))
    _form(form, lds)
    for m, mat in ((5, u.simple_mat(5, 2, 4, -1)), (20, u.random_mat(rng, 20, -5, 4)), (4, u.random_mat(rng, 4, -6, 1))):
        q, t = o.ragged_batch(rng, n=30, m=m, qmax=90, tmax=260, long_targets=0)
        q += [q[0], q[0], q[1]]
        t += [t[0], t[0][::-1].copy(), t[1]]                               # same-shape partners for form 1
        t[3] = np.concatenate([rng.integers(0, m, 1100, dtype=np.uint8), q[3][:len(q[3]) // 2 + 1]])      # two generations, a prefix at the tail
        t[4] = np.concatenate([q[4][len(q[4]) // 2:], rng.integers(0, m, 1030, dtype=np.uint8)])
        for costs in COSTS:
            for ends in o.ENDS:
                _both(sim, q, t, mat, costs, ends, m, msg=(form, lds, m), flat=ends == 3)


@pytest.mark.parametrize("form", ["0", "2"])
def test_golden_file_on_the_simulator(sim, form):
    os.environ["KSW2AMD_LL_FORM"] = form
    for name, m, mat, c2, c4, q, t, exp, expd in o.load_golden():
        for e in o.ENDS:
            _both(sim, q, t, mat, c2, e, m, exp=exp[e], msg=name, flat=False)
            _both(sim, q, t, mat, c4, e, m, exp=expd[e], msg=name, flat=False)


_grid = {}


def _qend_grid():
    if not _grid:
        qs, ts, what = o.qend_grid(np.random.default_rng(78))
        _grid.update(q=qs, t=ts, what=what)
        for costs in ((4, 2), d.CROSS):
            for e in (2, 3):
                _grid[(costs, e)] = o.oracle_batch(qs, ts, s.unit_mat(5), costs, e, 5)
    return _grid


@pytest.mark.parametrize("form,lds", FORMS)
def test_edge_grid_query_end(sim, form, lds):
    """tlen 1 .. 2 049 x qlen 1 .. 130, the query's first p residues planted as the target's last p: the last row in strip registers 0, 7, 14,
    15, in lanes 0, 1, 63 and in generations 0, 1, 2; p - 1 around the 4-step prefetch and the 63-step skew"""
    _form(form, lds)
    g = _qend_grid()
    mat = s.unit_mat(5)
    for costs in ((4, 2), d.CROSS):
        for e in (2, 3):
            exp = _both(sim, g["q"], g["t"], mat, costs, e, 5, exp=g[(costs, e)], msg=(form, lds), flat=False)
    exp = g[((4, 2), 3)]
    seen = set()
    for (tl, ql, p), r in zip(g["what"], exp):
        if p <= tl:                                                         # the whole prefix fits: p matches ending in the last row
            assert tuple(r) == (2 * p, p - 1, tl - 1) or r[0] > 2 * p, (tl, ql, p, r)
            if tuple(r) == (2 * p, p - 1, tl - 1):
                seen.add(((tl - 1) % 16, ((tl - 1) % 1024) // 16, (tl - 1) // 1024))
    assert {c for c, _, _ in seen} >= {0, 7, 14, 15} and {l for _, l, _ in seen} >= {0, 1, 63} and {x for _, _, x in seen} == {0, 1, 2}


@pytest.mark.parametrize("form,lds", FORMS)
def test_edge_grid_query_start(sim, form, lds):
    _form(form, lds)
    qs, ts, what = o.qbeg_grid(np.random.default_rng(79))
    mat = s.unit_mat(5)
    for costs in ((4, 2), d.CROSS):
        e1 = _both(sim, qs, ts, mat, costs, 1, 5, msg=(form, lds), flat=False)
        e0 = _both(sim, qs, ts, mat, costs, 0, 5, msg=(form, lds), flat=False)
        _both(sim, qs, ts, mat, costs, 3, 5, msg=(form, lds), flat=False)
        for (tl, ql, x), r1, r0 in zip(what, e1, e0):
            if x > 0:
                assert tuple(r1) == (2 * x, ql - 1, x - 1), (tl, ql, x, r1)     # the hanging prefix costs nothing
                assert x == ql or r0[0] < r1[0]
            else:
                assert tuple(r1) == tuple(r0) == (2 * ql, ql - 1, -x)          # a whole copy inside the target: the free start changes nothing


@pytest.mark.parametrize("form,lds", FORMS)
def test_both_ends_and_ties(sim, form, lds):
    _form(form, lds)
    mat = s.unit_mat(5)
    qs, ts, kinds = o.both_pairs(np.random.default_rng(80))
    res = {e: _both(sim, qs, ts, mat, (4, 2), e, 5, msg=kinds) for e in range(4)}
    for e in range(4):
        _both(sim, qs, ts, mat, d.CROSS, e, 5, msg=kinds)
    assert tuple(res[1][0]) == (50, 59, 24) and res[0][0][0] < 50           # query suffix = target prefix needs the start free
    assert tuple(res[2][1]) == (50, 24, 59) and res[0][1][0] < 50           # query prefix = target suffix needs the end free
    assert all(tuple(res[e][2]) == (60, 29, 739) for e in range(4))         # a contained query: every mode agrees
    assert tuple(res[3][3]) == (90, 69, 44) and all(res[e][3][0] < 90 for e in range(3))      # a contained target needs both
    qs, ts, es, exp = o.tie_cases()
    for q, t, e, x in zip(qs, ts, es, exp):
        assert o.brute(q, t, mat, (4, 2), e, 5) == x
        _both(sim, [q], [t], mat, (4, 2), e, 5, exp=np.array([x], np.int32))
        _both(sim, [q, q], [t, t], mat, (4, 2, 4, 2), e, 5, exp=np.array([x, x], np.int32))
    qs, ts, tes = s.tie_pairs()                                             # two equal last-column rows across a lane and a generation boundary
    for e in o.ENDS:
        got = _both(sim, qs, ts, mat, (4, 2), e, 5)
        assert [int(v) for v in got[:, 2]] == tes and (got[:, 0] == 12).all() and (got[:, 1] == 5).all()


@pytest.mark.parametrize("form,lds", FORMS)
def test_identities(sim, form, lds):
    """ends == 0 is the semi-global entry bit for bit; equal or dominated second pieces give the single-piece result"""
    _form(form, lds)
    rng = np.random.default_rng(12)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=40, m=5, qmax=80, tmax=300, long_targets=0)
    t[2] = rng.integers(0, 5, 1200, dtype=np.uint8)
    np.testing.assert_array_equal(sim.ov_batch(q, t, mat, 4, 2, 0, m=5), sim.sg_batch(q, t, mat, 4, 2, m=5))
    np.testing.assert_array_equal(sim.ovd_batch(q, t, mat, 4, 2, 24, 1, 0, m=5), sim.sgd_batch(q, t, mat, 4, 2, 24, 1, m=5))
    ar = lf.arena(q, t, lead=1, gap=1)
    np.testing.assert_array_equal(sim.ov_batch_flat(*ar, mat, 4, 2, 0, m=5), sim.sg_batch_flat(*ar, mat, 4, 2, m=5))
    for e in range(4):
        one = sim.ov_batch(q, t, mat, 4, 2, e, m=5)
        for c2 in ((4, 2), (5, 2), (4, 3), (127, 127)):
            np.testing.assert_array_equal(sim.ovd_batch(q, t, mat, 4, 2, c2[0], c2[1], e, m=5), one, str((e, c2)))


def _admission_mat():
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    return mat.reshape(-1)


def test_admission_bound(sim, capfd):
    """smax = 127, costs (5, 1): B + (qlen + 1) * smax = 128 qlen + 132 <= 65 535 up to qlen 510, with the ends free as without"""
    os.environ["KSW2AMD_LL_FORM"] = "2"
    os.environ["KSW2AMD_TRACE"] = "1"
    rng = np.random.default_rng(3)
    mat = _admission_mat()
    for ql, packed in ((510, True), (511, False)):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q[:ql - 7]])
        for name, costs in (("ov", (5, 1)), ("ovd", (5, 1, 9, 1))):
            capfd.readouterr()
            got = o.call(sim, [q], [t], mat, costs, 3, 4)
            err = capfd.readouterr().err
            assert tuple(got[0]) == (127 * (ql - 7), ql - 8, len(t) - 1)
            np.testing.assert_array_equal(got, o.oracle_batch([q], [t], mat, costs, 3, 4))
            assert o.pk_tasks(err, name) == [(1, 0) if packed else (0, 1)], err
            assert " ends=3" in err


def long_query_case():
    """qlen = 65 537 against tlen = 20 under a matrix without a positive entry and gape = 0: B = gapo, so the packed bound admits the pair,
    but the best cell is the last row's column 65 536, which no 16-bit index holds.  The target has no border, so the corner is the only
    candidate that scores 0"""
    t = np.array([0] + [1] * 19, np.uint8)
    q = np.concatenate([np.full(65537 - 20, 2, np.uint8), t])
    mat = u.simple_mat(4, 0, 3)
    return q, t, mat


def test_16_bit_column_condition(sim, capfd):
    os.environ["KSW2AMD_LL_FORM"] = "2"
    os.environ["KSW2AMD_TRACE"] = "1"
    q, t, mat = long_query_case()
    assert mat.max() == 0
    for name, costs in (("ov", (3, 0)), ("ovd", (3, 0, 9, 0))):
        exp = o.oracle_batch([q], [t], mat, costs, 3, 4)
        assert tuple(exp[0]) == (0, 65536, 19)
        capfd.readouterr()
        np.testing.assert_array_equal(o.call(sim, [q], [t], mat, costs, 3, 4), exp)
        assert o.pk_tasks(capfd.readouterr().err, name) == [(0, 1)]           # int32: the column does not fit
        np.testing.assert_array_equal(o.call(sim, [q], [t], mat, costs, 1, 4), o.oracle_batch([q], [t], mat, costs, 1, 4))
        assert o.pk_tasks(capfd.readouterr().err, name) == [(1, 0)]           # without the free end no column index is kept
    # one residue fewer: column 65 535 fits, the pair is packed and right
    exp = o.oracle_batch([q[1:]], [t], mat, (3, 0), 3, 4)
    assert tuple(exp[0]) == (0, 65535, 19)
    np.testing.assert_array_equal(o.call(sim, [q[1:]], [t], mat, (3, 0), 3, 4), exp)
    assert o.pk_tasks(capfd.readouterr().err, "ov") == [(1, 0)]


def test_scores_beyond_16_bits_and_negative_scores(sim):
    rng = np.random.default_rng(4)
    os.environ["KSW2AMD_LL_FORM"] = "2"
    q = rng.integers(0, 4, 1700, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q[:1650]])
    exp = _both(sim, [q], [t], u.simple_mat(4, 40, 30), (4, 2), 2, 4)
    assert tuple(exp[0]) == (40 * 1650, 1649, len(t) - 1) and exp[0, 0] > 65535
    # unrelated sequences under +1 / -100: the best candidate is a real cell, never the boundary, so the score stays negative with both ends free
    q, t = np.zeros(40, np.uint8), np.ones(300, np.uint8)
    for costs in ((20, 3), (2, 1), (0, 0), (20, 3, 30, 1)):
        for e in range(4):
            exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), costs, e, 4)
            assert exp[0, 0] < 0 or costs == (0, 0)
    mat = u.random_mat(rng, 5, -7, 1)
    assert mat.max() <= 0
    qs, ts = u.ragged(rng, 12, 5, 1, 60)
    o.launches(sim, reset=True)
    for e in o.ENDS:
        exp = _both(sim, qs, ts, mat, (3, 1), e, 5)
        assert (exp[:, 0] <= 0).all()
    assert o.launches(sim)[0] > 0


def test_packed_halves_on_different_edges(sim, capfd):
    """two pairs of one shape in one packed task: one ends in the last column in the middle of the target, the other in the last row"""
    os.environ["KSW2AMD_LL_FORM"] = "1"
    os.environ["KSW2AMD_TRACE"] = "1"
    rng = np.random.default_rng(6)
    qa, ta = s.planted(rng, 5, 1040, 64, 500)
    qb, tb = o.qend_pair(rng, 1040, 64, 40)
    capfd.readouterr()
    exp = _both(sim, [qa, qb, qb, qa], [ta, tb, tb, ta], s.unit_mat(5), (4, 2), 3, 5, flat=False)
    assert o.pk_tasks(capfd.readouterr().err) == [(2, 0)]
    assert tuple(exp[0]) == (128, 63, 500) and tuple(exp[1]) == (80, 39, 1039)


def test_corner_results_launch_nothing(sim):
    e = np.zeros(0, np.uint8)
    q = np.array([0, 1, 2, 3, 0], np.uint8)
    mat = u.simple_mat(5, 2, 4, -1)
    for costs in ((4, 2), (4, 2, 1, 3)):
        ins = -o.gap_cost(costs, 5)
        for ends in range(4):
            o.launches(sim, reset=True)
            exp = np.array([[0, -1, -1], [0 if ends & 1 else ins, 4, -1], [0, -1, -1]], np.int32)
            np.testing.assert_array_equal(o.call(sim, [e, q, e], [q, e, e], mat, costs, ends, 5), exp)
            np.testing.assert_array_equal(o.oracle_batch([e, q, e], [q, e, e], mat, costs, ends, 5), exp)
            np.testing.assert_array_equal(o.call_flat(sim, lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, costs, ends, 5), exp)
            assert o.launches(sim)[:3] == (0, 0, 0)                            # (the flat entry's check ran)
            assert o.call(sim, [], [], mat, costs, ends, 5).shape == (0, 3)
            # corners beside real pairs
            np.testing.assert_array_equal(o.call(sim, [q, e, q], [e, q, q], mat, costs, ends, 5), [[0 if ends & 1 else ins, 4, -1], [0, -1, -1], [10, 4, 4]])
    assert sim.ov(q, e, mat, 4, 2, 1) == (0, 4, -1) and sim.ov(q, e, mat, 4, 2, 2) == (-14, 4, -1) and sim.ov(e, q, mat, 4, 2, 3) == (0, -1, -1)
    assert sim.ovd(q, e, mat, 4, 2, 1, 3, 2) == (-14, 4, -1) and sim.ovd(q, q, mat, 4, 2, 1, 3, 3) == (10, 4, 4)


def test_single_pair_entries(sim):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=9, m=5, qmax=60, tmax=200, long_targets=0)
    for ends in range(4):
        exp = o.oracle_batch(q, t, mat, (4, 2), ends, 5)
        expd = o.oracle_batch(q, t, mat, d.CROSS, ends, 5)
        for k in range(len(q)):
            assert sim.ov(q[k], t[k], mat, 4, 2, ends) == tuple(exp[k])
            assert sim.ovd(q[k], t[k], mat, *d.CROSS, ends) == tuple(expd[k])


def test_bad_arguments(sim):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = sim.local_pairs(q, t)
    res = (ksw2_amd.LocalResult * 6)()
    L = sim.lib
    mp = mat.ctypes.data_as(_i8p)
    a = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = sim._local_flat(*a, None)
    E = ksw2_amd.KSW2AMD_E_PARAM if hasattr(ksw2_amd, "KSW2AMD_E_PARAM") else -2
    o.launches(sim, reset=True)
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, 128), (5, mp, -1, 2), (5, mp, 4, -1)):
        assert L.ksw2amd_ov_batch(*args, 3, 6, pairs, res) == E, args
        assert L.ksw2amd_ov_batch_flat(*args, 3, 6, ctypes.byref(f), res) == E, args
        assert L.ksw2amd_ovd_batch(*args, 24, 1, 3, 6, pairs, res) == E, args
        assert L.ksw2amd_ovd_batch_flat(*args, 24, 1, 3, 6, ctypes.byref(f), res) == E, args
    for c2 in ((128, 1), (24, 128), (-1, 1), (24, -1)):
        assert L.ksw2amd_ovd_batch(5, mp, 4, 2, *c2, 3, 6, pairs, res) == E, c2
        assert L.ksw2amd_ovd_batch_flat(5, mp, 4, 2, *c2, 3, 6, ctypes.byref(f), res) == E, c2
    for ends in (4, 7, 8, -1, 0x10001):                                     # a bit other than the two
        for r in res:
            r.score, r.qe, r.te = 7, 7, 7
        assert L.ksw2amd_ov_batch(5, mp, 4, 2, ends, 6, pairs, res) == E and "ends" in sim.last_error()
        assert L.ksw2amd_ov_batch_flat(5, mp, 4, 2, ends, 6, ctypes.byref(f), res) == E and "ends" in sim.last_error()
        assert L.ksw2amd_ovd_batch(5, mp, 4, 2, 24, 1, ends, 6, pairs, res) == E and "ends" in sim.last_error()
        assert L.ksw2amd_ovd_batch_flat(5, mp, 4, 2, 24, 1, ends, 6, ctypes.byref(f), res) == E and "ends" in sim.last_error()
        assert all((r.score, r.qe, r.te) == (7, 7, 7) for r in res)          # checked before anything is staged or reset
        assert sim.ov(q[0], t[0], mat, 4, 2, ends) == (0, -1, -1) and sim.ovd(q[0], t[0], mat, 4, 2, 24, 1, ends) == (0, -1, -1)
    assert L.ksw2amd_ov_batch(5, mp, 4, 2, 3, 6, None, res) == E and L.ksw2amd_ov_batch(5, mp, 4, 2, 3, 6, pairs, None) == E
    assert L.ksw2amd_ov_batch(5, mp, 4, 2, 3, -1, pairs, res) == E
    assert L.ksw2amd_ov_batch_flat(5, mp, 4, 2, 3, 6, None, res) == E and L.ksw2amd_ov_batch_flat(5, mp, 4, 2, 3, 6, ctypes.byref(f), None) == E
    bad_t = [x.copy() for x in t]
    bad_t[4][3] = 5
    bad_t[2][len(bad_t[2]) - 1] = 9
    for costs in ((4, 2), d.CROSS):
        with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
            o.call(sim, q, bad_t, mat, costs, 3, 5)
        out = np.full((6, 3), 7, np.int32)
        with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
            o.call_flat(sim, lf.arena(q, bad_t, lead=1, gap=2), mat, costs, 3, 5, out=out)
        assert (out == np.array([0, -1, -1])).all()
    # the range limit of the semi-global entries
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    ql = (0x3fffffff - 127 - 127) // (127 + 127) + 1
    pairs[1].qlen = ql
    assert L.ksw2amd_ov_batch(5, big.ctypes.data_as(_i8p), 127, 127, 3, 1, ctypes.byref(pairs[1]), res) == E
    assert "0x3fffffff" in sim.last_error()
    pairs[1].qlen = len(q[1])
    assert o.launches(sim)[:3] == (0, 0, 0)                                 # nothing of all this launched an alignment kernel
    before = sim.error_count()
    qe, te = ctypes.c_int(5), ctypes.c_int(5)
    assert L.ksw2amd_ov(None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, 3, ctypes.byref(qe), ctypes.byref(te)) == 0
    assert (qe.value, te.value) == (-1, -1) and sim.error_count() > before and "NULL profile" in sim.last_error()
    assert L.ksw2amd_ovd(None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, 24, 1, 3, ctypes.byref(qe), ctypes.byref(te)) == 0
    assert "NULL profile" in sim.last_error()


def test_chunked_flat_batches(sim):
    """KSW2AMD_LL_CHUNK_BYTES cuts the flat batch into several chunks: the same results; a bad code in a later chunk leaves the earlier
    chunks' results and resets its own and the later ones"""
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=40, m=5, qmax=100, tmax=200, long_targets=0)
    q[7], t[9] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    a = lf.arena(q, t, lead=1, gap=1)
    os.environ["KSW2AMD_LL_CHUNK_BYTES"] = "2000"
    for costs in ((4, 2), d.CROSS):
        exp = o.oracle_batch(q, t, mat, costs, 3, 5)
        o.launches(sim, reset=True)
        np.testing.assert_array_equal(o.call_flat(sim, a, mat, costs, 3, 5), exp)
        assert o.launches(sim)[3] > 3
        bad = a[0].copy()
        bad[int(a[3][30]) + 1] = 6
        out = np.full((40, 3), 7, np.int32)
        with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
            o.call_flat(sim, (bad,) + tuple(a[1:]), mat, costs, 3, 5, out=out)
        k = int(np.nonzero((out != exp).any(1))[0][0])
        assert 0 < k <= 30 and (out[:k] == exp[:k]).all() and (out[k:] == np.array([0, -1, -1])).all()


@pytest.mark.parametrize("pool", [False, True])
def test_c_caller(simso, tmp_path, pool):
    exe = str(tmp_path / "ov_caller")
    libdir = os.path.dirname(simso)
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "ov_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=12, m=5, qmax=80, tmax=300, long_targets=0)
    q.append(np.zeros(0, np.uint8)); t.append(t[0])
    q.append(q[0]); t.append(np.zeros(0, np.uint8))
    inp = str(tmp_path / "pairs.txt")
    o.write_input(inp, q, t, mat, 5, d.CROSS)
    out = subprocess.run([exe, inp] + (["pool"] if pool else []), check=True, capture_output=True, text=True).stdout.strip().splitlines()
    if pool:
        assert out[-1] == "pool %d" % (8 * len(q))                          # every profile came from the caller's pool
        out = out[:-1]
    k = 0
    for costs in (d.CROSS[:2], d.CROSS):
        if len(costs) == 4:
            assert out[k] == "two-piece"
            k += 1
        for ends in range(4):
            assert out[k] == "ends %d" % ends
            got = np.array([list(map(int, l.split())) for l in out[k + 1:k + 1 + len(q)]], dtype=np.int32)
            np.testing.assert_array_equal(got, o.oracle_batch(q, t, mat, costs, ends, 5), str((costs, ends)))
            k += 1 + len(q)
    assert k == len(out)


def test_other_host_objects_do_not_name_the_overlap_launchers(tmp_path):
    """only ksw2_host_ov.o refers to k2a_shim_launch_ov / k2a_shim_launch_ovd: the simulator builds of the other tests/*_util.py link the other
    host objects against twins without them"""
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    names = sorted(f[len("ksw2_host_"):-2] for f in os.listdir(csrc) if f.startswith("ksw2_host_") and f.endswith(".c"))
    assert "ov" in names and {"ll", "llf", "sg", "sga", "sgd"} <= set(names)
    for h in names:
        obj = str(tmp_path / ("host_%s.o" % h))
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", obj], check=True)
        undefined = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout.split()
        assert ("k2a_shim_launch_ov" in undefined) == (h == "ov") and ("k2a_shim_launch_ovd" in undefined) == (h == "ov"), (h, undefined)
