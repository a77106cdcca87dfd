"""GPU: semi-global alignment with the start of the interval and a CIGAR (ksw2amd_sg_align_batch / ksw2amd_sg_align_batch_flat /
ksw2amd_sg_align) on libksw2_amd.so against the contract (tests/sga_oracle.c for score, tb, te; the scalar ksw_extz for the CIGAR), bit for
bit, and against tests/golden/sga_cases.npz, which the compiled reference produced.  The shapes are the smallest at which the anchored
reverse pass (k2a_sg_rev_kernel) can go wrong: rl = te + 1 and the interval's length on either side of a lane (16 rows) and of a generation
(1 024 rows, the boundary in HBM), packed tasks whose halves end in very different rows, empty intervals, ties under free gaps, the packed
admission limit, scores beyond 16 bits, negative optima, matrices without a positive entry."""
import contextlib
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_util as u
from tests import llf_util as lf
from tests import lla_util as la
from tests import sg_util as s
from tests import sga_util as a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (6, 1), (0, 0))
CELL = ("score", "qb", "qe", "tb", "te")
RESET = dict(score=0, qb=-1, qe=-1, tb=-1, te=-1, n_cigar=0, cigar=[])


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS", "KSW2AMD_ABORT_ON_ERROR"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")


@contextlib.contextmanager
def placed(lib, base, kind):
    """the arena as the call sees it -> keyword arguments for the flat methods"""
    if kind == "host":
        yield dict()
    elif kind == "pinned":
        assert lib.lib.ksw2amd_host_register(ctypes.c_void_p(base.ctypes.data), ctypes.c_size_t(base.nbytes)) == 0, lib.last_error()
        try:
            yield dict()
        finally:
            lib.lib.ksw2amd_host_unregister(ctypes.c_void_p(base.ctypes.data))
    else:
        d = lib.device_copy(base)
        try:
            yield dict(device_base=d)
        finally:
            lib.device_free(d)


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 3)
    return mat.reshape(-1)


def _tasks(err, n=None):
    """(pk_tasks, int32_tasks, profile) of the forward trace line; the start pass's line must name the same split"""
    line = re.search(r"sga: pairs=(\d+) pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
    assert line, err
    assert n is None or int(line.group(1)) == n, err
    rev = re.search(r"sga-rev: pk_tasks=(\d+) int32_tasks=(\d+)", err)
    assert rev and rev.groups() == line.groups()[1:3], err
    return int(line.group(2)), int(line.group(3)), line.group(4)


def _cells(got):
    return np.array([[g[f] for f in CELL] for g in got], dtype=np.int32).reshape(-1, 5)


def _check(lib, qs, ts, mat, gapo, gape, m, flag=0, msg="", exp=None):
    exp = a.expected(qs, ts, mat, gapo, gape, m, flag) if exp is None else exp
    got = lib.sg_align_batch(qs, ts, mat, gapo, gape, flag=flag, m=m)
    a.assert_same(got, exp, str(msg))
    return exp


# ---------------------------------------------------------------- ragged batches

_ragged = {}


def _ragged_pairs(m):
    """4 000 pairs of q 1-200 x t 1-1 500, a third with a mutated copy of the query in the target, and 40 pairs with targets up to 5 000
    (five generations, the boundary in HBM); made once per m, the oracle's cells once per (m, costs)"""
    if m not in _ragged:
        rng = np.random.default_rng(2000 + m)
        qs, ts = [], []
        for k in range(4040):
            big = k >= 4000
            q = rng.integers(0, m, int(rng.integers(1, 201)), dtype=np.uint8)
            t = rng.integers(0, m, int(rng.integers(4000, 5001)) if big else int(rng.integers(1, 1501)), dtype=np.uint8)
            if (k % 3 == 0 or big) and len(t) > len(q):
                c = u.mutate(rng, q, m, 0.05, 0.04)[:len(t)]
                at = int(rng.integers(0, len(t) - len(c) + 1))
                t[at:at + len(c)] = c
            qs.append(q); ts.append(t)
        mat = u.simple_mat(5, 2, 4, -1) if m == 5 else _m20(rng)
        _ragged[m] = (qs, ts, mat)
    return _ragged[m]


@pytest.mark.parametrize("m", [5, 20])
@pytest.mark.parametrize("costs", COSTS)
def test_ragged_batch(lib, monkeypatch, capfd, m, costs):
    qs, ts, mat = _ragged_pairs(m)
    if costs[1] != 1:                                                        # (4, 2) and (0, 0): packed for every admissible pair
        monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    cells = a.oracle_cells(qs, ts, mat, *costs, m)
    capfd.readouterr()
    got = lib.sg_align_batch(qs, ts, mat, *costs, m=m)
    pk, i32, prof = _tasks(capfd.readouterr().err, len(qs))
    np.testing.assert_array_equal(_cells(got), cells, str((m, costs)))
    np.testing.assert_array_equal(cells[:, [0, 2, 4]], lib.sg_batch(qs, ts, mat, *costs, m=m))          # score, qe, te: sg_batch's bit for bit
    assert prof == ("registers" if m == 5 else "lds") and pk + i32 > 0 and (costs[1] == 1 or (pk > 2000 and i32 == 0))
    sub = list(range(0, len(qs), 8))                                         # the CIGARs of every eighth pair against the scalar ksw_extz
    exp = a.expected([qs[i] for i in sub], [ts[i] for i in sub], mat, *costs, m, cells=cells[sub])
    a.assert_same([got[i] for i in sub], exp, str((m, costs)))
    assert all(g["n_cigar"] > 0 for g in got)
    assert (cells[:, 3] <= cells[:, 4]).sum() > 1000


_forms = {}


def _form_case():
    if not _forms:
        rng = np.random.default_rng(50)
        mat = u.simple_mat(5, 2, 4, -1)
        qs = [rng.integers(0, 4, 100, dtype=np.uint8) for _ in range(512)] + [rng.integers(0, 4, 300, dtype=np.uint8) for _ in range(6)]
        ts = [rng.integers(0, 4, 1024, dtype=np.uint8) for _ in range(512)] + [rng.integers(0, 4, 2500, dtype=np.uint8) for _ in range(6)]
        for i in range(0, 518, 2):
            at = int(rng.integers(0, len(ts[i]) - len(qs[i]) + 1))
            ts[i][at:at + len(qs[i])] = u.mutate(rng, qs[i], 4, 0.05, 0.0)[:len(qs[i])]
        _forms.update(q=qs, t=ts, mat=mat, cells=a.oracle_cells(qs, ts, mat, 4, 2, 5))
    return _forms


@pytest.mark.parametrize("form", ["0", "1", "2"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_forced_forms(lib, monkeypatch, capfd, form, lds):
    """512 same-shape pairs of 100 x 1 024 (every other one with a copy: the halves of a packed task end in different rows) plus six of
    300 x 2 500 under every KSW2AMD_LL_FORM x KSW2AMD_LL_LDS"""
    c = _form_case()
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
    capfd.readouterr()
    got = lib.sg_align_batch(c["q"], c["t"], c["mat"], 4, 2, flag=a.SCORE_ONLY, m=5)
    pk, i32, prof = _tasks(capfd.readouterr().err, 518)
    np.testing.assert_array_equal(_cells(got), c["cells"], str((form, lds)))
    assert (pk, i32) == ((0, 518) if form == "0" else (259, 0)) and prof == ("lds" if lds == "1" else "registers")


# ---------------------------------------------------------------- where the reversed schedule changes hands

_grid = {}


@pytest.mark.parametrize("form,m", [("2", 5), ("0", 5), ("2", 20), ("0", 20)])
def test_edge_grid(lib, monkeypatch, capfd, form, m):
    """qlen {1, 2, 15, 16, 17, 63, 64, 65, 1 023, 1 024, 1 025} in targets of 17 / 1 025 / 2 049, a lightly mutated copy of the query ending
    at te in {qlen - 1, 15, 16, 1 023, 1 024, tlen - 1}: rl = te + 1 lands on 16 / 17 / 1 024 / 1 025, interval lengths on either side of
    a lane and of a generation"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    cases = a.edge_cases()
    if not _grid:
        qs, ts = a.edge_grid(np.random.default_rng(77), 5, cases)
        _grid.update(q=qs, t=ts)
    qs, ts = _grid["q"], _grid["t"]
    mat = s.unit_mat(m)
    capfd.readouterr()
    exp = _check(lib, qs, ts, mat, 4, 2, m, msg=(form, m))
    pk, i32, _ = _tasks(capfd.readouterr().err, len(qs))
    a.assert_same(lib.sg_align_batch_flat(*lf.arena(qs, ts, lead=3, gap=2), mat, 4, 2, m=m), exp, str((form, m, "flat")))
    assert (pk == 0) if form == "0" else (pk > 0 and i32 == 0)
    lens, ends = set(), set()
    for (tl, ql, te), e in zip(cases, exp):
        assert e["te"] == te and ql - 1 <= te - e["tb"] + 1 <= ql, (tl, ql, te, e)
        lens.add(te - e["tb"] + 1); ends.add(te)
    assert {15, 16, 1023, 1024, 2048} <= ends and {1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025} <= lens


@pytest.mark.parametrize("order", [0, 1])
def test_packed_halves_with_different_te_and_an_empty_interval(lib, monkeypatch, capfd, order):
    """two pairs of one shape whose copies end at rows ql + 5 and 2 090, in both orders: one packed task over the bounding rectangle; then
    an empty interval (the whole query inserted) beside a copy that ends in row 2 090"""
    rng = np.random.default_rng(31 + order)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "1")
    mat = s.unit_mat(5)
    for ql in (40, 1030):
        qs, ts = a.uneven_halves(rng, 5, 2100, ql, (ql + 5, 2090))
        if order:
            qs, ts = qs[::-1], ts[::-1]
        capfd.readouterr()
        exp = _check(lib, qs, ts, mat, 4, 2, 5, msg=(order, ql))
        assert _tasks(capfd.readouterr().err, 2)[:2] == (1, 0)
        assert sorted(e["te"] for e in exp) == [ql + 5, 2090] and all(e["te"] - e["tb"] + 1 == ql for e in exp)
    q1, t1 = a.planted_copy(rng, 5, 2100, 40, 2090)
    q2, t2 = rng.integers(2, 4, 40, dtype=np.uint8), rng.integers(0, 2, 2100, dtype=np.uint8)
    qs, ts = ([q1, q2], [t1, t2]) if order == 0 else ([q2, q1], [t2, t1])
    capfd.readouterr()
    exp = _check(lib, qs, ts, mat, 4, 2, 5, msg=("empty", order))
    assert _tasks(capfd.readouterr().err, 2)[:2] == (1, 0)
    e = exp[1 - order]
    assert (e["score"], e["tb"], e["te"], e["cigar"]) == (-84, 1, 0, [40 << 4 | 1])


@pytest.mark.parametrize("m", [5, 20])
def test_empty_intervals_negative_optima_and_ties(lib, monkeypatch, m):
    """matrices without a positive entry (empty intervals are plentiful, optima negative) and free gaps (0, 0), (3, 0), (0, 1): many
    starts tie, the largest is the answer; packed and int32"""
    rng = np.random.default_rng(8 + m)
    qs, ts = u.ragged(rng, 60, m, 1, 150)
    ts = [np.concatenate([rng.integers(0, m, int(rng.integers(0, 1200)), dtype=np.uint8), x]) for x in ts]
    seen_empty = seen_neg = 0
    for mat, costs in ((u.random_mat(rng, m, -7, 1), (3, 1)), (u.random_mat(rng, m, -7, 1), (0, 0)), (s.unit_mat(m), (0, 0)),
                       (s.unit_mat(m), (3, 0)), (u.random_mat(rng, m, -3, 2), (0, 1))):
        cells = a.oracle_cells(qs, ts, mat, *costs, m)
        exp = a.expected(qs, ts, mat, *costs, m, cells=cells)
        for form in ("2", "0"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            a.assert_same(lib.sg_align_batch(qs, ts, mat, *costs, m=m), exp, str((costs, form)))
        seen_empty += int((cells[:, 3] == cells[:, 4] + 1).sum())
        seen_neg += int(((cells[:, 0] < 0) & (cells[:, 3] <= cells[:, 4])).sum())
    assert seen_empty > 20 and seen_neg > 20
    # a strongly negative optimum with a real interval (dear gaps), and the all-insert optimum: te = 0, tb = 1
    q, t = np.zeros(40, np.uint8), np.ones(1300, np.uint8)
    for costs, expect in (((120, 110), None), ((2, 1), (-42, 0, 39, 1, 0))):
        for form in ("2", "0"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            exp = _check(lib, [q], [t], u.simple_mat(4, 1, 100), *costs, 4, msg=(costs, form))
            assert exp[0]["score"] < -40 and (expect is None or tuple(exp[0][f] for f in CELL) == expect)


# ---------------------------------------------------------------- the range of the two number formats

def test_packed_admission_limit(lib, monkeypatch, capfd):
    """smax = 127, costs (5, 1): 128 qlen + 132 <= 65 535 up to qlen 510 -- 510 is packed in both passes, 511 goes to int32"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    for ql, tasks in ((510, (1, 0)), (511, (0, 1))):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q, rng.integers(0, 4, 9, dtype=np.uint8)])
        capfd.readouterr()
        exp = _check(lib, [q], [t], mat, 5, 1, 4, msg=ql)
        assert _tasks(capfd.readouterr().err, 1)[:2] == tasks
        assert (exp[0]["score"], exp[0]["tb"], exp[0]["te"], exp[0]["cigar"]) == (127 * ql, 20, 20 + ql - 1, [ql << 4])


def test_score_above_16_bits(lib, monkeypatch, capfd):
    rng = np.random.default_rng(4)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    q = rng.integers(0, 4, 2000, dtype=np.uint8)
    t = rng.integers(0, 4, 3000, dtype=np.uint8)
    t[700:2700] = u.mutate(rng, q, 4, 0.03, 0.0)[:2000]
    capfd.readouterr()
    exp = _check(lib, [q], [t], u.simple_mat(4, 40, 30), 4, 2, 4)
    assert _tasks(capfd.readouterr().err, 1)[:2] == (0, 1)
    assert exp[0]["score"] > 65535 and (exp[0]["tb"], exp[0]["te"]) == (700, 2699)


# ---------------------------------------------------------------- flags, buffers, golden file

def test_flags_and_cigar_buffers(lib):
    """KSW_EZ_RIGHT / KSW_EZ_REV_CIGAR as the scalar ksw_extz places and orders them; buffers are reused; SCORE_ONLY leaves them alone"""
    rng = np.random.default_rng(6)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 16, 5, 20, 120, related=1.0)
    t = [np.concatenate([rng.integers(0, 5, 40, dtype=np.uint8), x]) for x in t]
    q.append(np.array([0, 0, 1, 1], np.uint8)); t.append(np.array([0, 0, 0, 1, 1], np.uint8))
    q.append(np.full(9, 2, np.uint8)); t.append(np.full(50, 1, np.uint8))                   # an empty interval
    cig = {fl: [e["cigar"] for e in _check(lib, q, t, mat, 4, 2, 5, flag=fl, msg=fl)] for fl in (0, a.RIGHT, a.REV_CIGAR, a.RIGHT | a.REV_CIGAR)}
    assert cig[0] != cig[a.RIGHT] and cig[a.REV_CIGAR] == [c[::-1] for c in cig[0]] and cig[0][-1] == [9 << 4 | 1]
    exp = a.expected(q, t, mat, 4, 2, 5)
    for e, qq, tt in zip(exp[:-1], q, t):
        assert la.rescore(e["cigar"], qq, tt[e["tb"]:e["te"] + 1], mat, 5, 4, 2) == (e["score"], len(qq), e["te"] - e["tb"] + 1)
    aln = (ka.LocalAln * len(q))()
    a.assert_same(lib.sg_align_batch(q, t, mat, 4, 2, aln=aln), exp)
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    a.assert_same(lib.sg_align_batch(q, t, mat, 4, 2, aln=aln), exp)
    assert [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    got = lib.sg_align_batch(q, t, mat, 4, 2, flag=a.SCORE_ONLY, aln=aln)
    assert all(g["n_cigar"] == 0 for g in got) and [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    np.testing.assert_array_equal(_cells(got), _cells(exp))
    for x in aln:
        ka._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


@pytest.mark.parametrize("form", ["1", "0"])
def test_golden_file(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    total = 0
    for name, m, mat, gapo, gape, q, t, cells, cig in a.load_golden():
        for fl in a.FLAGS:
            got = lib.sg_align_batch(q, t, mat, gapo, gape, flag=fl, m=m)
            np.testing.assert_array_equal(_cells(got), cells, name)
            assert [g["cigar"] for g in got] == cig[fl], (name, fl)
        got = lib.sg_align_batch_flat(*lf.arena(q, t, lead=1, gap=3), mat, gapo, gape, m=m)
        assert [g["cigar"] for g in got] == cig[0] and (_cells(got) == cells).all(), name
        total += len(q)
    assert total == 324


# ---------------------------------------------------------------- corners and bad arguments

def test_corners_and_bad_arguments(lib, capfd):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    e = np.zeros(0, np.uint8)
    q5 = np.array([0, 1, 2, 3, 0], np.uint8)
    ins = dict(score=-14, qb=0, qe=4, tb=0, te=-1, n_cigar=1, cigar=[5 << 4 | 1])
    capfd.readouterr()
    got = lib.sg_align_batch([e, q5, e], [q5, e, e], mat, 4, 2, m=5)
    assert [{f: g[f] for f in a.FIELDS} for g in got] == [RESET, ins, RESET]
    assert lib.sg_align_batch([], [], mat, 4, 2, m=5) == []
    assert "pk_tasks=0 int32_tasks=0" in capfd.readouterr().err              # nothing to launch
    for got in (lib.sg_align_batch([q5, e, q5], [e, q5, q5], mat, 4, 2, m=5),
                lib.sg_align_batch_flat(*lf.arena([q5, e, q5], [e, q5, q5], lead=2, gap=1), mat, 4, 2, m=5)):
        assert [{f: g[f] for f in a.FIELDS} for g in got] == [ins, RESET, dict(score=10, qb=0, qe=4, tb=0, te=4, n_cigar=1, cigar=[5 << 4])]
    # every bad argument: KSW2AMD_E_PARAM before anything is staged or launched
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = lib.local_pairs(q, t)
    aln = (ka.LocalAln * 6)()
    L = lib.lib
    mp = mat.ctypes.data_as(_i8p)
    ar = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = lib._local_flat(*ar, None)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    ql = (0x3fffffff - 127 - 127) // (127 + 127) + 1
    bad_t = [x.copy() for x in t]
    bad_t[2][len(bad_t[2]) - 1] = 9
    stats = lib.host_stats()
    capfd.readouterr()
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, 128), (5, mp, -1, 2)):
        assert L.ksw2amd_sg_align_batch(None, *args, 0, 6, pairs, aln) == -2, args
        assert L.ksw2amd_sg_align_batch_flat(None, *args, 0, 6, ctypes.byref(f), aln) == -2, args
    for flag in (0x04, 0x40, 0x100):
        assert L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, flag, 6, pairs, aln) == -2
        assert L.ksw2amd_sg_align_batch_flat(None, 5, mp, 4, 2, flag, 6, ctypes.byref(f), aln) == -2
    assert L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, 0, 6, None, aln) == -2 and L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, 0, 6, pairs, None) == -2
    assert L.ksw2amd_sg_align_batch_flat(None, 5, mp, 4, 2, 0, 6, None, aln) == -2 and L.ksw2amd_sg_align_batch_flat(None, 5, mp, 4, 2, 0, 6, ctypes.byref(f), None) == -2
    with pytest.raises(ka.Ksw2Error, match=r"pair 2: residue code >= m"):
        lib.sg_align_batch(q, bad_t, mat, 4, 2, m=5)
    pairs[1].qlen = ql                                                       # the range limit (only the length is looked at)
    assert L.ksw2amd_sg_align_batch(None, 5, big.ctypes.data_as(_i8p), 127, 127, 0, 2, pairs, aln) == -2 and "0x3fffffff" in lib.last_error()
    pairs[1].qlen = len(q[1])
    before = lib.error_count()
    one = ka.LocalAln()
    one.score = 5
    assert L.ksw2amd_sg_align(None, None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, 0, ctypes.byref(one)) == 0
    assert (one.score, one.qb, one.qe, one.tb, one.te, one.n_cigar) == (0, -1, -1, -1, -1, 0) and lib.error_count() > before
    assert {k: v for k, v in lib.sg_align(q[0], t[0], mat, 200, 2).items() if k in RESET} == RESET
    assert "sga: pairs" not in capfd.readouterr().err and lib.host_stats() == stats     # nothing was staged or launched by any of them


# ---------------------------------------------------------------- flat arenas, the single-pair entry, a C caller

@pytest.mark.parametrize("kind", ["host", "pinned", "device"])
def test_flat_arenas(lib, monkeypatch, capfd, kind):
    """a host arena, a page-locked arena and a device arena equal the pointer entry, chunked as well; a code >= m inside a referenced
    sequence is caught on the device with the lowest pair named and resets EVERY entry, a bad byte between sequences is ignored"""
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    qq = rng.integers(0, 5, 150, dtype=np.uint8)
    ts = [np.concatenate([rng.integers(0, 5, int(rng.integers(1, 1400)), dtype=np.uint8), u.mutate(rng, qq, 5, 0.05, 0.1),
                          rng.integers(0, 5, int(rng.integers(0, 300)), dtype=np.uint8)]) for _ in range(64)]
    base, qo, ql, to, tl = lf.arena([qq], ts, lead=1, gap=3, fill=255)       # 255 between the sequences: never looked at
    n = len(ts)
    ar = (base, np.repeat(qo, n), np.repeat(ql, n), to, tl)                 # ONE copy of the query in the arena
    exp = a.expected([qq] * n, ts, mat, 4, 2, 5)
    with placed(lib, base, kind) as kw:
        capfd.readouterr()
        a.assert_same(lib.sg_align_batch_flat(*ar, mat, 4, 2, m=5, **kw), exp, kind)
        assert ("arena=device" if kind == "device" else "arena=host") in capfd.readouterr().err
        monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "20000")
        capfd.readouterr()
        a.assert_same(lib.sg_align_batch_flat(*ar, mat, 4, 2, flag=a.REV_CIGAR, m=5, **kw), a.expected([qq] * n, ts, mat, 4, 2, 5, a.REV_CIGAR), kind)
        assert capfd.readouterr().err.count("sga: pairs=") > 3
    bad = base.copy()
    bad[int(to[40]) + 2] = 5
    bad[int(to[45]) + int(tl[45]) - 1] = 200
    with placed(lib, bad, kind) as kw:
        aln = (ka.LocalAln * n)()
        with pytest.raises(ka.Ksw2Error, match=r"pair 40: residue code >= m"):
            lib.sg_align_batch_flat(bad, *ar[1:], mat, 4, 2, m=5, aln=aln, **kw)
        assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)      # the earlier chunks' as well


def test_single_pair_and_c_caller(lib, tmp_path):
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 1, 80, related=0.8)
    t = [np.concatenate([rng.integers(0, 5, int(rng.integers(0, 1300)), dtype=np.uint8), x, rng.integers(0, 5, 50, dtype=np.uint8)]) for x in t]
    q += [np.zeros(0, np.uint8), q[0], np.full(6, 2, np.uint8)]
    t += [t[0], np.zeros(0, np.uint8), np.full(30, 1, np.uint8)]
    for flag in (0, a.RIGHT | a.REV_CIGAR):
        exp = a.expected(q, t, mat, 4, 2, 5, flag)
        a.assert_same([lib.sg_align(q[i], t[i], mat, 4, 2, flag=flag) for i in range(len(q))], exp, "single")
        exe = str(tmp_path / "sga_caller")
        libdir = os.path.dirname(os.path.abspath(lib.path))
        subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "dropin", "sga_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
        inp = str(tmp_path / "pairs.txt")
        la.write_input(inp, q, t, mat, 5, 4, 2, flag)
        out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
        batch, single, _ = la.parse_caller(out)
        a.assert_same(batch, exp, "batch")
        a.assert_same(single, exp, "single")
