"""GPU: semi-global alignment under the two-piece gap cost (ksw2amd_sgd_batch / ksw2amd_sgd_align_batch, their flat forms and the single-pair
entries) on libksw2_amd.so against the contract (tests/sgd_oracle.c for score, tb, te; the scalar ksw_extd for the CIGAR), bit for bit, and
against tests/golden/sgd_cases.npz, which the compiled reference produced.  The shapes are the smallest at which k2a_sgd_kernel and
k2a_sgd_rev_kernel can go wrong: the best row on either side of a lane (16 rows) and of a generation (1 024 rows, the 16-byte boundary in
HBM), a long gap along either axis that is open across those boundaries, row -1 and column -1 past the point where the pieces cross, packed
halves that end in very different rows, the packed admission limit under B = min of the pieces, both orders of the pieces and zero costs."""
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
from tests import sgd_util as d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
CROSS = d.CROSS
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
        dev = lib.device_copy(base)
        try:
            yield dict(device_base=dev)
        finally:
            lib.device_free(dev)


def _tasks(err, n=None):
    """(pk_tasks, int32_tasks, profile) of the align entry's forward trace line; the start pass's line must name the same split, and no
    packed task is sent to the LDS profile behind the caller's back (K2A_SGD_PK_REG = 1)"""
    line = re.search(r"sgda: pairs=(\d+) pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
    assert line, err
    assert n is None or int(line.group(1)) == n, err
    rev = re.search(r"sgda-rev: pk_tasks=(\d+) int32_tasks=(\d+)", err)
    assert rev and rev.groups() == line.groups()[1:3], err
    assert "pk_profile=lds" not in err
    return int(line.group(2)), int(line.group(3)), line.group(4)


def _cells(got):
    return np.array(d.cells_of(got), dtype=np.int32).reshape(-1, 5)


def _check(lib, qs, ts, mat, costs, m, flag=0, msg="", exp=None, flat=False):
    """the align entry (and its flat form) against the contract, the score entry against its score, qe, te"""
    exp = d.expected(qs, ts, mat, costs, m, flag) if exp is None else exp
    d.assert_same(lib.sgd_align_batch(qs, ts, mat, *costs, flag=flag, m=m), exp, str(msg))
    want = np.array([[e["score"], e["qe"], e["te"]] for e in exp], dtype=np.int32).reshape(-1, 3)
    np.testing.assert_array_equal(lib.sgd_batch(qs, ts, mat, *costs, m=m), want, str(msg))
    if flat:
        ar = lf.arena(qs, ts, lead=3, gap=2)
        d.assert_same(lib.sgd_align_batch_flat(*ar, mat, *costs, flag=flag, m=m), exp, str((msg, "flat")))
        np.testing.assert_array_equal(lib.sgd_batch_flat(*ar, mat, *costs, m=m), want, str((msg, "flat")))
    return exp


# ---------------------------------------------------------------- 1. where the schedule changes hands

_grid = {}


@pytest.mark.parametrize("form,m", [("2", 5), ("0", 5), ("2", 20), ("0", 20)])
def test_edge_grid(lib, monkeypatch, capfd, form, m):
    """tlen {1, 15, 16, 17, 1 023, 1 024, 1 025, 2 049} x qlen {1, 2, 3, 5, 63, 64, 65}, the best row planted at 15 / 16 / 1 023 / 1 024 /
    tlen - 1; registers (m = 5) and LDS (m = 20), packed and int32, the pointer and the flat entry"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    if not _grid:
        qs, ts = s.edge_grid(np.random.default_rng(77), 5, qlens=(1, 2, 3, 5, 63, 64, 65))
        _grid.update(q=qs, t=ts)
    qs, ts = _grid["q"], _grid["t"]
    mat = s.unit_mat(m)
    if "exp%d" % m not in _grid:
        _grid["exp%d" % m] = d.expected(qs, ts, mat, CROSS, m)
    capfd.readouterr()
    exp = _check(lib, qs, ts, mat, CROSS, m, msg=(form, m), exp=_grid["exp%d" % m], flat=True)
    pk, i32, prof = _tasks(capfd.readouterr().err, len(qs))
    assert ((pk == 0) if form == "0" else (pk > 0 and i32 == 0)) and prof == ("registers" if m == 5 else "lds")
    assert {15, 16, 1023, 1024, 2048} <= {e["te"] for e in exp}


# ---------------------------------------------------------------- 2. the second piece along both axes

@pytest.mark.parametrize("form", ["2", "0"])
def test_long_gaps_along_rows_and_columns(lib, monkeypatch, capfd, form):
    """a copy of a 200-residue query with a 40-residue deletion (E2 down the rows: through the lane rotate at row 64 and, in rows
    1 000 .. 1 039, through the 16-byte HBM boundary) or a 40-residue insertion (F2 along the columns, in row 63 / 1 023), and a gap of one
    beside it: under (4, 2, 24, 1) they cost 64 and 6 -- (4, 2) alone pays 84 for the long one, (24, 1) alone 25 for the short one"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    rng = np.random.default_rng(8)
    mat = s.unit_mat(5)
    qs, ts, want = [], [], []
    for deletion, at, gap_at in ((True, 0, 60), (True, 950, 50), (False, 0, 64), (False, 950, 74)):
        q, t, (tb, te) = d.gapped_copy(rng, 1300, 200, at, gap_at, 40, deletion, short_at=170)
        qs.append(q); ts.append(t); want.append((2 * (199 if deletion else 159) - 64 - 6, tb, te))
    capfd.readouterr()
    exp = _check(lib, qs, ts, mat, CROSS, 5, msg=form, flat=True)
    pk, i32, _ = _tasks(capfd.readouterr().err, 4)
    assert (pk, i32) == ((0, 4) if form == "0" else (2, 0))                  # four pairs of one shape: two packed tasks
    assert [(e["score"], e["tb"], e["te"]) for e in exp] == want
    assert ts[1][1000:1040].max() <= 1                 # the deletion is open when lane 63 hands E2 to the boundary
    for go, ge in ((4, 2), (24, 1)):
        one = lib.sg_batch(qs, ts, mat, go, ge, m=5)
        assert all(int(r[0]) < w[0] for r, w in zip(one, want)), (go, ge, one)


# ---------------------------------------------------------------- 3. row -1 and column -1 under the second piece

@pytest.mark.parametrize("form", ["2", "0"])
def test_boundary_row_and_column_use_both_pieces(lib, monkeypatch, form):
    """target = query[30:] + other letters: the optimum inserts the first 30 query residues before target[0] at cost(30) = 54, not 64
    (fit_top).  The mirror image: the last 30 query residues are inserted behind the copy -- the reverse pass meets them along its row -1,
    and its column -1 runs past row 20, where the pieces cross (fit_left); the start deletes nothing."""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    rng = np.random.default_rng(12)
    mat = s.unit_mat(5)
    q1, t1 = d.suffix_copy(rng, 100, 30, 60)
    q2, t2 = d.suffix_copy(rng, 100, 30, 60, mirror=True)
    q3, t3 = d.suffix_copy(rng, 100, 30, 1200, mirror=True)                  # ... with the copy in the second generation
    exp = _check(lib, [q1, q2, q3], [t1, t2, t3], mat, CROSS, 5, msg=form, flat=True)
    assert [(e["score"], e["tb"], e["te"]) for e in exp] == [(86, 0, 69), (86, 60, 129), (86, 1200, 1269)]
    assert exp[0]["cigar"] == [30 << 4 | 1, 70 << 4]
    assert all(int(r[0]) == 76 for r in lib.sg_batch([q1, q2], [t1, t2], mat, 4, 2, m=5))      # one piece: cost(30) = 64


# ---------------------------------------------------------------- 4. both orders of the pieces, zero costs

_rag = {}


def _ragged():
    if not _rag:
        rng = np.random.default_rng(2024)
        qs, ts = d.ragged_batch(rng, 300, 5, 150, 1300)
        _rag.update(q=qs, t=ts, mats=(u.simple_mat(5, 2, 4, -1), u.random_mat(rng, 5, -7, 1)))
    return _rag


@pytest.mark.parametrize("costs", [(24, 1, 4, 2), (0, 1, 5, 0), (6, 3, 0, 0)])
def test_ragged_batch_both_orders_and_zero_costs(lib, monkeypatch, capfd, costs):
    """about 300 pairs of q 1-150 x t 1-1 300 under a match / mismatch matrix and under one without a positive entry: empty intervals,
    negative optima and ties are plentiful (under (6, 3, 0, 0) every gap is free, cost(l) = 0: no score is negative, and under the second
    matrix every interval is empty)"""
    c = _ragged()
    qs, ts = c["q"], c["t"]
    seen_empty = seen_neg = 0
    for k, mat in enumerate(c["mats"]):
        cells = d.oracle_cells(qs, ts, mat, costs, 5)
        for form in ("2", "0") if k else ("1",):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            capfd.readouterr()
            got = lib.sgd_align_batch(qs, ts, mat, *costs, m=5)
            _tasks(capfd.readouterr().err, len(qs))
            np.testing.assert_array_equal(_cells(got), cells, str((costs, k, form)))
            np.testing.assert_array_equal(lib.sgd_batch(qs, ts, mat, *costs, m=5), cells[:, [0, 2, 4]], str((costs, k, form)))
        sub = list(range(0, len(qs), 6))                                     # the CIGARs of every sixth pair against the scalar ksw_extd
        exp = d.expected([qs[i] for i in sub], [ts[i] for i in sub], mat, costs, 5, cells=cells[sub])
        d.assert_same([got[i] for i in sub], exp, str((costs, k)))
        seen_empty += int((cells[:, 3] == cells[:, 4] + 1).sum())
        seen_neg += int(((cells[:, 0] < 0) & (cells[:, 3] <= cells[:, 4])).sum())
    assert seen_empty > 20 and (seen_neg > 20 or costs[2:] == (0, 0))


# ---------------------------------------------------------------- 5. packed halves

@pytest.mark.parametrize("order", [0, 1])
def test_packed_halves_with_different_te_and_an_empty_interval(lib, monkeypatch, capfd, order):
    """two pairs of one shape whose copies end at rows ql + 5 and 2 090, in both orders: one packed task over the bounding rectangle; then
    an empty interval (the whole query inserted at cost(40) = 64) beside a copy that ends in row 2 090"""
    rng = np.random.default_rng(31 + order)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "1")
    mat = s.unit_mat(5)
    for ql in (40, 1030):
        qs, ts = a.uneven_halves(rng, 5, 2100, ql, (ql + 5, 2090))
        if order:
            qs, ts = qs[::-1], ts[::-1]
        capfd.readouterr()
        exp = _check(lib, qs, ts, mat, CROSS, 5, msg=(order, ql))
        assert _tasks(capfd.readouterr().err, 2)[:2] == (1, 0)
        assert sorted(e["te"] for e in exp) == [ql + 5, 2090] and all(e["te"] - e["tb"] + 1 == ql for e in exp)
    q1, t1 = a.planted_copy(rng, 5, 2100, 40, 2090)
    q2, t2 = rng.integers(2, 4, 40, dtype=np.uint8), rng.integers(0, 2, 2100, dtype=np.uint8)
    qs, ts = ([q1, q2], [t1, t2]) if order == 0 else ([q2, q1], [t2, t1])
    capfd.readouterr()
    exp = _check(lib, qs, ts, mat, CROSS, 5, msg=("empty", order))
    assert _tasks(capfd.readouterr().err, 2)[:2] == (1, 0)
    e = exp[1 - order]
    assert (e["score"], e["tb"], e["te"], e["cigar"]) == (-64, 1, 0, [40 << 4 | 1])


# ---------------------------------------------------------------- 6. the range of the two number formats

def test_packed_admission_limit(lib, monkeypatch, capfd):
    """smax = 127, costs (5, 3, 60, 1): B = 60 + qlen, 128 qlen + 187 <= 65 535 up to qlen 510 -- 510 is packed in both passes, 511 goes to
    int32.  Under the first piece alone (130 qlen + 132) 510 would not be admitted: B is the min"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    costs = (5, 3, 60, 1)
    for ql, tasks in ((510, (1, 0)), (511, (0, 1))):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q, rng.integers(0, 4, 9, dtype=np.uint8)])
        capfd.readouterr()
        exp = _check(lib, [q], [t], mat, costs, 4, msg=ql)
        assert _tasks(capfd.readouterr().err, 1)[:2] == tasks
        assert (exp[0]["score"], exp[0]["tb"], exp[0]["te"], exp[0]["cigar"]) == (127 * ql, 20, 20 + ql - 1, [ql << 4])
    capfd.readouterr()
    lib.sg_batch([q[:510]], [t], mat, 5, 3, m=4)
    assert "sg: pairs=1 pk_tasks=0 int32_tasks=1" in capfd.readouterr().err


def test_score_above_16_bits(lib, monkeypatch, capfd):
    rng = np.random.default_rng(4)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    q = rng.integers(0, 4, 2000, dtype=np.uint8)
    t = rng.integers(0, 4, 3000, dtype=np.uint8)
    t[700:2700] = u.mutate(rng, q, 4, 0.03, 0.0)[:2000]
    capfd.readouterr()
    exp = _check(lib, [q], [t], u.simple_mat(4, 40, 30), CROSS, 4)
    assert _tasks(capfd.readouterr().err, 1)[:2] == (0, 1)
    assert exp[0]["score"] > 65535 and (exp[0]["tb"], exp[0]["te"]) == (700, 2699)


# ---------------------------------------------------------------- 7. equal pieces

@pytest.mark.parametrize("costs", [(4, 2, 4, 2), (4, 2, 9, 5)])
def test_equal_or_dominated_second_piece_equals_the_single_piece_entries(lib, monkeypatch, costs):
    c = _ragged()
    qs, ts = c["q"], c["t"]
    for k, mat in enumerate(c["mats"]):
        monkeypatch.setenv("KSW2AMD_LL_FORM", "12"[k])
        np.testing.assert_array_equal(lib.sgd_batch(qs, ts, mat, *costs, m=5), lib.sg_batch(qs, ts, mat, costs[0], costs[1], m=5))
        one = lib.sg_align_batch(qs, ts, mat, costs[0], costs[1], m=5)
        two = lib.sgd_align_batch(qs, ts, mat, *costs, m=5)
        assert [{f: g[f] for f in d.FIELDS} for g in two] == [{f: g[f] for f in d.FIELDS} for g in one], (costs, k)


# ---------------------------------------------------------------- 8. the golden file

@pytest.mark.parametrize("form", ["1", "0"])
def test_golden_file(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    total = 0
    for name, m, mat, costs, q, t, cells, cig in d.load_golden():
        ar = lf.arena(q, t, lead=1, gap=3)
        for fl in d.FLAGS:
            got = lib.sgd_align_batch(q, t, mat, *costs, flag=fl, m=m)
            np.testing.assert_array_equal(_cells(got), cells, name)
            assert [g["cigar"] for g in got] == cig[fl], (name, fl)
            got = lib.sgd_align_batch_flat(*ar, mat, *costs, flag=fl, m=m)
            assert [g["cigar"] for g in got] == cig[fl] and (_cells(got) == cells).all(), (name, fl)
        np.testing.assert_array_equal(lib.sgd_batch(q, t, mat, *costs, m=m), cells[:, [0, 2, 4]], name)
        np.testing.assert_array_equal(lib.sgd_batch_flat(*ar, mat, *costs, m=m), cells[:, [0, 2, 4]], name)
        total += len(q)
    assert total == 324


# ---------------------------------------------------------------- 9. flags and CIGAR buffers

def test_flags_and_cigar_buffers(lib):
    """KSW_EZ_RIGHT / KSW_EZ_REV_CIGAR as the scalar ksw_extd places and orders them; buffers are reused; SCORE_ONLY leaves them alone"""
    rng = np.random.default_rng(6)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 16, 5, 20, 120, related=1.0)
    t = [np.concatenate([rng.integers(0, 5, 40, dtype=np.uint8), x]) for x in t]
    q.append(np.array([0, 0, 1, 1], np.uint8)); t.append(np.array([0, 0, 0, 1, 1], np.uint8))
    q.append(np.full(9, 2, np.uint8)); t.append(np.full(50, 1, np.uint8))                   # an empty interval
    cig = {fl: [e["cigar"] for e in _check(lib, q, t, mat, CROSS, 5, flag=fl, msg=fl)] for fl in (0, d.RIGHT, d.REV_CIGAR, d.RIGHT | d.REV_CIGAR)}
    assert cig[0] != cig[d.RIGHT] and cig[d.REV_CIGAR] == [c[::-1] for c in cig[0]] and cig[0][-1] == [9 << 4 | 1]
    exp = d.expected(q, t, mat, CROSS, 5)
    aln = (ka.LocalAln * len(q))()
    d.assert_same(lib.sgd_align_batch(q, t, mat, *CROSS, aln=aln), exp)
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    d.assert_same(lib.sgd_align_batch(q, t, mat, *CROSS, aln=aln), exp)
    assert [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    got = lib.sgd_align_batch(q, t, mat, *CROSS, flag=d.SCORE_ONLY, aln=aln)
    assert all(g["n_cigar"] == 0 for g in got) and [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    np.testing.assert_array_equal(_cells(got), _cells(exp))
    for x in aln:
        ka._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


# ---------------------------------------------------------------- 10. corners and bad arguments

def test_corners_and_bad_arguments(lib, capfd):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    e = np.zeros(0, np.uint8)
    q30 = np.array([0, 1, 2, 3, 0] * 6, np.uint8)                             # cost(30) = 54 under (4, 2, 24, 1)
    ins = dict(score=-54, qb=0, qe=29, tb=0, te=-1, n_cigar=1, cigar=[30 << 4 | 1])
    full = dict(score=60, qb=0, qe=29, tb=0, te=29, n_cigar=1, cigar=[30 << 4])
    capfd.readouterr()
    got = lib.sgd_align_batch([e, q30, e], [q30, e, e], mat, *CROSS, m=5)
    assert [{f: g[f] for f in d.FIELDS} for g in got] == [RESET, ins, RESET]
    assert lib.sgd_batch([e, q30, e], [q30, e, e], mat, *CROSS, m=5).tolist() == [[0, -1, -1], [-54, 29, -1], [0, -1, -1]]
    assert lib.sgd_align_batch([], [], mat, *CROSS, m=5) == []
    assert "pk_tasks=0 int32_tasks=0" in capfd.readouterr().err              # nothing to launch
    for got in (lib.sgd_align_batch([q30, e, q30], [e, q30, q30], mat, *CROSS, m=5),
                lib.sgd_align_batch_flat(*lf.arena([q30, e, q30], [e, q30, q30], lead=2, gap=1), mat, *CROSS, m=5)):
        assert [{f: g[f] for f in d.FIELDS} for g in got] == [ins, RESET, full]
    # every bad argument: KSW2AMD_E_PARAM before anything is staged or launched
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = lib.local_pairs(q, t)
    aln = (ka.LocalAln * 6)()
    res = np.zeros((6, 3), np.int32)
    rp = res.ctypes.data_as(ctypes.POINTER(ka.LocalResult))
    L = lib.lib
    mp = mat.ctypes.data_as(_i8p)
    ar = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = lib._local_flat(*ar, None)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    one = np.array([3], np.int8)
    zs = [np.zeros(4, np.uint8)] * 6
    zp, keepz = lib.local_pairs(zs, zs)
    bad_t = [x.copy() for x in t]
    bad_t[2][len(bad_t[2]) - 1] = 9
    stats = lib.host_stats()
    capfd.readouterr()
    for args in ((0, mp, 4, 2, 24, 1), (128, mp, 4, 2, 24, 1), (5, None, 4, 2, 24, 1), (5, mp, 128, 2, 24, 1), (5, mp, 4, 128, 24, 1),
                 (5, mp, 4, 2, 128, 1), (5, mp, 4, 2, 24, 128), (5, mp, 4, 2, -1, 1)):
        assert L.ksw2amd_sgd_align_batch(None, *args, 0, 6, pairs, aln) == -2, args
        assert L.ksw2amd_sgd_align_batch_flat(None, *args, 0, 6, ctypes.byref(f), aln) == -2, args
        assert L.ksw2amd_sgd_batch(*args, 6, pairs, rp) == -2, args
        assert L.ksw2amd_sgd_batch_flat(*args, 6, ctypes.byref(f), rp) == -2, args
    assert L.ksw2amd_sgd_align_batch(None, 1, one.ctypes.data_as(_i8p), 4, 2, 24, 1, 0, 6, zp, aln) == -2 and "m >= 2" in lib.last_error()
    for flag in (0x04, 0x40, 0x100):
        assert L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, flag, 6, pairs, aln) == -2
        assert L.ksw2amd_sgd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, flag, 6, ctypes.byref(f), aln) == -2
    assert L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, 0, 6, None, aln) == -2 and L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, 0, 6, pairs, None) == -2
    assert L.ksw2amd_sgd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, 0, 6, None, aln) == -2
    assert L.ksw2amd_sgd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, 0, 6, ctypes.byref(f), None) == -2
    with pytest.raises(ka.Ksw2Error, match=r"pair 2: residue code >= m"):
        lib.sgd_align_batch(q, bad_t, mat, *CROSS, m=5)
    pairs[1].qlen = (0x3fffffff - 127) // 127 + 1                            # the range limit under cost() = 0 (only the length is looked at)
    assert L.ksw2amd_sgd_align_batch(None, 5, big.ctypes.data_as(_i8p), 127, 127, 0, 0, 0, 2, pairs, aln) == -2 and "0x3fffffff" in lib.last_error()
    assert L.ksw2amd_sgd_batch(5, big.ctypes.data_as(_i8p), 127, 127, 0, 0, 2, pairs, rp) == -2
    pairs[1].qlen = len(q[1])
    before = lib.error_count()
    rec = ka.LocalAln()
    rec.score = 5
    assert L.ksw2amd_sgd_align(None, None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, 24, 1, 0, ctypes.byref(rec)) == 0
    assert (rec.score, rec.qb, rec.qe, rec.tb, rec.te, rec.n_cigar) == (0, -1, -1, -1, -1, 0) and lib.error_count() > before
    assert {k: v for k, v in lib.sgd_align(q[0], t[0], mat, 4, 2, 200, 1).items() if k in RESET} == RESET
    assert lib.sgd(q[0], t[0], mat, 4, 2, 24, 200) == (0, -1, -1)
    assert not re.search(r"sgda?(-rev)?: ", capfd.readouterr().err) and lib.host_stats() == stats     # no trace line: nothing was staged or launched by any of them


# ---------------------------------------------------------------- 11. flat arenas

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
    exp = d.expected([qq] * n, ts, mat, CROSS, 5)
    want = np.array([[e["score"], e["qe"], e["te"]] for e in exp], np.int32)
    with placed(lib, base, kind) as kw:
        capfd.readouterr()
        d.assert_same(lib.sgd_align_batch_flat(*ar, mat, *CROSS, m=5, **kw), exp, kind)
        assert ("arena=device" if kind == "device" else "arena=host") in capfd.readouterr().err
        monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "20000")
        capfd.readouterr()
        d.assert_same(lib.sgd_align_batch_flat(*ar, mat, *CROSS, flag=d.REV_CIGAR, m=5, **kw), d.expected([qq] * n, ts, mat, CROSS, 5, d.REV_CIGAR), kind)
        assert capfd.readouterr().err.count("sgda: pairs=") > 3
        np.testing.assert_array_equal(lib.sgd_batch_flat(*ar, mat, *CROSS, m=5, **kw), want)
        assert capfd.readouterr().err.count("sgd: pairs=") > 3
    bad = base.copy()
    bad[int(to[40]) + 2] = 5
    bad[int(to[45]) + int(tl[45]) - 1] = 200
    with placed(lib, bad, kind) as kw:
        aln = (ka.LocalAln * n)()
        with pytest.raises(ka.Ksw2Error, match=r"pair 40: residue code >= m"):
            lib.sgd_align_batch_flat(bad, *ar[1:], mat, *CROSS, m=5, aln=aln, **kw)
        assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)      # the earlier chunks' as well


# ---------------------------------------------------------------- 12. the single-pair entries, a C caller

def test_single_pair_and_c_caller(lib, tmp_path):
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 1, 80, related=0.8)
    t = [np.concatenate([rng.integers(0, 5, int(rng.integers(0, 1300)), dtype=np.uint8), x, rng.integers(0, 5, 50, dtype=np.uint8)]) for x in t]
    q += [np.zeros(0, np.uint8), q[0], np.full(6, 2, np.uint8)]
    t += [t[0], np.zeros(0, np.uint8), np.full(30, 1, np.uint8)]
    q2, t2, _ = d.gapped_copy(rng, 1300, 200, 950, 50, 40, True, short_at=170)
    q.append(q2); t.append(t2)
    exe = str(tmp_path / "sgd_caller")
    libdir = os.path.dirname(os.path.abspath(lib.path))
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "sgd_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    for flag in (0, d.RIGHT | d.REV_CIGAR):
        exp = d.expected(q, t, mat, CROSS, 5, flag)
        d.assert_same([lib.sgd_align(q[i], t[i], mat, *CROSS, flag=flag) for i in range(len(q))], exp, "single")
        assert [lib.sgd(q[i], t[i], mat, *CROSS) for i in range(len(q))] == [(e["score"], e["qe"], e["te"]) for e in exp]
        inp = str(tmp_path / "pairs.txt")
        d.write_input(inp, q, t, mat, 5, CROSS, flag)
        out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
        batch, single, _ = la.parse_caller(out)
        d.assert_same(batch, exp, "batch")
        d.assert_same(single, exp, "single")
