"""GPU: overlap alignment with the start cell and a CIGAR (ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch, their flat forms and the
single-pair entries) on libksw2_amd.so against the contract (tests/ova_oracle.c for score, qb, qe, tb, te; the scalar ksw_extz / ksw_extd for
the CIGAR), bit for bit, and against tests/golden/ova_cases.npz, which the compiled reference produced.  The shapes are the smallest at which
the anchored start pass of this mode (k2a_ov_rev_kernel / k2a_ovd_rev_kernel) can go wrong: the reversed rectangle's rows on either side of a
lane (16 rows) and of a generation (1 024 rows, the boundary in HBM), its column limit qe at the prefetch depth and the 63-step skew, the last
row as a candidate row with its owner in either generation, packed tasks whose halves disagree in te, in qe and in the owning generation,
empty intervals of both kinds, ties, scores and columns beyond the packed range, negative optima, free gaps."""
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
from tests import ov_util as o
from tests import ova_util as a
from tests import sg_util as s
from tests import sga_util as sa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (0, 0), (4, 2, 24, 1), (24, 1, 4, 2))
RESET = dict(score=0, qb=-1, qe=-1, tb=-1, te=-1, n_cigar=0, cigar=[])
FORMS = [("2", 5), ("0", 5), ("2", 20), ("0", 20)]


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


def _tn(costs):
    return "ovda" if len(costs) == 4 else "ova"


def _tasks(err, costs, n=None):
    """(pk_tasks, int32_tasks, profile) of the forward trace line; the start pass's line must name the same split"""
    line = re.search(r"\] %s: pairs=(\d+) pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)" % _tn(costs), err)
    assert line, err
    assert n is None or int(line.group(1)) == n, err
    rev = re.search(r"\] %s-rev: pk_tasks=(\d+) int32_tasks=(\d+)" % _tn(costs), err)
    assert rev and rev.groups() == line.groups()[1:3], err
    return int(line.group(2)), int(line.group(3)), line.group(4)


def _cells(got):
    return np.array(a.cells_of(got), dtype=np.int32).reshape(-1, 5)


def _check(lib, qs, ts, mat, costs, ends, m, flag=0, msg="", exp=None):
    exp = a.expected(qs, ts, mat, costs, ends, m, flag) if exp is None else exp
    a.assert_same(a.call(lib, qs, ts, mat, costs, ends, m, flag), exp, str((msg, costs, ends)))
    return exp


def _forms_check(lib, monkeypatch, capfd, qs, ts, costs, ends, form, m, flag=a.SCORE_ONLY):
    """one group under one form, the packed / int32 split asserted from the trace line"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = s.unit_mat(m)
    capfd.readouterr()
    exp = _check(lib, qs, ts, mat, costs, ends, m, flag, msg=(form, m))
    pk, i32, prof = _tasks(capfd.readouterr().err, costs, len(qs))
    assert ((pk == 0) if form == "0" else (pk > 0 and i32 == 0)) and prof == ("registers" if m == 5 else "lds")
    return exp


# ---------------------------------------------------------------- 1. start-row grid

_rows = {}


@pytest.mark.parametrize("form,m", FORMS)
def test_start_row_grid(lib, monkeypatch, capfd, form, m):
    """te - tb on both sides of 15 / 16 / 17 and 1 023 / 1 024 / 1 025 -- rows per lane and per generation of the reversed rectangle --
    with tb = 0 exactly, tb = 1 and tb = 7; the empty target interval beside them"""
    if not _rows:
        rng = np.random.default_rng(70)
        qs, ts, want = [], [], []
        for span in (15, 16, 17, 18, 1023, 1024, 1025, 1026):
            for lead in (0, 1, 7):
                q, t = a.start_row_pair(rng, span + lead, span)
                qs.append(q); ts.append(t); want.append((0, lead, span + lead - 1))
        _rows.update(q=qs, t=ts, want=want, empty=a.start_row_pair(rng, 1030, 1, empty=True))
    for costs in ((4, 2), (4, 2, 24, 1)):
        for ends in (2, 3):
            exp = _forms_check(lib, monkeypatch, capfd, _rows["q"], _rows["t"], costs, ends, form, m)
            assert [(e["qb"], e["tb"], e["te"]) for e in exp] == _rows["want"]
    q, t = _rows["empty"]
    e = _check(lib, [q], [t], s.unit_mat(m), (1, 1), 2, m, msg="empty")[0]
    assert (e["score"], e["tb"], e["te"], e["cigar"]) == (-2, 1, 0, [1 << 4 | 1])


# ---------------------------------------------------------------- 2. last-column grid (QEND)

_cols = {}


@pytest.mark.parametrize("form,m", FORMS)
def test_last_column_grid(lib, monkeypatch, capfd, form, m):
    """qe at 0, 1, 3, 4, 5, 62, 63, 64, 65, qlen - 2 and qlen - 1 with te = tlen - 1: the prefetch depth and the 63-step skew on the
    rectangle's column limit, targets of one lane, one generation and two"""
    if not _cols:
        qs, ts, what = o.qend_grid(np.random.default_rng(72), tlens=(8, 17, 1025), qlens=(5, 6, 64, 65, 67, 130))
        _cols.update(q=qs, t=ts, what=what)
    for costs in ((4, 2), (24, 1, 4, 2)):
        exp = _forms_check(lib, monkeypatch, capfd, _cols["q"], _cols["t"], costs, 2, form, m)
        seen = {e["qe"] for (tl, ql, p), e in zip(_cols["what"], exp) if e["te"] == tl - 1}
        assert {0, 1, 3, 4, 5, 62, 63, 64, 65, 66, 128, 129} <= seen, sorted(seen)
        _forms_check(lib, monkeypatch, capfd, _cols["q"], _cols["t"], costs, 3, form, m)


# ---------------------------------------------------------------- 3. last-row grid (QBEG)

_lastrow = {}


@pytest.mark.parametrize("form,m", FORMS)
def test_last_row_grid(lib, monkeypatch, capfd, form, m):
    """the best start is (0, qb): qb around 1, 4, 63, 64, 65 and the last row te at 0, 15, 16, 1 023, 1 024; qb = qe (the shortest query
    interval); qb = qe + 1, the (te + 1) D case"""
    if not _lastrow:
        rng = np.random.default_rng(71)
        qs, ts, want = [], [], []
        for te in (0, 15, 16, 1023, 1024):
            for qb in (1, 3, 4, 5, 63, 64, 65):
                q, t = a.qbeg_start_pair(rng, te, qb, qb + te + 1)
                qs.append(q); ts.append(t); want.append((qb, qb + te, 0, te))
        _lastrow.update(q=qs, t=ts, want=want)
    for costs in ((4, 2), (4, 2, 24, 1)):
        exp = _forms_check(lib, monkeypatch, capfd, _lastrow["q"], _lastrow["t"], costs, 1, form, m)
        assert [(e["qb"], e["qe"], e["tb"], e["te"]) for e in exp] == _lastrow["want"]
        assert any(e["qb"] == e["qe"] for e in exp)
        _forms_check(lib, monkeypatch, capfd, _lastrow["q"], _lastrow["t"], costs, 3, form, m)
    dm = a.dear_mismatch_mat(m)
    for tl, ends in ((1, 1), (3, 1), (3, 3)):
        e = _check(lib, [np.array([0, 0, 0], np.uint8)], [np.full(tl, 1, np.uint8)], dm, (4, 2), ends, m, msg="empty query")[0]
        assert (e["score"], e["qb"], e["tb"], e["te"], e["cigar"]) == (-6, e["qe"] + 1, 0, 0, [1 << 4 | 2])


# ---------------------------------------------------------------- 4. ties

@pytest.mark.parametrize("form", ["2", "0"])
def test_hand_built_ties(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    qs, ts, es, exp = a.tie_cases()
    mat = s.unit_mat(5)
    for q, t, e, x in zip(qs, ts, es, exp):
        assert tuple(_cells(a.call(lib, [q], [t], mat, (4, 2), e, 5))[0]) == x, (form, q, t, e)
        assert tuple(_cells(a.call(lib, [q], [t], mat, (4, 2, 4, 2), e, 5))[0]) == x, (form, q, t, e, "two-piece")
        _check(lib, [q], [t], mat, (4, 2), e, 5, msg="tie")


# ---------------------------------------------------------------- 5. packed halves that disagree

@pytest.mark.parametrize("order", [0, 1])
def test_packed_halves_that_disagree(lib, monkeypatch, capfd, order):
    """pairs of ONE shape in one packed task (asserted from the trace line): te differs, qe differs (one half ends in the last column, the
    other in the last row), one half has an empty interval, the last row's owning generation differs (te 1 000 against 1 030)"""
    rng = np.random.default_rng(31 + order)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "1")
    mat = s.unit_mat(5)

    def run(qs, ts, costs, ends, name):
        if order:
            qs, ts = qs[::-1], ts[::-1]
        capfd.readouterr()
        exp = _check(lib, qs, ts, mat, costs, ends, 5, msg=(name, order))
        assert _tasks(capfd.readouterr().err, costs, 2)[:2] == (1, 0)
        return exp[::-1] if order else exp

    for costs in ((4, 2), (4, 2, 24, 1)):
        qs, ts = sa.uneven_halves(rng, 5, 2100, 40, (45, 2090))
        assert [e["te"] for e in run(qs, ts, costs, 3, "te")] == [45, 2090]
        q1, t1 = s.planted(rng, 5, 300, 70, 200)
        q2, t2 = o.qend_pair(rng, 300, 70, 9)
        exp = run([q1, q2], [t1, t2], costs, 2, "qe")
        assert (exp[0]["qe"], exp[1]["qe"], exp[1]["te"]) == (69, 8, 299)
        q1 = rng.integers(2, 4, 1100, dtype=np.uint8)
        q2 = rng.integers(2, 4, 1100, dtype=np.uint8)
        t1 = np.concatenate([q1[60:1061], rng.integers(0, 2, 99, dtype=np.uint8)])          # te = 1 000, qb = 60
        t2 = np.concatenate([q2[30:1061], rng.integers(0, 2, 69, dtype=np.uint8)])          # te = 1 030, qb = 30
        exp = run([q1, q2], [t1, t2], costs, 3, "generation")
        assert [(e["qb"], e["tb"], e["te"]) for e in exp] == [(60, 0, 1000), (30, 0, 1030)]
    q1, t1 = sa.planted_copy(rng, 5, 2100, 1, 2090)
    q2, t2 = rng.integers(2, 4, 1, dtype=np.uint8), rng.integers(0, 2, 2100, dtype=np.uint8)
    exp = run([q1, q2], [t1, t2], (1, 1), 2, "empty")
    assert (exp[1]["score"], exp[1]["tb"], exp[1]["te"], exp[1]["cigar"]) == (-2, 1, 0, [1 << 4 | 1]) and exp[0]["tb"] == exp[0]["te"] == 2090


# ---------------------------------------------------------------- 6. beyond the packed range

def test_int32_form_beyond_the_packed_range(lib, monkeypatch, capfd):
    """a score above 65 535 and a query beyond the 16-bit column index take the int32 form in both passes, with the same results"""
    rng = np.random.default_rng(4)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    q = rng.integers(0, 4, 2000, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q[:1800]])
    capfd.readouterr()
    exp = _check(lib, [q], [t], u.simple_mat(4, 40, 30), (4, 2), 3, 4)
    assert _tasks(capfd.readouterr().err, (4, 2), 1)[:2] == (0, 1)
    assert exp[0]["score"] == 40 * 1800 > 65535 and (exp[0]["qb"], exp[0]["qe"], exp[0]["tb"], exp[0]["te"]) == (0, 1799, 30, 1829)
    zero = np.zeros(25, np.int8)                                             # no positive entry, free gaps: B = 0, every length is admitted
    q = rng.integers(0, 5, 65540, dtype=np.uint8)
    t = rng.integers(0, 5, 3, dtype=np.uint8)
    for ends, tasks in ((0, (1, 0)), (1, (0, 1)), (2, (0, 1))):
        capfd.readouterr()
        got = a.call(lib, [q], [t], zero, (0, 0), ends, 5, a.SCORE_ONLY)
        assert _tasks(capfd.readouterr().err, (0, 0), 1)[:2] == tasks
        np.testing.assert_array_equal(_cells(got), a.oracle_cells([q], [t], zero, (0, 0), ends, 5))


# ---------------------------------------------------------------- 7. negative optima, matrices without a positive entry, free gaps

@pytest.mark.parametrize("m", [5, 20])
def test_negative_optima_nonpositive_matrices_free_gaps(lib, monkeypatch, m):
    rng = np.random.default_rng(8 + m)
    qs, ts = u.ragged(rng, 40, m, 1, 150)
    ts = [np.concatenate([rng.integers(0, m, int(rng.integers(0, 1200)), dtype=np.uint8), x]) for x in ts]
    seen_empty = seen_neg = 0
    for mat, costs in ((u.random_mat(rng, m, -7, 1), (3, 1)), (u.random_mat(rng, m, -7, 1), (0, 0)), (s.unit_mat(m), (0, 0)),
                       (u.random_mat(rng, m, -3, 2), (0, 1, 3, 0)), (u.simple_mat(m, 1, 100), (120, 110))):
        for ends in o.ENDS:
            cells = a.oracle_cells(qs, ts, mat, costs, ends, m)
            exp = a.expected(qs, ts, mat, costs, ends, m, cells=cells)
            for form in ("2", "0"):
                monkeypatch.setenv("KSW2AMD_LL_FORM", form)
                a.assert_same(a.call(lib, qs, ts, mat, costs, ends, m), exp, str((costs, ends, form)))
            seen_empty += int(((cells[:, 3] > cells[:, 4]) | (cells[:, 1] > cells[:, 2])).sum())
            seen_neg += int((cells[:, 0] < 0).sum())
    assert seen_empty > 20 and seen_neg > 20


# ---------------------------------------------------------------- 8. corners and bad arguments

def test_corners_and_bad_arguments_launch_nothing(lib, capfd):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    mp = mat.ctypes.data_as(_i8p)
    e = np.zeros(0, np.uint8)
    q5 = np.array([0, 1, 2, 3, 0], np.uint8)
    ins = dict(score=-14, qb=0, qe=4, tb=0, te=-1, n_cigar=1, cigar=[5 << 4 | 1])
    hang = dict(score=0, qb=5, qe=4, tb=0, te=-1, n_cigar=0, cigar=[])
    F = lambda got: [{f: g[f] for f in a.FIELDS} for g in got]
    capfd.readouterr()
    for costs in ((4, 2), (4, 2, 24, 1)):
        for ends in range(4):
            want = [RESET, hang if ends & 1 else ins, RESET]
            assert F(a.call(lib, [e, q5, e], [q5, e, e], mat, costs, ends, 5)) == want
            assert F(a.call_flat(lib, lf.arena([e, q5, e], [q5, e, e], lead=2, gap=1), mat, costs, ends, 5)) == want
    err = capfd.readouterr().err
    assert "pk_tasks=0 int32_tasks=0" in err and not re.search(r"(pk|int32)_tasks=[1-9]", err)      # nothing to launch
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = lib.local_pairs(q, t)
    aln = (ka.LocalAln * 6)()
    L = lib.lib
    ar = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = lib._local_flat(*ar, None)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    bad_t = [x.copy() for x in t]
    bad_t[2][len(bad_t[2]) - 1] = 9
    one = np.zeros(1, np.int8)
    p1, k1 = lib.local_pairs([np.zeros(4, np.uint8)], [np.zeros(4, np.uint8)])
    stats = lib.host_stats()
    capfd.readouterr()
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, -1)):
        assert L.ksw2amd_ov_align_batch(None, *args, 3, 0, 6, pairs, aln) == -2, args
        assert L.ksw2amd_ov_align_batch_flat(None, *args, 3, 0, 6, ctypes.byref(f), aln) == -2, args
        assert L.ksw2amd_ovd_align_batch(None, *args, 24, 1, 3, 0, 6, pairs, aln) == -2, args
    for ends in (4, -1):
        assert L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, ends, 0, 6, pairs, aln) == -2
        assert L.ksw2amd_ovd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, ends, 0, 6, ctypes.byref(f), aln) == -2
    for flag in (0x04, 0x40, 0x100):
        assert L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, flag, 6, pairs, aln) == -2
        assert L.ksw2amd_ovd_align_batch(None, 5, mp, 4, 2, 24, 1, 3, flag, 6, pairs, aln) == -2
    assert L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, 0, 6, None, aln) == -2 and L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, 0, 6, pairs, None) == -2
    assert L.ksw2amd_ovd_align_batch(None, 1, one.ctypes.data_as(_i8p), 4, 2, 24, 1, 3, 0, 1, p1, aln) == -2 and "m >= 2" in lib.last_error()
    with pytest.raises(ka.Ksw2Error, match=r"pair 2: residue code >= m"):
        a.call(lib, q, bad_t, mat, (4, 2), 3, 5)
    pairs[1].qlen = (0x3fffffff - 127 - 127) // (127 + 127) + 1                # the range limit (only the length is looked at)
    assert L.ksw2amd_ov_align_batch(None, 5, big.ctypes.data_as(_i8p), 127, 127, 3, 0, 2, pairs, aln) == -2 and "0x3fffffff" in lib.last_error()
    pairs[1].qlen = len(q[1])
    before = lib.error_count()
    rec = ka.LocalAln()
    rec.score = 5
    assert L.ksw2amd_ov_align(None, None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, 3, 0, ctypes.byref(rec)) == 0
    assert (rec.score, rec.qb, rec.qe, rec.tb, rec.te, rec.n_cigar) == (0, -1, -1, -1, -1, 0) and lib.error_count() > before
    assert not re.search(r"\] ovd?a: pairs", capfd.readouterr().err) and lib.host_stats() == stats      # nothing was staged or launched


# ---------------------------------------------------------------- 9. flat arenas

@pytest.mark.parametrize("kind", ["host", "pinned", "device"])
def test_flat_arenas(lib, monkeypatch, capfd, kind):
    """a host arena, a page-locked arena and a device arena equal the pointer entry, chunked as well (the device arena brings back the span
    [qoff + qb, qoff + qe] and [toff + tb, toff + te]); a code >= m in a later chunk is caught on the device and resets EVERY entry"""
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    qs, ts = o.ragged_batch(rng, n=64, m=5, qmax=150, tmax=1400, long_targets=0)
    base, qo, ql, to, tl = ar = lf.arena(qs, ts, lead=1, gap=3, fill=255)    # 255 between the sequences: never looked at
    n = len(ts)
    for costs in ((4, 2), (24, 1, 4, 2)):
        exp = a.expected(qs, ts, mat, costs, 3, 5)
        assert sum(e["qb"] > 0 for e in exp) > 5
        with placed(lib, base, kind) as kw:
            capfd.readouterr()
            a.assert_same(a.call_flat(lib, ar, mat, costs, 3, 5, **kw), exp, kind)
            assert ("arena=device" if kind == "device" else "arena=host") in capfd.readouterr().err
            monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "20000")
            capfd.readouterr()
            a.assert_same(a.call_flat(lib, ar, mat, costs, 1, 5, flag=a.REV_CIGAR, **kw), a.expected(qs, ts, mat, costs, 1, 5, a.REV_CIGAR), kind)
            assert capfd.readouterr().err.count("%s: pairs=" % _tn(costs)) > 3
            monkeypatch.delenv("KSW2AMD_LL_CHUNK_BYTES")
    monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "20000")
    bad = base.copy()
    bad[int(to[40]) + 2] = 5
    with placed(lib, bad, kind) as kw:
        aln = (ka.LocalAln * n)()
        with pytest.raises(ka.Ksw2Error, match=r"pair 40: residue code >= m"):
            a.call_flat(lib, (bad,) + tuple(ar[1:]), mat, (4, 2), 3, 5, aln=aln, **kw)
        assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)      # the earlier chunks' as well


# ---------------------------------------------------------------- 10. flags, buffers, the single-pair entries, the C caller

def test_flags_and_cigar_buffers(lib):
    rng = np.random.default_rng(6)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=18, m=5, qmax=90, tmax=200, long_targets=0)
    q.append(np.array([0, 0, 1, 1], np.uint8)); t.append(np.array([0, 0, 0, 1, 1], np.uint8))
    for costs in ((4, 2), (4, 2, 24, 1)):
        cig = {fl: [e["cigar"] for e in _check(lib, q, t, mat, costs, 3, 5, flag=fl, msg=fl)] for fl in (0, a.RIGHT, a.REV_CIGAR, a.RIGHT | a.REV_CIGAR)}
        assert cig[0] != cig[a.RIGHT] and cig[a.REV_CIGAR] == [c[::-1] for c in cig[0]]
    exp = a.expected(q, t, mat, (4, 2), 3, 5)
    aln = (ka.LocalAln * len(q))()
    a.assert_same(a.call(lib, q, t, mat, (4, 2), 3, 5, aln=aln), exp)
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    a.assert_same(a.call(lib, q, t, mat, (4, 2), 3, 5, aln=aln), exp)
    assert [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    got = a.call(lib, q, t, mat, (4, 2), 3, 5, a.SCORE_ONLY, aln=aln)
    assert all(g["n_cigar"] == 0 for g in got) and [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    np.testing.assert_array_equal(_cells(got), _cells(exp))
    for x in aln:
        ka._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


@pytest.mark.parametrize("mode", ["", "dual"])
def test_single_pair_and_c_caller(lib, tmp_path, mode):
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=12, m=5, qmax=80, tmax=1300, long_targets=0)
    q += [np.zeros(0, np.uint8), q[0]]
    t += [t[0], np.zeros(0, np.uint8)]
    costs = (4, 2, 24, 1) if mode else (4, 2)
    exe = str(tmp_path / "ova_caller")
    libdir = os.path.dirname(os.path.abspath(lib.path))
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "ova_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    for ends, flag in ((3, 0), (1, a.RIGHT | a.REV_CIGAR)):
        exp = a.expected(q, t, mat, costs, ends, 5, flag)
        got = [lib.ov_align(q[i], t[i], mat, costs[0], costs[1], ends, flag=flag, costs2=costs[2:] if mode else None) for i in range(len(q))]
        a.assert_same(got, exp, "single")
        inp = str(tmp_path / "pairs.txt")
        a.write_input(inp, q, t, mat, 5, costs, ends, flag)
        out = subprocess.run([exe, inp] + ([mode] if mode else []), check=True, capture_output=True, text=True).stdout
        batch, single, _ = la.parse_caller(out)
        a.assert_same(batch, exp, "batch")
        a.assert_same(single, exp, "single")


# ---------------------------------------------------------------- 11. identities

def test_identities(lib):
    """ends == 0 is the semi-global align entry in every field; equal or dominated second pieces are the single-piece entry"""
    rng = np.random.default_rng(12)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=200, m=5, qmax=120, tmax=1300, long_targets=2)
    F = lambda got: [{f: g[f] for f in a.FIELDS} for g in got]
    assert F(a.call(lib, q, t, mat, (4, 2), 0, 5)) == F(lib.sg_align_batch(q, t, mat, 4, 2, m=5))
    assert F(a.call(lib, q, t, mat, (4, 2, 24, 1), 0, 5)) == F(lib.sgd_align_batch(q, t, mat, 4, 2, 24, 1, m=5))
    for ends in o.ENDS:
        one = F(a.call(lib, q, t, mat, (4, 2), ends, 5))
        assert F(a.call(lib, q, t, mat, (4, 2, 4, 2), ends, 5)) == one and F(a.call(lib, q, t, mat, (4, 2, 9, 3), ends, 5)) == one


# ---------------------------------------------------------------- 12. a ragged batch

_ragged = {}


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("form,m", [("2", 5), ("0", 20)])
def test_ragged_batch(lib, monkeypatch, capfd, costs, form, m):
    """tests/ov_util.ragged_batch at a reduced n (queries to 200, targets to 1 500 and six of 4 000 - 5 000: five generations), every ends;
    score, qe, te are ksw2amd_ov_batch's bit for bit; the CIGARs of every eighth pair against the scalar contract"""
    if m not in _ragged:
        rng = np.random.default_rng(2000 + m)
        qs, ts = o.ragged_batch(rng, n=600, m=m, long_targets=6)
        _ragged[m] = (qs, ts, u.simple_mat(5, 2, 4, -1) if m == 5 else u.random_mat(rng, 20, -5, 4))
    qs, ts, mat = _ragged[m]
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    sub = list(range(0, len(qs), 8))
    for ends in o.ENDS:
        cells = a.oracle_cells(qs, ts, mat, costs, ends, m)
        capfd.readouterr()
        got = a.call(lib, qs, ts, mat, costs, ends, m)
        pk, i32, prof = _tasks(capfd.readouterr().err, costs, len(qs))
        np.testing.assert_array_equal(_cells(got), cells, str((m, costs, ends)))
        np.testing.assert_array_equal(cells[:, [0, 2, 4]], o.call(lib, qs, ts, mat, costs, ends, m))
        assert prof == ("registers" if m == 5 else "lds") and ((pk >= 300 and i32 == 0) if form == "2" else pk == 0)
        exp = a.expected([qs[i] for i in sub], [ts[i] for i in sub], mat, costs, ends, m, cells=cells[sub])
        a.assert_same([got[i] for i in sub], exp, str((m, costs, ends)))


# ---------------------------------------------------------------- 13. the golden file

@pytest.mark.parametrize("form", ["1", "0"])
def test_golden_file(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    total = 0
    for name, m, mat, c2, c4, q, t, per in a.load_golden():
        for (kind, e), (cells, cig) in per.items():
            costs = c2 if kind == "ov" else c4
            for fl in a.GOLDEN_FLAGS:
                got = a.call(lib, q, t, mat, costs, e, m, fl)
                np.testing.assert_array_equal(_cells(got), cells, str((name, kind, e)))
                assert [g["cigar"] for g in got] == cig[fl], (name, kind, e, fl)
        total += len(q)
    assert total == 324
