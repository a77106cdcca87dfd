"""GPU: overlap alignment (ksw2amd_ov_batch / ksw2amd_ovd_batch, their flat forms and the single-pair entries) on libksw2_amd.so against the
contract (tests/ov_oracle.c), bit for bit, and against tests/golden/ov_cases.npz, which the compiled reference produced.  The shapes are the
smallest at which k2a_ov_kernel and k2a_ovd_kernel can go wrong: the last target row in strip registers 0, 7, 14, 15, in lanes 0, 1, 63 and in
generations 0, 1, 2, its best column around the 4-step prefetch and the 63-step skew, the hanging query prefix on either side of a lane (16
rows) and of a generation (1 024 rows), ties between the last column and the last row, packed halves that end on different edges, the packed
admission limits (16-bit values, 16-bit column), both gap costs."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_util as u
from tests import llf_util as lf
from tests import ov_util as o
from tests import sg_util as s
from tests import sgd_util as d

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
CROSS = d.CROSS
NAME = {2: "ov", 4: "ovd"}


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


def _check(lib, q, t, mat, costs, ends, m, exp=None, msg="", flat=False):
    exp = o.oracle_batch(q, t, mat, costs, ends, m) if exp is None else exp
    np.testing.assert_array_equal(o.call(lib, q, t, mat, costs, ends, m), exp, str((msg, costs, ends)))
    if flat:
        np.testing.assert_array_equal(o.call_flat(lib, lf.arena(q, t, lead=3, gap=2), mat, costs, ends, m), exp, str((msg, costs, ends, "flat")))
    return exp


def _split(capfd, costs, form, n=None):
    """the trace lines of the entry since the last read: packed under form 2, int32 under form 0"""
    err = capfd.readouterr().err
    tasks = o.pk_tasks(err, NAME[len(costs)])
    assert tasks, err
    for pk, i32 in tasks:
        assert (pk == 0 and i32 > 0) if form == "0" else (pk > 0 and i32 == 0), err
    assert "pk_profile=lds" not in err                                      # every packed form has its register profile
    return tasks


# ---------------------------------------------------------------- 1. the last row: where its maximum changes hands

_grid = {}


def _qend_grid(m):
    if "q" not in _grid:
        qs, ts, what = o.qend_grid(np.random.default_rng(78))
        _grid.update(q=qs, t=ts, what=what)
    if m not in _grid:
        _grid[m] = {(c, e): o.oracle_batch(_grid["q"], _grid["t"], s.unit_mat(m), c, e, m) for c in ((4, 2), CROSS) for e in (2, 3)}
    return _grid


@pytest.mark.parametrize("form,m", [("2", 5), ("0", 5), ("2", 20), ("0", 20)])
def test_edge_grid_query_end(lib, monkeypatch, capfd, form, m):
    """tlen {1, 2, 8, 15, 16, 17, 31, 32, 1 023, 1 024, 1 025, 1 040, 2 047, 2 049} x qlen {1, 2, 5, 63, 64, 65, 130}, the query's first p
    residues planted as the target's last p, p - 1 in {0 .. 4, 62, 63, 64, qlen - 2, qlen - 1}; registers (m = 5) and LDS (m = 20), packed and
    int32, both gap costs, the pointer and the flat entry"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    g = _qend_grid(m)
    mat = s.unit_mat(m)
    for costs in ((4, 2), CROSS):
        for e in (2, 3):
            capfd.readouterr()
            _check(lib, g["q"], g["t"], mat, costs, e, m, exp=g[m][(costs, e)], msg=(form, m), flat=e == 3)
            _split(capfd, costs, form)
    seen = set()
    for (tl, ql, p), r in zip(g["what"], g[m][((4, 2), 3)]):
        if p <= tl and tuple(r) == (2 * p, p - 1, tl - 1):
            seen.add(((tl - 1) % 16, ((tl - 1) % 1024) // 16, (tl - 1) // 1024, p - 1))
    assert {c for c, _, _, _ in seen} >= {0, 7, 14, 15} and {l for _, l, _, _ in seen} >= {0, 1, 63} and {x for _, _, x, _ in seen} == {0, 1, 2}
    assert {x for _, _, _, x in seen} >= {0, 1, 2, 3, 4, 62, 63, 64, 128, 129}


# ---------------------------------------------------------------- 2. the free first row

@pytest.mark.parametrize("form,m", [("2", 5), ("0", 5), ("2", 20), ("0", 20)])
def test_edge_grid_query_start(lib, monkeypatch, form, m):
    """the query's last s residues are the target's first s, s - 1 on both sides of rows 15 / 16 and 1 023 / 1 024: the best cell is
    (s - 1, qlen - 1) and the hanging prefix costs nothing; a whole copy in the middle of the target keeps its score"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    qs, ts, what = o.qbeg_grid(np.random.default_rng(79))
    mat = s.unit_mat(m)
    for costs in ((4, 2), CROSS):
        e1 = _check(lib, qs, ts, mat, costs, 1, m, msg=(form, m), flat=True)
        e0 = _check(lib, qs, ts, mat, costs, 0, m, msg=(form, m))
        _check(lib, qs, ts, mat, costs, 3, m, msg=(form, m))
        for (tl, ql, x), r1, r0 in zip(what, e1, e0):
            if x > 0:
                assert tuple(r1) == (2 * x, ql - 1, x - 1) and (x == ql or r0[0] < r1[0]), (tl, ql, x, r1, r0)
            else:
                assert tuple(r1) == tuple(r0) == (2 * ql, ql - 1, -x)
    assert {x - 1 for _, _, x in what if x > 0} >= {14, 15, 16, 1022, 1023, 1024}


# ---------------------------------------------------------------- 3. both bits, 4. ties

@pytest.mark.parametrize("form", ["2", "0"])
def test_both_ends(lib, monkeypatch, form):
    """a suffix-prefix overlap in both orientations, a contained query, a contained target, under ends 0, 1, 2, 3"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = s.unit_mat(5)
    qs, ts, kinds = o.both_pairs(np.random.default_rng(80))
    res = {e: _check(lib, qs, ts, mat, (4, 2), e, 5, msg=kinds, flat=True) for e in range(4)}
    for e in range(4):
        _check(lib, qs, ts, mat, CROSS, e, 5, msg=kinds, flat=True)
    assert tuple(res[1][0]) == (50, 59, 24) and res[0][0][0] < 50
    assert tuple(res[2][1]) == (50, 24, 59) and res[0][1][0] < 50
    assert all(tuple(res[e][2]) == (60, 29, 739) for e in range(4))
    assert tuple(res[3][3]) == (90, 69, 44) and all(res[e][3][0] < 90 for e in range(3))


@pytest.mark.parametrize("form", ["2", "0"])
def test_ties(lib, monkeypatch, form):
    """last column against last row -> the last column; two maxima in the last row -> the smaller column; the corner against a smaller
    column -> the smaller column; two equal last-column rows across a lane and a generation boundary -> the smaller row"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = s.unit_mat(5)
    qs, ts, es, exp = o.tie_cases()
    for q, t, e, x in zip(qs, ts, es, exp):
        want = np.array([x, x], np.int32)
        _check(lib, [q, q], [t, t], mat, (4, 2), e, 5, exp=want)
        _check(lib, [q, q], [t, t], mat, CROSS, e, 5, exp=want)
        np.testing.assert_array_equal(o.oracle_batch([q], [t], mat, (4, 2), e, 5), want[:1])
    qs, ts, tes = s.tie_pairs()
    for e in o.ENDS:
        for costs in ((4, 2), CROSS):
            got = _check(lib, qs, ts, mat, costs, e, 5)
            assert [int(v) for v in got[:, 2]] == tes and (got[:, 0] == 12).all() and (got[:, 1] == 5).all()


# ---------------------------------------------------------------- 5. packed and int32

def test_admission_bound(lib, monkeypatch, capfd):
    """smax = 127, costs (5, 1): B + (qlen + 1) * smax <= 65 535 up to qlen 510"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    for ql, packed in ((510, True), (511, False)):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q[:ql - 7]])
        for costs in ((5, 1), (5, 1, 9, 1)):
            capfd.readouterr()
            got = _check(lib, [q], [t], mat, costs, 3, 4)
            err = capfd.readouterr().err
            assert tuple(got[0]) == (127 * (ql - 7), ql - 8, len(t) - 1)
            assert o.pk_tasks(err, NAME[len(costs)]) == [(1, 0) if packed else (0, 1)], err
            assert " ends=3" in err


def test_16_bit_column_condition(lib, monkeypatch, capfd):
    """qlen = 65 537, tlen = 20, a matrix without a positive entry, gape = 0: the values fit the packed form, the best cell's column 65 536
    does not, so the pair runs as int32; one residue fewer is packed"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    t = np.array([0] + [1] * 19, np.uint8)
    q = np.concatenate([np.full(65537 - 20, 2, np.uint8), t])
    mat = u.simple_mat(4, 0, 3)
    for costs in ((3, 0), (3, 0, 9, 0)):
        capfd.readouterr()
        exp = _check(lib, [q], [t], mat, costs, 3, 4)
        assert tuple(exp[0]) == (0, 65536, 19)
        assert o.pk_tasks(capfd.readouterr().err, NAME[len(costs)]) == [(0, 1)]
        exp = _check(lib, [q[1:]], [t], mat, costs, 3, 4)
        assert tuple(exp[0]) == (0, 65535, 19)
        assert o.pk_tasks(capfd.readouterr().err, NAME[len(costs)]) == [(1, 0)]
        _check(lib, [q], [t], mat, costs, 1, 4)
        assert o.pk_tasks(capfd.readouterr().err, NAME[len(costs)]) == [(1, 0)]


def test_score_above_16_bits(lib, monkeypatch):
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    rng = np.random.default_rng(4)
    q = rng.integers(0, 4, 1700, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q[:1650]])
    for costs in ((4, 2), CROSS):
        exp = _check(lib, [q], [t], u.simple_mat(4, 40, 30), costs, 2, 4, flat=True)
        assert tuple(exp[0]) == (40 * 1650, 1649, len(t) - 1) and exp[0, 0] > 65535


@pytest.mark.parametrize("m", [5, 20])
def test_packed_halves_on_different_edges(lib, monkeypatch, capfd, m):
    """two pairs of one shape in one packed task: one ends in the last column in the middle of the target, the other in the last row"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", "1")
    rng = np.random.default_rng(6)
    qa, ta = s.planted(rng, 5, 1040, 64, 500)
    qb, tb = o.qend_pair(rng, 1040, 64, 40)
    for costs in ((4, 2), CROSS):
        capfd.readouterr()
        exp = _check(lib, [qa, qb, qb, qa], [ta, tb, tb, ta], s.unit_mat(m), costs, 3, m)
        assert o.pk_tasks(capfd.readouterr().err, NAME[len(costs)]) == [(2, 0)]
        assert tuple(exp[0]) == (128, 63, 500) and tuple(exp[1]) == (80, 39, 1039)


# ---------------------------------------------------------------- 6. scores and corners

@pytest.mark.parametrize("form", ["2", "0"])
def test_negative_optima_nonpositive_matrices_free_gaps(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    rng = np.random.default_rng(14)
    q, t = np.zeros(40, np.uint8), np.ones(300, np.uint8)
    for costs in ((20, 3), (2, 1), (20, 3, 30, 1)):
        for e in range(4):
            assert _check(lib, [q, q], [t, t], u.simple_mat(4, 1, 100), costs, e, 4)[0, 0] < 0      # a real cell, never the boundary
    qs, ts = o.ragged_batch(rng, n=60, m=5, qmax=90, tmax=1200, long_targets=0)
    for mat in (u.random_mat(rng, 5, -7, 1), u.random_mat(rng, 5, -9, 0)):
        assert mat.max() <= 0
        for costs in ((3, 1), (0, 0), (3, 1, 9, 0)):
            for e in o.ENDS:
                assert (_check(lib, qs, ts, mat, costs, e, 5)[:, 0] <= 0).all()
    for e in o.ENDS:
        _check(lib, qs, ts, u.simple_mat(5, 2, 4, -1), (0, 0), e, 5, flat=True)
        _check(lib, qs, ts, u.simple_mat(5, 2, 4, -1), (0, 0, 0, 0), e, 5)


def test_corners_and_bad_arguments_launch_nothing(lib, capfd):
    e = np.zeros(0, np.uint8)
    q = np.array([0, 1, 2, 3, 0], np.uint8)
    mat = u.simple_mat(5, 2, 4, -1)
    for costs in ((4, 2), (4, 2, 1, 3)):
        ins = -o.gap_cost(costs, 5)
        for ends in range(4):
            capfd.readouterr()
            exp = np.array([[0, -1, -1], [0 if ends & 1 else ins, 4, -1], [0, -1, -1]], np.int32)
            np.testing.assert_array_equal(o.call(lib, [e, q, e], [q, e, e], mat, costs, ends, 5), exp)
            np.testing.assert_array_equal(o.call_flat(lib, lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, costs, ends, 5), exp)
            assert all(x == (0, 0) for x in o.pk_tasks(capfd.readouterr().err, NAME[len(costs)]))
            np.testing.assert_array_equal(o.call(lib, [q, e, q], [e, q, q], mat, costs, ends, 5), [[0 if ends & 1 else ins, 4, -1], [0, -1, -1], [10, 4, 4]])
    rng = np.random.default_rng(9)
    qs, ts = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = lib.local_pairs(qs, ts)
    res = (ka.LocalResult * 6)()
    a = lf.arena(qs, ts, lead=1, gap=2)
    f, n, keep2 = lib._local_flat(*a, None)
    mp = mat.ctypes.data_as(_i8p)
    E = ka.KSW2AMD_E_PARAM if hasattr(ka, "KSW2AMD_E_PARAM") else -2
    capfd.readouterr()
    for ends in (4, 7, -1):
        assert lib.lib.ksw2amd_ov_batch(5, mp, 4, 2, ends, 6, pairs, res) == E and "ends" in lib.last_error()
        assert lib.lib.ksw2amd_ov_batch_flat(5, mp, 4, 2, ends, 6, ctypes.byref(f), res) == E
        assert lib.lib.ksw2amd_ovd_batch(5, mp, 4, 2, 24, 1, ends, 6, pairs, res) == E
        assert lib.lib.ksw2amd_ovd_batch_flat(5, mp, 4, 2, 24, 1, ends, 6, ctypes.byref(f), res) == E
    for args in ((0, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, -1)):
        assert lib.lib.ksw2amd_ov_batch(*args, 3, 6, pairs, res) == E and lib.lib.ksw2amd_ovd_batch(*args, 24, 1, 3, 6, pairs, res) == E
    assert lib.lib.ksw2amd_ovd_batch(5, mp, 4, 2, 128, 1, 3, 6, pairs, res) == E
    assert "pairs=" not in capfd.readouterr().err                          # no chunk was staged


# ---------------------------------------------------------------- 7. flat entries

@pytest.mark.parametrize("kind", ["host", "pinned", "device"])
def test_flat_arenas_chunked_with_the_device_check(lib, monkeypatch, capfd, kind):
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=60, m=5, qmax=100, tmax=400, long_targets=0)
    t[5] = np.concatenate([rng.integers(0, 5, 1100, dtype=np.uint8), q[5][:len(q[5]) // 2 + 1]])
    q[7], t[9] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    a = lf.arena(q, t, lead=3, gap=2)
    for costs in ((4, 2), CROSS):
        exp = o.oracle_batch(q, t, mat, costs, 3, 5)
        with placed(lib, a[0], kind) as kw:
            np.testing.assert_array_equal(o.call_flat(lib, a, mat, costs, 3, 5, **kw), exp)
            monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "6000")
            capfd.readouterr()
            np.testing.assert_array_equal(o.call_flat(lib, a, mat, costs, 3, 5, **kw), exp)
            assert len(o.pk_tasks(capfd.readouterr().err, NAME[len(costs)])) > 3
        bad = a[0].copy()
        bad[int(a[3][41])] = 6
        out = np.full((60, 3), 7, np.int32)
        with placed(lib, bad, kind) as kw:
            with pytest.raises(ka.Ksw2Error, match=r"pair 41: residue code >= m"):
                o.call_flat(lib, (bad,) + tuple(a[1:]), mat, costs, 3, 5, out=out, **kw)
        k = int(np.nonzero((out != exp).any(1))[0][0])
        assert 0 < k <= 41 and (out[:k] == exp[:k]).all() and (out[k:] == np.array([0, -1, -1])).all()
        monkeypatch.delenv("KSW2AMD_LL_CHUNK_BYTES")


# ---------------------------------------------------------------- 8. entry points

def test_single_pair_entries(lib):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=6, m=5, qmax=60, tmax=1100, long_targets=0)
    for ends in range(4):
        exp = o.oracle_batch(q, t, mat, (4, 2), ends, 5)
        expd = o.oracle_batch(q, t, mat, CROSS, ends, 5)
        for k in range(len(q)):
            assert lib.ov(q[k], t[k], mat, 4, 2, ends) == tuple(exp[k])
            assert lib.ovd(q[k], t[k], mat, *CROSS, ends) == tuple(expd[k])
    assert lib.ov(q[0], t[0], mat, 4, 2, 4) == (0, -1, -1) and "ends" in lib.last_error()


@pytest.mark.parametrize("pool", [False, True])
def test_c_caller(tmp_path, pool):
    exe = str(tmp_path / "ov_caller")
    libdir = os.path.dirname(ka.DEFAULT_SO)
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "ov_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=12, m=5, qmax=80, tmax=300, long_targets=0)
    q.append(np.zeros(0, np.uint8)); t.append(t[0])
    q.append(q[0]); t.append(np.zeros(0, np.uint8))
    inp = str(tmp_path / "pairs.txt")
    o.write_input(inp, q, t, mat, 5, CROSS)
    env = dict(os.environ)
    env.pop("KSW2AMD_TRACE", None)
    out = subprocess.run([exe, inp] + (["pool"] if pool else []), check=True, capture_output=True, text=True, env=env).stdout.strip().splitlines()
    if pool:
        assert out[-1] == "pool %d" % (8 * len(q))
        out = out[:-1]
    k = 0
    for costs in (CROSS[:2], CROSS):
        if len(costs) == 4:
            assert out[k] == "two-piece"
            k += 1
        for ends in range(4):
            assert out[k] == "ends %d" % ends
            got = np.array([list(map(int, l.split())) for l in out[k + 1:k + 1 + len(q)]], dtype=np.int32)
            np.testing.assert_array_equal(got, o.oracle_batch(q, t, mat, costs, ends, 5), str((costs, ends)))
            k += 1 + len(q)
    assert k == len(out)


# ---------------------------------------------------------------- 9. identities

@pytest.mark.parametrize("form", ["1", "0"])
def test_identities(lib, monkeypatch, form):
    """ends == 0 is the semi-global entry bit for bit; equal or dominated second pieces give the single-piece result"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    rng = np.random.default_rng(12)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=300, m=5, qmax=150, tmax=1300, long_targets=2)
    np.testing.assert_array_equal(lib.ov_batch(q, t, mat, 4, 2, 0, m=5), lib.sg_batch(q, t, mat, 4, 2, m=5))
    np.testing.assert_array_equal(lib.ovd_batch(q, t, mat, 4, 2, 24, 1, 0, m=5), lib.sgd_batch(q, t, mat, 4, 2, 24, 1, m=5))
    ar = lf.arena(q, t, lead=1, gap=1)
    np.testing.assert_array_equal(lib.ov_batch_flat(*ar, mat, 4, 2, 0, m=5), lib.sg_batch_flat(*ar, mat, 4, 2, m=5))
    np.testing.assert_array_equal(lib.ovd_batch_flat(*ar, mat, 4, 2, 24, 1, 0, m=5), lib.sgd_batch_flat(*ar, mat, 4, 2, 24, 1, m=5))
    for e in range(4):
        one = lib.ov_batch(q, t, mat, 4, 2, e, m=5)
        for c2 in ((4, 2), (5, 2), (4, 3), (127, 127)):
            np.testing.assert_array_equal(lib.ovd_batch(q, t, mat, 4, 2, c2[0], c2[1], e, m=5), one, str((e, c2)))


# ---------------------------------------------------------------- 10. ragged batch

_ragged = {}


def _m20():
    mat = u.random_mat(np.random.default_rng(8), 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 3)
    return mat.reshape(-1)


@pytest.mark.parametrize("ends", o.ENDS)
@pytest.mark.parametrize("costs", [(4, 2), (0, 1), (0, 0), (4, 2, 24, 1), (24, 1, 4, 2)])
@pytest.mark.parametrize("m", [5, 20])
def test_ragged_batch(lib, m, costs, ends):
    """about 4 000 pairs, queries 1 - 200 x targets 1 - 1 500 plus 40 targets of 4 000 - 5 000, a third with a mutated query prefix at the
    target's tail or a suffix at its head; registers (m = 5) and LDS (m = 20)"""
    if m not in _ragged:
        _ragged[m] = o.ragged_batch(np.random.default_rng(100 + m), n=4000, m=m)
    q, t = _ragged[m]
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else _m20()
    exp = _check(lib, q, t, mat, costs, ends, m)
    nq = np.array([len(x) - 1 for x in q])
    if ends & 2 and costs[:2] == (4, 2):
        assert ((exp[:, 1] < nq) & (exp[:, 1] >= 0)).sum() > 100            # best cells in the last row off the corner


# ---------------------------------------------------------------- 11. the golden file

@pytest.mark.parametrize("form", ["2", "0"])
def test_golden_file(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    total = 0
    for name, m, mat, c2, c4, q, t, exp, expd in o.load_golden():
        for e in o.ENDS:
            _check(lib, q, t, mat, c2, e, m, exp=exp[e], msg=name, flat=e == 3)
            _check(lib, q, t, mat, c4, e, m, exp=expd[e], msg=name, flat=e == 3)
        total += len(q)
    assert total == 324
