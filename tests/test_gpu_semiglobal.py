"""GPU: semi-global alignment (ksw2amd_sg_batch / ksw2amd_sg_batch_flat / ksw2amd_sg) on libksw2_amd.so against the contract's formula
(tests/sg_oracle.c), bit for bit, and against tests/golden/sg_cases.npz, which the compiled reference produced.  The shapes are the
smallest at which the biased strip schedule can go wrong: the strip (16 rows), the generation (1 024 rows, the boundary in HBM), the
4-step prefetch and the 63-step skew of the columns, the best row on either side of a lane and of a generation boundary, ties across
them, the packed admission limit, scores beyond 16 bits, negative scores, matrices without a positive entry."""
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
from tests import sg_util as s

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (6, 1), (0, 0))


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
    line = re.search(r"sg: pairs=(\d+) pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
    assert line, err
    assert n is None or int(line.group(1)) == n, err
    return int(line.group(2)), int(line.group(3)), line.group(4)


# ---------------------------------------------------------------- ragged batches

_ragged = {}


def _ragged_pairs(m):
    """4 000 pairs of q 1-200 x t 1-1 500, a third with a mutated copy of the query in the target, and 40 pairs with targets up to 5 000
    (five generations, the boundary in HBM); made once per m"""
    if m not in _ragged:
        rng = np.random.default_rng(1000 + m)
        qs, ts = [], []
        for k in range(4040):
            big = k >= 4000
            q = rng.integers(0, m, int(rng.integers(1, 201)), dtype=np.uint8)
            t = rng.integers(0, m, int(rng.integers(4000, 5001)) if big else int(rng.integers(1, 1501)), dtype=np.uint8)
            if k % 3 == 0 and len(t) > len(q):
                c = q.copy()
                c[rng.random(len(c)) < 0.05] = int(rng.integers(0, m))
                at = int(rng.integers(0, len(t) - len(c) + 1))
                t[at:at + len(c)] = c
            qs.append(q); ts.append(t)
        mat = u.simple_mat(5, 2, 4, -1) if m == 5 else _m20(rng)
        _ragged[m] = (qs, ts, mat, {})
    return _ragged[m]


@pytest.mark.parametrize("m", [5, 20])
@pytest.mark.parametrize("costs", COSTS)
def test_ragged_batch(lib, monkeypatch, capfd, m, costs):
    qs, ts, mat, _ = _ragged_pairs(m)
    if costs[1] != 1:                                                        # (4, 2) and (0, 0): packed for every admissible pair
        monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    exp = s.oracle_batch(qs, ts, mat, *costs, m)
    capfd.readouterr()
    got = lib.sg_batch(qs, ts, mat, *costs, m=m)
    pk, i32, prof = _tasks(capfd.readouterr().err, len(qs))
    np.testing.assert_array_equal(got, exp, str((m, costs)))
    assert prof == ("registers" if m == 5 else "lds") and pk + i32 > 0 and (costs[1] == 1 or (pk > 2000 and i32 == 0))
    assert (exp[:, 1] == np.array([len(x) - 1 for x in qs])).all()


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
        _forms.update(q=qs, t=ts, mat=mat, exp=s.oracle_batch(qs, ts, mat, 4, 2, 5))
    return _forms


@pytest.mark.parametrize("form", ["0", "1", "2"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_forced_forms(lib, monkeypatch, capfd, form, lds):
    """512 same-shape pairs of 100 x 1 024 plus six of 300 x 2 500 under every KSW2AMD_LL_FORM x KSW2AMD_LL_LDS"""
    c = _form_case()
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
    capfd.readouterr()
    got = lib.sg_batch(c["q"], c["t"], c["mat"], 4, 2, m=5)
    pk, i32, prof = _tasks(capfd.readouterr().err, 518)
    np.testing.assert_array_equal(got, c["exp"], str((form, lds)))
    assert (pk, i32) == ((0, 518) if form == "0" else (259, 0)) and prof == ("lds" if lds == "1" else "registers")


# ---------------------------------------------------------------- where the schedule changes hands

@pytest.mark.parametrize("form,m", [("2", 5), ("0", 5), ("2", 20), ("0", 20)])
def test_edge_grid(lib, monkeypatch, capfd, form, m):
    """tlen {1, 15, 16, 17, 1 023, 1 024, 1 025, 2 049} x qlen {1, 2, 3, 4, 5, 63, 64, 65}, the query planted so that the best row is the last
    of a lane, the first of the next, the last of generation 0, the first of generation 1, the last of the target"""
    rng = np.random.default_rng(77)
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = s.unit_mat(m)
    tlens, qlens = (1, 15, 16, 17, 1023, 1024, 1025, 2049), (1, 2, 3, 4, 5, 63, 64, 65)
    qs, ts = s.edge_grid(rng, m, tlens, qlens)
    exp = s.oracle_batch(qs, ts, mat, 4, 2, m)
    capfd.readouterr()
    got = lib.sg_batch(qs, ts, mat, 4, 2, m=m)
    pk, i32, _ = _tasks(capfd.readouterr().err, len(qs))
    np.testing.assert_array_equal(got, exp, str((form, m)))
    np.testing.assert_array_equal(lib.sg_batch_flat(*lf.arena(qs, ts, lead=3, gap=2), mat, 4, 2, m=m), exp, str((form, m, "flat")))
    assert (pk == 0) if form == "0" else (pk > 0 and i32 == 0)
    k, seen = 0, set()
    for tl in tlens:
        for ql in qlens:
            for r in s.edge_rows(tl):
                if ql <= r + 1:                                             # the whole copy fits in front of row r
                    assert tuple(exp[k]) == (2 * ql, ql - 1, r), (tl, ql, r, exp[k])
                    seen.add(r)
                k += 1
    assert {15, 16, 1023, 1024, 2048} <= seen


@pytest.mark.parametrize("form", ["2", "0"])
def test_ties_take_the_smallest_te(lib, monkeypatch, capfd, form):
    """the best score in two rows on either side of a lane boundary and of a generation boundary"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    qs, ts, tes = s.tie_pairs()
    exp = s.oracle_batch(qs, ts, s.unit_mat(5), 4, 2, 5)
    assert [int(x) for x in exp[:, 2]] == tes and (exp[:, 0] == 12).all()
    capfd.readouterr()
    got = lib.sg_batch(qs, ts, s.unit_mat(5), 4, 2, m=5)
    pk, i32, _ = _tasks(capfd.readouterr().err, len(qs))
    np.testing.assert_array_equal(got, exp)
    assert (pk == 0) if form == "0" else (i32 == 0)


def test_repeats(lib):
    """a unit repeated three times as the query in a target of the unit repeated two hundred times: every period ties, the first wins"""
    unit = np.array([0, 1, 2, 3, 1, 0, 2], np.uint8)
    q, t = np.tile(unit, 3), np.tile(unit, 200)
    for form_q, form_t in (([q], [t]), ([q, q], [t, t])):                  # int32 (no partner), packed
        got = lib.sg_batch(form_q, form_t, u.simple_mat(5, 2, 4, -1), 4, 2, m=5)
        assert all(tuple(r) == (42, 20, 20) for r in got), got
    np.testing.assert_array_equal(lib.sg_batch([q], [t], u.simple_mat(5, 2, 4, -1), 4, 2, m=5), s.oracle_batch([q], [t], u.simple_mat(5, 2, 4, -1), 4, 2, 5))


# ---------------------------------------------------------------- the range of the two number formats

def test_packed_admission_limit(lib, monkeypatch, capfd):
    """smax = 127, costs (5, 1): B + (qlen + 1) * smax = 128 qlen + 132 <= 65 535 up to qlen 510 -- 510 is packed, 511 goes to int32"""
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    for ql, tasks in ((510, (1, 0)), (511, (0, 1))):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q, rng.integers(0, 4, 9, dtype=np.uint8)])
        exp = s.oracle_batch([q], [t], mat, 5, 1, 4)
        assert tuple(exp[0]) == (127 * ql, ql - 1, 20 + ql - 1)
        capfd.readouterr()
        got = lib.sg_batch([q], [t], mat, 5, 1, m=4)
        assert _tasks(capfd.readouterr().err, 1)[:2] == tasks
        np.testing.assert_array_equal(got, exp)


def test_beyond_16_bits_negative_scores_and_all_insert(lib, monkeypatch, capfd):
    rng = np.random.default_rng(4)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    # 2 000 x 3 000 with match 40: a score above 65 535, in int32
    q = rng.integers(0, 4, 2000, dtype=np.uint8)
    t = rng.integers(0, 4, 3000, dtype=np.uint8)
    t[700:2700] = u.mutate(rng, q, 4, 0.03, 0.0)[:2000]
    mat = u.simple_mat(4, 40, 30)
    exp = s.oracle_batch([q], [t], mat, 4, 2, 4)
    assert exp[0, 0] > 65535
    capfd.readouterr()
    np.testing.assert_array_equal(lib.sg_batch([q], [t], mat, 4, 2, m=4), exp)
    assert _tasks(capfd.readouterr().err, 1)[:2] == (0, 1)
    # an unrelated pair under +1 / -100: strongly negative, packed and int32
    q, t = np.zeros(40, np.uint8), np.ones(1300, np.uint8)
    for costs, expect in (((20, 3), None), ((2, 1), (-(2 + 40), 39, 0))):   # (2, 1): inserting the whole query is best -> (-B, qlen - 1, 0)
        exp = s.oracle_batch([q], [t], u.simple_mat(4, 1, 100), *costs, 4)
        assert exp[0, 0] < -40 and (expect is None or tuple(exp[0]) == expect)
        for form in ("2", "0"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            np.testing.assert_array_equal(lib.sg_batch([q], [t], u.simple_mat(4, 1, 100), *costs, m=4), exp, str((costs, form)))


@pytest.mark.parametrize("m", [5, 20])
def test_matrix_without_a_positive_entry(lib, monkeypatch, capfd, m):
    rng = np.random.default_rng(8 + m)
    mat = u.random_mat(rng, m, -7, 1)
    assert mat.max() <= 0
    qs, ts = u.ragged(rng, 60, m, 1, 150)
    ts = [np.concatenate([x, rng.integers(0, m, int(rng.integers(0, 1200)), dtype=np.uint8)]) for x in ts]
    exp = s.oracle_batch(qs, ts, mat, 3, 1, m)
    for form in ("2", "0"):
        monkeypatch.setenv("KSW2AMD_LL_FORM", form)
        capfd.readouterr()
        np.testing.assert_array_equal(lib.sg_batch(qs, ts, mat, 3, 1, m=m), exp, form)
        pk, i32, _ = _tasks(capfd.readouterr().err, 60)
        assert pk + i32 > 0                                                 # launched, although nothing scores above 0
    assert (lib.ll_batch(qs, ts, mat, 3, 1, m=m) == np.array([0, -1, -1])).all()


@pytest.mark.parametrize("form", ["1", "0"])
def test_golden_file(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    total = 0
    for name, m, mat, gapo, gape, q, t, exp in s.load_golden():
        np.testing.assert_array_equal(lib.sg_batch(q, t, mat, gapo, gape, m=m), exp, name)
        np.testing.assert_array_equal(lib.sg_batch_flat(*lf.arena(q, t, lead=1, gap=3), mat, gapo, gape, m=m), exp, name)
        total += len(q)
    assert total >= 300


# ---------------------------------------------------------------- corners and bad arguments

def test_corners_and_bad_arguments(lib, capfd):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    e = np.zeros(0, np.uint8)
    q5 = np.array([0, 1, 2, 3, 0], np.uint8)
    capfd.readouterr()
    np.testing.assert_array_equal(lib.sg_batch([e, q5, e], [q5, e, e], mat, 4, 2, m=5), [[0, -1, -1], [-14, 4, -1], [0, -1, -1]])
    assert lib.sg_batch([], [], mat, 4, 2, m=5).shape == (0, 3)
    assert "pk_tasks=0 int32_tasks=0" in capfd.readouterr().err              # nothing to launch
    np.testing.assert_array_equal(lib.sg_batch([q5, e, q5], [e, q5, q5], mat, 4, 2, m=5), [[-14, 4, -1], [0, -1, -1], [10, 4, 4]])
    np.testing.assert_array_equal(lib.sg_batch_flat(*lf.arena([q5, e, q5], [e, q5, q5], lead=2, gap=1), mat, 4, 2, m=5), [[-14, 4, -1], [0, -1, -1], [10, 4, 4]])
    # every bad argument: KSW2AMD_E_PARAM before anything is staged or launched
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = lib.local_pairs(q, t)
    res = (ka.LocalResult * 6)()
    L = lib.lib
    mp = mat.ctypes.data_as(_i8p)
    a = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = lib._local_flat(*a, None)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    ql = (0x3fffffff - 127 - 127) // (127 + 127) + 1
    bad_t = [x.copy() for x in t]
    bad_t[4][3] = 5
    bad_t[2][len(bad_t[2]) - 1] = 9
    stats = lib.host_stats()
    capfd.readouterr()
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, 128), (5, mp, -1, 2)):
        assert L.ksw2amd_sg_batch(*args, 6, pairs, res) == -2, args
        assert L.ksw2amd_sg_batch_flat(*args, 6, ctypes.byref(f), res) == -2, args
    assert L.ksw2amd_sg_batch(5, mp, 4, 2, 6, None, res) == -2 and L.ksw2amd_sg_batch(5, mp, 4, 2, 6, pairs, None) == -2
    assert L.ksw2amd_sg_batch_flat(5, mp, 4, 2, 6, None, res) == -2
    with pytest.raises(ka.Ksw2Error, match=r"pair 2: residue code >= m"):
        lib.sg_batch(q, bad_t, mat, 4, 2, m=5)
    pairs[1].qlen = ql                                                       # the range limit (only the length is looked at)
    assert L.ksw2amd_sg_batch(5, big.ctypes.data_as(_i8p), 127, 127, 2, pairs, res) == -2 and "0x3fffffff" in lib.last_error()
    pairs[1].qlen = len(q[1])
    before = lib.error_count()
    qe, te = ctypes.c_int(5), ctypes.c_int(5)
    assert L.ksw2amd_sg(None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, ctypes.byref(qe), ctypes.byref(te)) == 0
    assert (qe.value, te.value) == (-1, -1) and lib.error_count() > before
    assert lib.sg(q[0], t[0], mat, 200, 2) == (0, -1, -1)
    assert "sg: pairs" not in capfd.readouterr().err and lib.host_stats() == stats     # nothing was staged or launched by any of them


# ---------------------------------------------------------------- flat arenas, the single-pair entry, a C caller

@pytest.mark.parametrize("kind", ["host", "pinned", "device"])
def test_flat_arenas(lib, capfd, kind):
    """a host arena, a page-locked arena and a device arena equal the pointer entry; a code >= m inside a referenced sequence is caught on
    the device with the lowest pair named, a bad byte between sequences is ignored"""
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    qq = rng.integers(0, 5, 150, dtype=np.uint8)
    ts = [np.concatenate([rng.integers(0, 5, int(rng.integers(1, 1400)), dtype=np.uint8), u.mutate(rng, qq, 5, 0.05, 0.1)]) for _ in range(64)]
    base, qo, ql, to, tl = lf.arena([qq], ts, lead=1, gap=3, fill=255)       # 255 between the sequences: never looked at
    n = len(ts)
    a = (base, np.repeat(qo, n), np.repeat(ql, n), to, tl)                  # ONE copy of the query in the arena
    exp = lib.sg_batch([qq] * n, ts, mat, 4, 2, m=5)
    np.testing.assert_array_equal(exp, s.oracle_batch([qq] * n, ts, mat, 4, 2, 5))
    with placed(lib, base, kind) as kw:
        capfd.readouterr()
        np.testing.assert_array_equal(lib.sg_batch_flat(*a, mat, 4, 2, m=5, **kw), exp)
        assert ("arena=device" if kind == "device" else "arena=host") in capfd.readouterr().err
    bad = base.copy()
    bad[int(to[40]) + 2] = 5
    bad[int(to[9]) + int(tl[9]) - 1] = 200
    with placed(lib, bad, kind) as kw:
        out = np.full((n, 3), 7, np.int32)
        with pytest.raises(ka.Ksw2Error, match=r"pair 9: residue code >= m"):
            lib.sg_batch_flat(bad, *a[1:], mat, 4, 2, m=5, out=out, **kw)
        assert (out == np.array([0, -1, -1])).all()


def test_single_pair_and_c_caller(lib, tmp_path):
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 1, 80)
    t = [np.concatenate([x, rng.integers(0, 5, int(rng.integers(0, 1300)), dtype=np.uint8)]) for x in t]
    q += [np.zeros(0, np.uint8), q[0]]
    t += [t[0], np.zeros(0, np.uint8)]
    exp = s.oracle_batch(q, t, mat, 4, 2, 5)
    for i in range(len(q)):
        assert lib.sg(q[i], t[i], mat, 4, 2) == tuple(int(x) for x in lib.sg_batch([q[i]], [t[i]], mat, 4, 2, m=5)[0]) == tuple(int(x) for x in exp[i])
    exe = str(tmp_path / "sg_caller")
    libdir = os.path.dirname(os.path.abspath(lib.path))
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "dropin", "sg_caller.c"),
                    "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    inp = str(tmp_path / "pairs.txt")
    with open(inp, "w") as f:
        f.write("%d %d %d\n%s\n%d\n" % (5, 4, 2, " ".join(str(int(x)) for x in mat), len(q)))
        for x, y in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(x), " ".join(map(str, x.tolist())), len(y), " ".join(map(str, y.tolist()))))
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
    got = np.array([list(map(int, l.split())) for l in out.strip().splitlines()], dtype=np.int32)
    np.testing.assert_array_equal(got, np.concatenate([exp, exp]))
