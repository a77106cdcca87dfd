"""CPU: semi-global alignment (ksw2amd_sg_batch / ksw2amd_sg_batch_flat / ksw2amd_sg; include/ksw2_amd.h).  The
contract's formula (tests/sg_oracle.c) is pinned to the compiled reference's scalar ksw_extz through tests/golden/sg_cases.npz and to a
brute-force statement of the formula and its tie rule; the product's host code and lane code (K2aLaneLL<.., FIT = true>, both number
formats and both score lookups) run on a test-local lock-step simulator build against that formula; a C caller compiled against
include/ksw2_amd.h prints the formula's answers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import llf_util as lf
from tests import sg_util as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (6, 1), (0, 0))


@pytest.fixture(scope="module")
def simso(tmp_path_factory):
    return s.sim_library(str(tmp_path_factory.mktemp("sgsim") / "libksw2_amd.so"))


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


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 3)
    return mat.reshape(-1)


def _both(lib, q, t, mat, gapo, gape, m, exp=None, msg=""):
    """ksw2amd_sg_batch and ksw2amd_sg_batch_flat (host arena with bytes that no matrix admits between the sequences) against the formula"""
    exp = s.oracle_batch(q, t, mat, gapo, gape, m) if exp is None else exp
    np.testing.assert_array_equal(lib.sg_batch(list(q), list(t), mat, gapo, gape, m=m), exp, str(msg))
    np.testing.assert_array_equal(lib.sg_batch_flat(*lf.arena(q, t, lead=3, gap=2), mat, gapo, gape, m=m), exp, str((msg, "flat")))
    return exp


# ---------------------------------------------------------------- the oracle itself

def test_oracle_equals_the_golden_file_of_the_compiled_reference():
    total = 0
    for name, m, mat, gapo, gape, q, t, exp in s.load_golden():
        np.testing.assert_array_equal(s.oracle_batch(q, t, mat, gapo, gape, m), exp, name)
        assert max(len(x) for x in q) <= 120 and max(len(x) for x in t) <= 400
        total += len(q)
    assert total >= 300
    names = [c[0] for c in s.load_golden()]
    assert any(c[3] == 0 for c in s.load_golden()) and any(c[4] == 0 for c in s.load_golden()) and any(c[1] == 20 for c in s.load_golden())
    assert any(int(c[2].max()) <= 0 for c in s.load_golden()), names


def test_golden_inputs_are_the_generators():
    """the file holds what tests/sg_util.golden_inputs() makes: tests/gen_sg_golden.py reproduces it where the reference is built"""
    for (name, m, mat, gapo, gape, q, t), g in zip(s.golden_inputs(), s.load_golden()):
        assert (name, m, gapo, gape) == (g[0], g[1], g[3], g[4]) and (mat == g[2]).all()
        assert all((a == b).all() for a, b in zip(q + t, g[5] + g[6]))


def test_oracle_is_the_formula_brute_force(sim):
    """tests/sg_oracle.c against full matrices in plain Python with unclamped gap states and the tie rule on the last column; the library
    (simulator build, biased and clamped values, packed and int32) returns the same."""
    rng = np.random.default_rng(5)
    for ci, (gapo, gape) in enumerate(((4, 2), (0, 1), (3, 0), (0, 0), (7, 3), (1, 1))):
        for m, mat in ((3, np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)), (4, u.random_mat(rng, 4, -6, 1)), (2, u.random_mat(rng, 2))):
            qs, ts = [], []
            for k in range(50):
                a = 1 if k % 5 == 0 else m                                   # homopolymers: every row ties
                q = rng.integers(0, a, int(rng.integers(1, 13)), dtype=np.uint8)
                t = rng.integers(0, a, int(rng.integers(1, 25)), dtype=np.uint8)
                if k % 3 == 0:
                    t = np.concatenate([t[:5], q, t[5:], q]).astype(np.uint8)    # two copies: a tie between two rows
                qs.append(q); ts.append(t)
            exp = np.array([s.brute(q, t, mat, gapo, gape, m) for q, t in zip(qs, ts)], dtype=np.int32)
            np.testing.assert_array_equal(s.oracle_batch(qs, ts, mat, gapo, gape, m), exp, str((gapo, gape, m)))
            os.environ["KSW2AMD_LL_FORM"] = str(ci % 3)
            np.testing.assert_array_equal(sim.sg_batch(qs, ts, mat, gapo, gape, m=m), exp, str((gapo, gape, m)))


# ---------------------------------------------------------------- the library on the simulator

@pytest.mark.parametrize("form", ["0", "1", "2"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_ragged_batch_every_form(sim, form, lds):
    rng = np.random.default_rng(11 + int(form))
    os.environ["KSW2AMD_LL_FORM"] = form
    os.environ["KSW2AMD_LL_LDS"] = lds
    for m, mat in ((5, u.simple_mat(5, 2, 4, -1)), (20, _m20(rng)), (4, u.random_mat(rng, 4, -6, 1))):
        q, t = u.ragged(rng, 24, m, 1, 90, related=0.6)
        t = [np.concatenate([x, rng.integers(0, m, int(rng.integers(0, 200)), dtype=np.uint8)]) for x in t]
        q += [q[0], q[0], q[1]]
        t += [t[0], t[0][::-1].copy(), t[1]]                               # same-shape partners for form 1
        t[3] = rng.integers(0, m, 1100, dtype=np.uint8)                    # two generations: the boundary in the scratch
        t[4] = np.concatenate([rng.integers(0, m, 1030, dtype=np.uint8), q[4]])
        for gapo, gape in COSTS:
            _both(sim, q, t, mat, gapo, gape, m, msg=(form, lds, m, gapo, gape))


@pytest.mark.parametrize("form", ["0", "2"])
def test_golden_file_on_the_simulator(sim, form):
    os.environ["KSW2AMD_LL_FORM"] = form
    for name, m, mat, gapo, gape, q, t, exp in s.load_golden():
        _both(sim, q, t, mat, gapo, gape, m, exp=exp, msg=name)


@pytest.mark.parametrize("form", ["0", "2"])
def test_edge_grid(sim, form):
    """tlen 1 .. 2 049 x qlen 1 .. 65, the query planted so that the best row is the last of a lane, the first of the next, the last of
    generation 0, the first of generation 1, the last of the target"""
    rng = np.random.default_rng(77)
    os.environ["KSW2AMD_LL_FORM"] = form
    mat = s.unit_mat(5)
    tlens, qlens = (1, 15, 16, 17, 1023, 1024, 1025, 2049), (1, 2, 3, 4, 5, 63, 64, 65)
    qs, ts = s.edge_grid(rng, 5, tlens, qlens)
    exp = _both(sim, qs, ts, mat, 4, 2, 5, msg=form)
    k, seen = 0, set()
    for tl in tlens:
        for ql in qlens:
            for r in s.edge_rows(tl):
                if ql <= r + 1:                                             # the whole copy fits in front of row r
                    assert tuple(exp[k]) == (2 * ql, ql - 1, r), (tl, ql, r, exp[k])
                    seen.add(r)
                k += 1
    assert {15, 16, 1023, 1024, 2048} <= seen


@pytest.mark.parametrize("form", ["0", "2"])
def test_ties_take_the_smallest_te(sim, form):
    os.environ["KSW2AMD_LL_FORM"] = form
    qs, ts, tes = s.tie_pairs()
    exp = _both(sim, qs, ts, s.unit_mat(5), 4, 2, 5, msg=form)
    assert [int(x) for x in exp[:, 2]] == tes and (exp[:, 0] == 12).all()
    for q, t, te in zip(qs[:2], ts[:2], tes[:2]):
        assert s.brute(q, t, s.unit_mat(5), 4, 2, 5) == (12, 5, te)


def test_admission_bound(sim, capfd):
    """smax = 127, costs (5, 1): B + (qlen + 1) * smax = 128 qlen + 132 <= 65 535 up to qlen 510"""
    os.environ["KSW2AMD_LL_FORM"] = "2"
    os.environ["KSW2AMD_TRACE"] = "1"
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    for ql, packed in ((510, True), (511, False)):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q, rng.integers(0, 4, 9, dtype=np.uint8)])
        capfd.readouterr()
        got = sim.sg_batch([q], [t], mat, 5, 1, m=4)
        err = capfd.readouterr().err
        assert tuple(got[0]) == (127 * ql, ql - 1, 20 + ql - 1)
        np.testing.assert_array_equal(got, s.oracle_batch([q], [t], mat, 5, 1, 4))
        assert ("sg: pairs=1 pk_tasks=%d int32_tasks=%d" % ((1, 0) if packed else (0, 1))) in err, err


def test_scores_beyond_16_bits_negative_scores_and_all_insert(sim):
    rng = np.random.default_rng(4)
    os.environ["KSW2AMD_LL_FORM"] = "2"
    q = rng.integers(0, 4, 1700, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q])
    exp = _both(sim, [q], [t], u.simple_mat(4, 40, 30), 4, 2, 4)
    assert exp[0, 0] == 40 * 1700 > 65535
    # an unrelated pair under +1 / -100: strongly negative
    q, t = np.zeros(40, np.uint8), np.ones(300, np.uint8)
    exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), 20, 3, 4)
    assert exp[0, 0] < -100
    # inserting the whole query is best: (-B, qlen - 1, 0)
    exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), 2, 1, 4)
    assert tuple(exp[0]) == (-(2 + 40), 39, 0)
    # a matrix without a positive entry: the local entries launch nothing, these do
    mat = u.random_mat(rng, 5, -7, 1)
    assert mat.max() <= 0
    qs, ts = u.ragged(rng, 12, 5, 1, 60)
    before = s.launches(sim, reset=True)
    exp = _both(sim, qs, ts, mat, 3, 1, 5)
    assert (exp[:, 0] <= 0).all() and s.launches(sim)[0] > 0
    assert (sim.ll_batch(qs, ts, mat, 3, 1, m=5) == np.array([0, -1, -1])).all()


def test_corner_results_launch_nothing(sim):
    e = np.zeros(0, np.uint8)
    q = np.array([0, 1, 2, 3, 0], np.uint8)
    mat = u.simple_mat(5, 2, 4, -1)
    s.launches(sim, reset=True)
    exp = np.array([[0, -1, -1], [-(4 + 5 * 2), 4, -1], [0, -1, -1]], np.int32)
    np.testing.assert_array_equal(sim.sg_batch([e, q, e], [q, e, e], mat, 4, 2, m=5), exp)
    np.testing.assert_array_equal(s.oracle_batch([e, q, e], [q, e, e], mat, 4, 2, 5), exp)
    assert s.launches(sim)[:2] == (0, 0)
    np.testing.assert_array_equal(sim.sg_batch_flat(*lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, 4, 2, m=5), exp)
    assert s.launches(sim)[:2] == (0, 0)                                    # (the flat entry's check ran)
    assert sim.sg_batch([], [], mat, 4, 2, m=5).shape == (0, 3)
    # corners beside real pairs
    np.testing.assert_array_equal(sim.sg_batch([q, e, q], [e, q, q], mat, 4, 2, m=5), [[-14, 4, -1], [0, -1, -1], [10, 4, 4]])
    assert sim.sg(q, e, mat, 4, 2) == (-14, 4, -1) and sim.sg(e, q, mat, 4, 2) == (0, -1, -1) and sim.sg(q, q, mat, 4, 2) == (10, 4, 4)


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
    s.launches(sim, reset=True)
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, 128), (5, mp, -1, 2), (5, mp, 4, -1)):
        assert L.ksw2amd_sg_batch(*args, 6, pairs, res) == E, args
        assert L.ksw2amd_sg_batch_flat(*args, 6, ctypes.byref(f), res) == E, args
    assert L.ksw2amd_sg_batch(5, mp, 4, 2, 6, None, res) == E and L.ksw2amd_sg_batch(5, mp, 4, 2, 6, pairs, None) == E
    assert L.ksw2amd_sg_batch(5, mp, 4, 2, -1, pairs, res) == E
    assert L.ksw2amd_sg_batch_flat(5, mp, 4, 2, 6, None, res) == E and L.ksw2amd_sg_batch_flat(5, mp, 4, 2, 6, ctypes.byref(f), None) == E
    # a code >= m: named by the pointer entry before anything runs, caught on the "device" by the flat entry with the lowest pair named
    bad_t = [x.copy() for x in t]
    bad_t[4][3] = 5
    bad_t[2][len(bad_t[2]) - 1] = 9
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        sim.sg_batch(q, bad_t, mat, 4, 2, m=5)
    out = np.full((6, 3), 7, np.int32)
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        sim.sg_batch_flat(*lf.arena(q, bad_t, lead=1, gap=2), mat, 4, 2, m=5, out=out)
    assert (out == np.array([0, -1, -1])).all()
    # the range limit: gapo + qlen * (gape + smax) + smax > 0x3fffffff (only the length is looked at before the rejection)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    ql = (0x3fffffff - 127 - 127) // (127 + 127) + 1
    assert 127 + ql * 254 + 127 > 0x3fffffff >= 127 + (ql - 1) * 254 + 127
    pairs[1].qlen = ql
    assert L.ksw2amd_sg_batch(5, big.ctypes.data_as(_i8p), 127, 127, 1, ctypes.byref(pairs[1]), res) == E
    assert "0x3fffffff" in sim.last_error()
    pairs[1].qlen = len(q[1])
    ql_arr = a[2].copy()
    ql_arr[3] = ql
    f2, _, keep3 = sim._local_flat(a[0], a[1], ql_arr, a[3], a[4], None)
    assert L.ksw2amd_sg_batch_flat(5, big.ctypes.data_as(_i8p), 127, 127, 6, ctypes.byref(f2), res) == E
    assert "pair 3" in sim.last_error()
    assert s.launches(sim)[:2] == (0, 0)                                    # nothing of all this launched an alignment kernel
    # ksw2amd_sg reports like ksw_ll_i16: 0 with the coordinates at -1, the error counted
    before = sim.error_count()
    qe, te = ctypes.c_int(5), ctypes.c_int(5)
    assert L.ksw2amd_sg(None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, ctypes.byref(qe), ctypes.byref(te)) == 0
    assert (qe.value, te.value) == (-1, -1) and sim.error_count() > before and "NULL profile" in sim.last_error()
    assert sim.sg(q[0], t[0], mat, 200, 2) == (0, -1, -1) and "gapo and gape" in sim.last_error()


def test_chunked_flat_batches(sim):
    """KSW2AMD_LL_CHUNK_BYTES cuts the flat batch into several chunks: the same results, a bad code in a later chunk leaves the earlier
    chunks' results and resets its own and the later ones"""
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 40, 5, 10, 200)
    q[7], t[9] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    exp = s.oracle_batch(q, t, mat, 4, 2, 5)
    a = lf.arena(q, t, lead=1, gap=1)
    os.environ["KSW2AMD_LL_CHUNK_BYTES"] = "4000"
    s.launches(sim, reset=True)
    np.testing.assert_array_equal(sim.sg_batch_flat(*a, mat, 4, 2, m=5), exp)
    assert s.launches(sim)[2] > 3
    bad = a[0].copy()
    bad[int(a[3][30]) + 1] = 6
    out = np.full((40, 3), 7, np.int32)
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
        sim.sg_batch_flat(bad, *a[1:], mat, 4, 2, m=5, out=out)
    k = int(np.nonzero((out != exp).any(1))[0][0])
    assert 0 < k <= 30 and (out[:k] == exp[:k]).all() and (out[k:] == np.array([0, -1, -1])).all()


def _write_input(path, q, t, mat, m, go, ge):
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n%d\n" % (m, go, ge, " ".join(str(int(x)) for x in mat), len(q)))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))


def test_c_caller(simso, tmp_path):
    exe = str(tmp_path / "sg_caller")
    libdir = os.path.dirname(simso)
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "dropin", "sg_caller.c"),
                    "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 1, 80)
    t = [np.concatenate([x, rng.integers(0, 5, 300, dtype=np.uint8)]) for x in t]
    q.append(np.zeros(0, np.uint8)); t.append(t[0])
    q.append(q[0]); t.append(np.zeros(0, np.uint8))
    inp = str(tmp_path / "pairs.txt")
    _write_input(inp, q, t, mat, 5, 4, 2)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
    got = np.array([list(map(int, l.split())) for l in out.strip().splitlines()], dtype=np.int32)
    exp = s.oracle_batch(q, t, mat, 4, 2, 5)
    np.testing.assert_array_equal(got, np.concatenate([exp, exp]))


def test_other_host_objects_do_not_name_the_semiglobal_launcher(tmp_path):
    """only ksw2_host_sg.o refers to k2a_shim_launch_sg: the simulator builds of the other tests/*_util.py link ksw2_host_ll.o and
    ksw2_host_llf.o against twins without it"""
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    for h, named in (("ll", False), ("llf", False), ("sg", True)):
        o = str(tmp_path / ("host_%s.o" % h))
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        undefined = subprocess.run(["nm", "-u", o], check=True, capture_output=True, text=True).stdout
        assert ("k2a_shim_launch_sg" in undefined) == named, (h, undefined)
