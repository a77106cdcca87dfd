"""CPU: local alignment (ksw_ll_qinit / ksw_ll_i16, ksw2amd_ll_batch; include/ksw2_amd.h).  The test oracle (tests/ll_oracle.c) is pinned
to the compiled reference's scalar ksw_extz and to a brute-force check of the tie rule; the product's host code and lane code
(ksw2_lane_ll.h, both kernel forms and both score lookups) run on a test-local lock-step simulator build against that oracle; a caller
compiled against the reference's own ksw2.h links the simulator build and prints the oracle's answers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libksw2ref.so")
REF_DIR = "/root/reference"
KSW_EZ_SCORE_ONLY, KSW_EZ_EXTZ_ONLY = 0x01, 0x40


@pytest.fixture(scope="module")
def sim():
    return ksw2_amd.Library(u.sim_library())


def _ref():
    if not os.path.exists(REF_SO):
        pytest.skip("oracle/_ref/libksw2ref.so not built (build() makes it where the reference's sources exist)")
    lib = ctypes.CDLL(REF_SO)
    lib.ksw_extz.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int8, ctypes.c_void_p,
                             ctypes.c_int8, ctypes.c_int8, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ksw2_amd.KswExtz)]
    lib.ksw_extz.restype = None
    return lib


def _ref_ext_max(ref, q, t, mat, m, gapo, gape):
    q, t, mat = np.ascontiguousarray(q[::-1]), np.ascontiguousarray(t[::-1]), np.ascontiguousarray(mat, dtype=np.int8)
    ez = ksw2_amd.KswExtz()
    ref.ksw_extz(None, len(q), q.ctypes.data, len(t), t.ctypes.data, m, mat.ctypes.data, gapo, gape, -1, -1,
                 KSW_EZ_EXTZ_ONLY | KSW_EZ_SCORE_ONLY, ctypes.byref(ez))
    return int(ez.max_zd & 0x7fffffff)


def _pin_sets(rng):
    """(queries, targets, mat, m, gapo, gape) sets: m = 5 with a wildcard row, m = 20 random, near-identical pairs, gapo = 0."""
    m5 = u.simple_mat(5, 2, 4, -1)
    m20 = u.random_mat(rng, 20)
    out = []
    q, t = u.ragged(rng, 600, 5, 1, 160, related=0.3)
    out.append((q, t, m5, 5, 4, 2))
    q, t = u.ragged(rng, 500, 20, 1, 120, related=0.3)
    out.append((q, t, m20, 20, 6, 1))
    q = [rng.integers(0, 4, int(rng.integers(20, 200)), dtype=np.uint8) for _ in range(500)]
    out.append((q, [u.mutate(rng, x, 4, 0.03, 0.02) for x in q], m5, 5, 4, 2))
    q, t = u.ragged(rng, 500, 5, 1, 120, related=0.5)
    out.append((q, t, m5, 5, 0, 1))
    return out


def test_oracle_pinned_to_reference_extz(sim):
    """For the oracle's best cell (qe, te): the reference's scalar ksw_extz on reversed query[0..qe] / target[0..te] (extension only,
    unbanded, no Z-drop) reaches exactly the local score.  The library's lane code (simulator build) returns the same cells."""
    ref = _ref()
    rng = np.random.default_rng(11)
    total = 0
    for q, t, mat, m, go, ge in _pin_sets(rng):
        res = u.oracle_batch(q, t, mat, go, ge, m)
        np.testing.assert_array_equal(sim.ll_batch(q, t, mat, go, ge, m=m), res)
        for i in range(len(q)):
            s, qe, te = map(int, res[i])
            total += 1
            if s == 0:
                assert qe == -1 and te == -1
                continue
            assert _ref_ext_max(ref, q[i][:qe + 1], t[i][:te + 1], mat, m, go, ge) == s, (i, s, qe, te, go, ge)
    assert total >= 2000


def test_oracle_tie_rule_brute_force(sim):
    """Tiny pairs over two letters with many equal maxima: the oracle's cell -- and the library's (simulator build) -- is the brute-force
    choice (largest score, smallest te, then smallest qe)."""
    rng = np.random.default_rng(5)
    mat = u.simple_mat(2, 1, 1)
    for k in range(400):
        q = rng.integers(0, 2, int(rng.integers(1, 9)), dtype=np.uint8)
        t = np.tile(q, 3) if k % 3 == 0 else rng.integers(0, 2, int(rng.integers(1, 9)), dtype=np.uint8)
        go, ge = [(1, 1), (0, 1), (0, 0), (2, 0)][k % 4]
        b = u.brute(q, t, mat, go, ge, 2)
        assert tuple(int(x) for x in u.oracle_batch([q], [t], mat, go, ge, 2)[0]) == b, (q, t, go, ge)
        assert tuple(int(x) for x in sim.ll_batch([q], [t], mat, go, ge, m=2)[0]) == b, (q, t, go, ge)


def test_local_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ksw2_amd.h")).read(), flags=re.S)
    for name in ("ksw_ll_qinit", "ksw_ll_i16", "ksw2amd_ll_batch"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ksw2_amd.EXPORTS
    if not os.path.exists(ksw2_amd.DEFAULT_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ksw2_amd", "csrc")], check=True, capture_output=True)
    lib = ctypes.CDLL(ksw2_amd.DEFAULT_SO)
    for name in ("ksw_ll_qinit", "ksw_ll_i16", "ksw2amd_ll_batch"):
        assert hasattr(lib, name), name


def _forms(sim, monkeypatch, capfd, q, t, mat, go, ge, m=None):
    """every (form, score lookup) the switches force; returns {(form, lds): (result, trace line)}"""
    out = {}
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form in ("0", "1", "2"):
        for lds in ("0", "1"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
            capfd.readouterr()
            r = sim.ll_batch(q, t, mat, go, ge, m=m)
            out[(form, lds)] = (r, capfd.readouterr().err)
    return out


@pytest.mark.parametrize("m,go,ge", [(5, 4, 2), (5, 0, 1), (20, 5, 2)])
def test_sim_ragged_both_forms(sim, monkeypatch, capfd, m, go, ge):
    rng = np.random.default_rng(100 + m + go)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else u.random_mat(rng, m)
    q, t = u.ragged(rng, 24, m, 1, 1500)
    for a, b in ((700, 200), (200, 700), (1, 1), (64, 1100), (300, 500), (500, 300)):   # same-shape pairs for the packed form, either
        x = rng.integers(0, m, a, dtype=np.uint8)                                         # orientation (the last two: same rows and
        for _ in range(2):                                                                # columns, opposite orientations)
            q.append(x)
            t.append(rng.integers(0, m, b, dtype=np.uint8))
    exp = u.oracle_batch(q, t, mat, go, ge, m)
    for key, (got, err) in _forms(sim, monkeypatch, capfd, q, t, mat, go, ge).items():
        np.testing.assert_array_equal(got, exp, err_msg=str(key))
        pk = int(re.search(r"pk_tasks=(\d+)", err).group(1))
        assert (pk == 0) if key[0] == "0" else (pk > 0), (key, err)
        assert ("profile=lds" in err) == (key[1] == "1" or m > 5), (key, err)


def test_sim_packed_admission_bound(sim, monkeypatch, capfd):
    """smax = 127: (min(qlen, tlen) + 1) * 127 <= 65535 admits min <= 515.  Identical pairs at 515 (packed, best 65405) and 516
    (int32), and 600 (best 76200 > 65535: int32, exact)."""
    mat = u.simple_mat(4, 127, 3)
    rng = np.random.default_rng(3)
    for n, packed in ((514, True), (515, True), (516, False), (600, False)):
        x = rng.integers(0, 4, n, dtype=np.uint8)
        q, t = [x, x.copy()], [x.copy(), x.copy()]
        exp = u.oracle_batch(q, t, mat, 5, 1)
        assert exp[0][0] == 127 * n
        monkeypatch.setenv("KSW2AMD_TRACE", "1")
        monkeypatch.setenv("KSW2AMD_LL_FORM", "1")
        capfd.readouterr()
        got = sim.ll_batch(q, t, mat, 5, 1)
        err = capfd.readouterr().err
        np.testing.assert_array_equal(got, exp)
        assert ("pk_tasks=1 " in err) == packed, (n, err)


def test_sim_ll_i16_single_calls(sim):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 1, 900)
    exp = u.oracle_batch(q, t, mat, 4, 2)
    for i in range(len(q)):
        assert sim.ll_i16(q[i], t[i], mat, 4, 2, size=1 + i % 2) == tuple(int(x) for x in exp[i])
    assert sim.ll_i16(np.zeros(0, np.uint8), t[0], mat, 4, 2) == (0, -1, -1)
    assert sim.ll_i16(q[0], np.zeros(0, np.uint8), mat, 4, 2) == (0, -1, -1)


def test_sim_bad_arguments(sim):
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = [np.array([0, 1, 2], np.uint8)], [np.array([0, 1, 5], np.uint8)]       # code 5 >= m
    for args in ((q, t, mat, 4, 2), ([q[0]], [q[0]], mat, -1, 2), ([q[0]], [q[0]], mat, 4, 128)):
        with pytest.raises(ksw2_amd.Ksw2Error, match="error -2"):
            sim.ll_batch(*args)
    with pytest.raises(ksw2_amd.Ksw2Error, match="ksw_ll_qinit"):
        sim.ll_i16(np.array([7], np.uint8), q[0], mat, 4, 2)
    assert sim.ll_batch([], [], mat, 4, 2).shape == (0, 3)
    assert sim.ll_batch(q[:1], q[:1], -np.abs(mat), 4, 2).tolist() == [[0, -1, -1]]     # no positive entry: no launch


def _write_input(path, q, t, mat, m, go, ge):
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n%d\n" % (m, go, ge, " ".join(str(int(x)) for x in mat), len(q)))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))


@pytest.mark.skipif(not os.path.isdir(REF_DIR), reason="the reference's sources are not on this machine")
def test_dropin_caller_reference_header(tmp_path):
    so = u.sim_library(str(tmp_path / "libksw2_amd.so"))
    exe = str(tmp_path / "ll_caller")
    subprocess.run(["gcc", "-O1", "-Wall", "-I" + REF_DIR, "-o", exe, os.path.join(ROOT, "tests", "dropin", "ll_caller.c"),
                    "-L" + str(tmp_path), "-lksw2_amd", "-Wl,-rpath," + str(tmp_path)], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 16, 5, 1, 700)
    inp = str(tmp_path / "pairs.txt")
    _write_input(inp, q, t, mat, 5, 4, 2)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
    got = np.array([list(map(int, l.split())) for l in out.strip().splitlines()], dtype=np.int32)
    np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, 4, 2))
