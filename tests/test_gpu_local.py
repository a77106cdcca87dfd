"""GPU: local alignment (ksw_ll_qinit / ksw_ll_i16, ksw2amd_ll_batch) on libksw2_amd.so against the scalar test oracle
(tests/ll_oracle.c): ragged batches, both kernel forms and both score lookups, the packed admission bound, a score above 65 535,
tie-heavy repeats, empty and single batches, bad arguments, single calls and a C caller built against include/ksw2_amd.h."""
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_util as u

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def _run(lib, monkeypatch, capfd, q, t, mat, go, ge, form="1", lds="0", m=None):
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
    capfd.readouterr()
    r = lib.ll_batch(q, t, mat, go, ge, m=m)
    return r, capfd.readouterr().err


@pytest.mark.parametrize("m", [5, 20])
def test_ragged_parity(lib, monkeypatch, capfd, m):
    rng = np.random.default_rng(40 + m)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else u.random_mat(rng, m)
    q, t = u.ragged(rng, 10000, m, 1, 600, related=0.4)
    q2, t2 = u.ragged(rng, 200, m, 1, 5000, related=0.4)            # lengths 1-5 000 (the oracle is scalar: the long ones are few)
    q, t = q + q2, t + t2
    for go, ge in ((4, 2), (0, 1), (6, 1)):
        got, err = _run(lib, monkeypatch, capfd, q, t, mat, go, ge)
        np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, go, ge, m), err_msg="%s %s" % ((go, ge), err))


@pytest.mark.parametrize("form,lds", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1"), ("2", "0")])
def test_uniform_packed_and_forced_forms(lib, monkeypatch, capfd, form, lds):
    rng = np.random.default_rng(7)
    mat = u.simple_mat(5, 2, 4, -1)
    q = [rng.integers(0, 5, 256, dtype=np.uint8) for _ in range(512)]
    t = [np.concatenate([rng.integers(0, 5, 300, dtype=np.uint8), u.mutate(rng, x, 5)[:200], rng.integers(0, 5, 1024, dtype=np.uint8)])[:1024]
         for x in q]
    q += [rng.integers(0, 5, 3000, dtype=np.uint8) for _ in range(6)]       # several generations, rows = the query
    t += [rng.integers(0, 5, 2500, dtype=np.uint8) for _ in range(6)]
    got, err = _run(lib, monkeypatch, capfd, q, t, mat, 4, 2, form, lds)
    np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, 4, 2))
    pk = int(re.search(r"pk_tasks=(\d+)", err).group(1))
    assert pk == 0 if form == "0" else pk >= 256, err


def test_admission_bound(lib, monkeypatch, capfd):
    mat = u.simple_mat(4, 127, 3)
    rng = np.random.default_rng(3)
    for n, packed in ((515, True), (516, False)):
        x = rng.integers(0, 4, n, dtype=np.uint8)
        q, t = [x] * 4, [x.copy()] * 4
        got, err = _run(lib, monkeypatch, capfd, q, t, mat, 5, 1)
        np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, 5, 1))
        assert got[0][0] == 127 * n
        assert ("pk_tasks=2 " in err) == packed, (n, err)


def test_score_above_16_bits(lib):
    rng = np.random.default_rng(8)
    mat = u.simple_mat(5, 4, 4, -1)
    x = rng.integers(0, 4, 20000, dtype=np.uint8)
    y = u.mutate(rng, x, 4, 0.002, 0.001)
    got = lib.ll_batch([x], [y], mat, 4, 2)
    exp = u.oracle_batch([x], [y], mat, 4, 2)
    assert exp[0][0] > 65535
    np.testing.assert_array_equal(got, exp)


def test_tie_heavy_repeats(lib, monkeypatch, capfd):
    rng = np.random.default_rng(12)
    mat = u.simple_mat(2, 1, 1)
    q, t = [], []
    for k in range(400):
        unit = rng.integers(0, 2, int(rng.integers(1, 6)), dtype=np.uint8)
        q.append(np.tile(unit, int(rng.integers(1, 40))))
        t.append(np.tile(unit, int(rng.integers(1, 400))))
    for form in ("0", "2"):
        for go, ge in ((0, 0), (1, 1)):
            got, _ = _run(lib, monkeypatch, capfd, q, t, mat, go, ge, form, "0", m=2)
            np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, go, ge, 2))


def test_empty_and_single(lib):
    mat = u.simple_mat(5, 2, 4, -1)
    assert lib.ll_batch([], [], mat, 4, 2).shape == (0, 3)
    x = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    np.testing.assert_array_equal(lib.ll_batch([x], [x[1:]], mat, 4, 2), u.oracle_batch([x], [x[1:]], mat, 4, 2))
    np.testing.assert_array_equal(lib.ll_batch([x, np.zeros(0, np.uint8)], [np.zeros(0, np.uint8), x], mat, 4, 2), [[0, -1, -1]] * 2)


def test_bad_arguments(lib, monkeypatch, capfd):
    mat = u.simple_mat(5, 2, 4, -1)
    x = np.array([0, 1, 2], np.uint8)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for args in (([x], [np.array([5], np.uint8)], mat, 4, 2), ([x], [x], mat, 128, 2), ([x], [x], mat, 4, -1)):
        capfd.readouterr()
        with pytest.raises(ka.Ksw2Error, match="error -2"):
            lib.ll_batch(*args)
        assert "ll: pairs" not in capfd.readouterr().err           # rejected before anything was staged or launched
    with pytest.raises(ka.Ksw2Error, match="ksw_ll_qinit"):
        lib.ll_i16(np.array([9], np.uint8), x, mat, 4, 2)
    with pytest.raises(ka.Ksw2Error, match="ksw_ll_qinit"):
        lib.ll_i16(x, x, mat, 4, 2, size=3)


def test_ll_i16_single_calls(lib):
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 20, 5, 1, 3000)
    exp = u.oracle_batch(q, t, mat, 4, 2)
    for i in range(len(q)):
        assert lib.ll_i16(q[i], t[i], mat, 4, 2) == tuple(int(v) for v in exp[i])


def test_dropin_caller_product_header(lib, tmp_path):
    exe = str(tmp_path / "ll_caller")
    sodir = os.path.dirname(ka.DEFAULT_SO)
    subprocess.run(["gcc", "-O1", "-Wall", "-DUSE_KSW2_AMD", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "ll_caller.c"), "-L" + sodir, "-l:libksw2_amd.so", "-Wl,-rpath," + sodir], check=True)
    rng = np.random.default_rng(22)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 10, 5, 1, 1500)
    inp = str(tmp_path / "pairs.txt")
    with open(inp, "w") as f:
        f.write("5 4 2\n%s\n%d\n" % (" ".join(str(int(v)) for v in mat), len(q)))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=300).stdout
    got = np.array([list(map(int, l.split())) for l in out.strip().splitlines()], dtype=np.int32)
    np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, 4, 2))
