"""GPU: local alignment with start cell and CIGAR (ksw2amd_ll_align_batch / ksw2amd_ll_align) on libksw2_amd.so against the contract's
formula (tests/lla_util.py: the scalar local oracle forward and on the reversed prefixes, then the project's restatement of the scalar
ksw_extz on the interval) and against tests/golden/lla_cases.npz, which the compiled reference produced."""
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_util as u
from tests import lla_util as a

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def _run(lib, monkeypatch, capfd, q, t, mat, go, ge, form="1", lds="0", flag=0, m=None):
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
    capfd.readouterr()
    r = lib.ll_align_batch(q, t, mat, go, ge, flag=flag, m=m)
    return r, capfd.readouterr().err


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 2)
    return mat.reshape(-1)


def test_golden_file(lib):
    z = np.load(os.path.join(ROOT, "tests", "golden", "lla_cases.npz"))
    total = 0
    for k in range(int(z["nsets"])):
        m, go, ge, flag = map(int, z["s%d_par" % k])
        ql, tl = z["s%d_qlen" % k], z["s%d_tlen" % k]
        q = np.split(z["s%d_q" % k], np.cumsum(ql)[:-1])
        t = np.split(z["s%d_t" % k], np.cumsum(tl)[:-1])
        res, cig = z["s%d_res" % k], z["s%d_cig" % k]
        got = lib.ll_align_batch(q, t, z["s%d_mat" % k], go, ge, flag=flag, m=m)
        pos = 0
        for i, g in enumerate(got):
            n = int(res[i][5])
            assert [g["score"], g["qb"], g["qe"], g["tb"], g["te"], g["n_cigar"]] == res[i].tolist(), (k, i, g, res[i])
            assert g["cigar"] == cig[pos:pos + n].tolist(), (k, i)
            pos += n
            total += 1
    assert total >= 300


@pytest.mark.parametrize("m", [5, 20])
def test_ragged_parity(lib, monkeypatch, capfd, m):
    rng = np.random.default_rng(140 + m)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else u.random_mat(rng, m)
    q, t = u.ragged(rng, 10000, m, 1, 600, related=0.4)
    q2, t2 = u.ragged(rng, 200, m, 1, 5000, related=0.4)
    q, t = q + q2, t + t2
    for go, ge in ((4, 2), (0, 1), (6, 1)):
        got, err = _run(lib, monkeypatch, capfd, q, t, mat, go, ge, m=m)
        a.assert_same(got, a.expected(q, t, mat, go, ge, m, which="oracle"), (go, ge))


@pytest.mark.parametrize("form,lds", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")])
def test_uniform_packed_and_forced_forms(lib, monkeypatch, capfd, form, lds):
    rng = np.random.default_rng(7)
    mat = u.simple_mat(5, 2, 4, -1)
    q = [rng.integers(0, 5, 256, dtype=np.uint8) for _ in range(512)]
    t = [np.concatenate([rng.integers(0, 5, int(rng.integers(0, 800)), dtype=np.uint8), u.mutate(rng, x, 5)[:200], rng.integers(0, 5, 1024, dtype=np.uint8)])[:1024]
         for x in q]
    q += [rng.integers(0, 5, 3000, dtype=np.uint8) for _ in range(6)]       # several generations, rows = the query
    t += [rng.integers(0, 5, 2500, dtype=np.uint8) for _ in range(6)]
    got, err = _run(lib, monkeypatch, capfd, q, t, mat, 4, 2, form, lds)
    a.assert_same(got, a.expected(q, t, mat, 4, 2, 5, which="oracle"), (form, lds))
    line = re.search(r"ll-rev: pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
    assert line, err
    assert int(line.group(1)) == 0 if form == "0" else int(line.group(1)) >= 256, err
    assert line.group(3) == ("lds" if lds == "1" else "registers"), err


@pytest.mark.parametrize("m", [5, 20])
def test_differing_end_cells_in_packed_tasks(lib, monkeypatch, capfd, m):
    rng = np.random.default_rng(200 + m)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else _m20(rng)
    go, ge = (4, 2) if m == 5 else (6, 1)
    q, t = a.new_ground(rng, m)
    exp = a.expected(q, t, mat, go, ge, m, which="oracle")
    for form in ("0", "1", "2"):
        for lds in ("0", "1"):
            got, err = _run(lib, monkeypatch, capfd, q, t, mat, go, ge, form, lds, m=m)
            a.assert_same(got, exp, (form, lds))
            pk = int(re.search(r"ll-rev: pk_tasks=(\d+)", err).group(1))
            assert (pk == 0) if form == "0" else (pk >= 12), (form, err)
    for i in (0, 9, 16, 17, 18, 20):
        r = lib.ll_align(q[i], t[i], mat, go, ge, m=m)
        assert all(r[f] == exp[i][f] for f in a.FIELDS), (i, r, exp[i])


def test_score_above_16_bits(lib):
    rng = np.random.default_rng(8)
    mat = u.simple_mat(5, 4, 4, -1)
    x = rng.integers(0, 4, 20000, dtype=np.uint8)
    y = u.mutate(rng, x, 4, 0.002, 0.001)
    exp = a.expected([x], [y], mat, 4, 2, 5, which="oracle")
    assert exp[0]["score"] > 65535
    a.assert_same(lib.ll_align_batch([x], [y], mat, 4, 2), exp)


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
            a.assert_same(got, a.expected(q, t, mat, go, ge, 2, which="oracle"), (form, go, ge))


def test_flags_and_corners(lib):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 200, 5, 1, 300, related=0.8)
    for flag in (a.RIGHT, a.REV_CIGAR, a.SCORE_ONLY):
        a.assert_same(lib.ll_align_batch(q, t, mat, 4, 2, flag=flag), a.expected(q, t, mat, 4, 2, 5, flag, which="oracle"), flag)
    for m, go, ge, lo, hi in ((5, 0, 0, -4, 3), (20, 0, 0, -6, 7), (127, 3, 1, -128, 128), (127, 127, 127, -20, 127)):
        mat = u.random_mat(rng, m, lo, hi)
        q, t = u.ragged(rng, 100, m, 1, 200, related=0.6)
        a.assert_same(lib.ll_align_batch(q, t, mat, go, ge, m=m), a.expected(q, t, mat, go, ge, m, which="oracle"), (m, go, ge))


def test_bad_arguments_and_degenerate_batches(lib, monkeypatch, capfd):
    mat = u.simple_mat(5, 2, 4, -1)
    x = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for kw in (dict(flag=0x40), dict(flag=0x800), dict(t=[np.array([0, 5], np.uint8)]), dict(go=128), dict(ge=-1)):
        capfd.readouterr()
        with pytest.raises(ka.Ksw2Error, match="error -2"):
            lib.ll_align_batch([x], kw.get("t", [x]), mat, kw.get("go", 4), kw.get("ge", 2), flag=kw.get("flag", 0))
        err = capfd.readouterr().err
        assert "ll:" not in err and "ll-rev:" not in err           # rejected before anything was staged or launched
    assert lib.ll_align_batch([], [], mat, 4, 2) == []
    r = lib.ll_align_batch([x, np.zeros(0, np.uint8)], [x, x], -np.abs(mat), 4, 2)
    assert all((d["score"], d["qb"], d["qe"], d["tb"], d["te"], d["n_cigar"]) == (0, -1, -1, -1, -1, 0) for d in r)


@pytest.mark.parametrize("pool", [False, True])
def test_c_caller_product_library(lib, tmp_path, pool):
    exe = str(tmp_path / "lla_caller")
    sodir = os.path.dirname(ka.DEFAULT_SO)
    subprocess.run(["gcc", "-O1", "-Wall", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "lla_caller.c"), "-L" + sodir, "-l:libksw2_amd.so", "-Wl,-rpath," + sodir], check=True)
    rng = np.random.default_rng(22)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 10, 5, 1, 1500, related=0.8)
    inp = str(tmp_path / "pairs.txt")
    a.write_input(inp, q, t, mat, 5, 4, 2, 0)
    out = subprocess.run([exe, inp] + (["pool"] if pool else []), check=True, capture_output=True, text=True, timeout=300).stdout
    batch, single, reallocs = a.parse_caller(out)
    exp = a.expected(q, t, mat, 4, 2, 5, which="oracle")
    a.assert_same(batch, exp, "batch")
    a.assert_same(single, exp, "single")
    assert (reallocs is not None and reallocs > len(q)) if pool else reallocs is None
