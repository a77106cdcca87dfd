"""CPU: local alignment with start cell and CIGAR (ksw2amd_ll_align_batch / ksw2amd_ll_align; include/ksw2_amd.h).
The contract's formula is pinned to the compiled reference's scalar ksw_extz and to a brute-force check of the start-cell tie rule; the
product's host code and lane code (the REV form of ksw2_lane_ll.h, both kernel forms and both score lookups) run on a test-local
lock-step simulator build against that formula; a C caller compiled against include/ksw2_amd.h prints the formula's answers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import lla_util as a
from tests.test_local_cpu import _pin_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ksw2amd_ll_align_batch", "ksw2amd_ll_align")


@pytest.fixture(scope="module")
def sim():
    return ksw2_amd.Library(a.sim_library())


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)                    # every mismatch costs: planted matches stay where they were put
    np.fill_diagonal(mat, 2)
    return mat.reshape(-1)


def test_contract_pinned_to_reference(sim):
    """Over the four parameter sets of the forward pin test: the reversed-prefix local score equals the forward score; the reference's
    global ksw_extz on the interval scores exactly `score`; its CIGAR re-scores to `score`, consumes both intervals exactly and begins
    and ends with M when a gap costs something.  The library (simulator build) returns the same coordinates and CIGARs."""
    if not a.have_ref():
        pytest.skip("oracle/_ref/libksw2ref.so not built (build() makes it where the reference's sources exist)")
    rng = np.random.default_rng(11)
    total = 0
    for q, t, mat, m, go, ge in _pin_sets(rng):
        exp = a.expected(q, t, mat, go, ge, m, which="ref")
        a.assert_same(sim.ll_align_batch(q, t, mat, go, ge, m=m), exp, (m, go, ge))
        for i, e in enumerate(exp):
            total += 1
            if e["score"] == 0:
                assert (e["qb"], e["qe"], e["tb"], e["te"], e["n_cigar"]) == (-1, -1, -1, -1, 0)
                continue
            assert e["rscore"] == e["score"] and e["gscore"] == e["score"], (i, e)
            qi, ti = q[i][e["qb"]:e["qe"] + 1], t[i][e["tb"]:e["te"] + 1]
            assert a.rescore(e["cigar"], qi, ti, mat, m, go, ge) == (e["score"], len(qi), len(ti)), (i, e)
            if go + ge > 0:
                assert e["cigar"][0] & 0xf == 0 and e["cigar"][-1] & 0xf == 0, (i, e)
    assert total >= 2000


def test_start_cell_tie_rule_brute_force(sim):
    """Tiny two-letter pairs with many equal optima: among the (qb, tb) whose sub-rectangle's global score equals the local score, the
    contract -- and the library (simulator build) -- picks the largest tb, then the largest qb."""
    rng = np.random.default_rng(5)
    mat = u.simple_mat(2, 1, 1)
    qs, ts, gaps, exp = [], [], [], []
    for k in range(320):
        q = rng.integers(0, 2, int(rng.integers(1, 8)), dtype=np.uint8)
        t = np.tile(q, 2) if k % 3 == 0 else rng.integers(0, 2, int(rng.integers(1, 8)), dtype=np.uint8)
        go, ge = [(1, 1), (0, 1), (0, 0), (2, 0)][k % 4]
        b = a.brute_start(q, t, mat, 2, go, ge)
        assert tuple(int(x) for x in a.start_cells([q], [t], mat, go, ge, 2)[0][:5]) == b, (q, t, go, ge)
        qs.append(q); ts.append(t); gaps.append((go, ge)); exp.append(b)
    for g in set(gaps):
        idx = [i for i in range(len(qs)) if gaps[i] == g]
        got = sim.ll_align_batch([qs[i] for i in idx], [ts[i] for i in idx], mat, g[0], g[1], flag=a.SCORE_ONLY, m=2)
        for i, r in zip(idx, got):
            assert (r["score"], r["qb"], r["qe"], r["tb"], r["te"]) == exp[i], (qs[i], ts[i], g)


@pytest.mark.parametrize("m", [5, 20])
def test_sim_pipeline_every_forced_form(sim, monkeypatch, capfd, m):
    rng = np.random.default_rng(200 + m)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else _m20(rng)
    go, ge = (4, 2) if m == 5 else (6, 1)
    q, t = a.new_ground(rng, m)
    exp = a.expected(q, t, mat, go, ge, m)
    # the inputs do what they are chosen for: distant end cells in same-shape neighbours, a zero beside a positive score, cell (0, 0), full span
    assert any(exp[i]["te"] < 60 and exp[i + 1]["te"] > 2000 for i in range(0, 16, 2)) and any(exp[i]["te"] > 2000 and exp[i + 1]["te"] < 60 for i in range(0, 16, 2))
    assert any(exp[i]["qe"] > 2000 for i in range(16)) and exp[16]["score"] == 0 and exp[17]["score"] > 0
    assert (exp[18]["qe"], exp[18]["te"]) == (0, 0) and (exp[20]["qb"], exp[20]["qe"], exp[20]["tb"], exp[20]["te"]) == (0, 179, 0, 179)
    fwd = u.oracle_batch(q, t, mat, go, ge, m)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form in ("0", "1", "2"):
        for lds in ("0", "1"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
            capfd.readouterr()
            got = sim.ll_align_batch(q, t, mat, go, ge, m=m)
            err = capfd.readouterr().err
            a.assert_same(got, exp, (form, lds))
            np.testing.assert_array_equal(np.array([[r["score"], r["qe"], r["te"]] for r in got]), fwd)
            np.testing.assert_array_equal(sim.ll_batch(q, t, mat, go, ge, m=m), fwd)
            line = re.search(r"ll-rev: pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+)", err)
            assert line, err
            assert (int(line.group(1)) == 0) if form == "0" else (int(line.group(1)) >= 12), (form, err)       # the packed reverse form really ran
            assert line.group(3) == ("lds" if lds == "1" or m > 5 else "registers"), err
    # single-call entry = batch entry
    for i in (0, 1, 9, 16, 17, 18, 20, 23):
        r = sim.ll_align(q[i], t[i], mat, go, ge, m=m)
        assert all(r[f] == exp[i][f] for f in a.FIELDS), (i, r, exp[i])


def test_sim_corners_of_the_argument_range(sim):
    """gapo = gape = 0, m > 5 with an arbitrary matrix, m = 127, gap costs of 127: every stage is exact (the CIGAR stage's kernels included)."""
    rng = np.random.default_rng(77)
    for m, go, ge, lo, hi in ((5, 0, 0, -4, 3), (20, 0, 0, -6, 7), (127, 3, 1, -128, 128), (127, 127, 127, -20, 127), (11, 127, 0, -9, 9), (3, 0, 127, -2, 3)):
        mat = u.random_mat(rng, m, lo, hi)
        q, t = u.ragged(rng, 40, m, 1, 90, related=0.6)
        a.assert_same(sim.ll_align_batch(q, t, mat, go, ge, m=m), a.expected(q, t, mat, go, ge, m), (m, go, ge))


def test_sim_flags(sim):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 60, 5, 1, 300, related=0.8)
    q += [np.tile(np.array([0, 1], np.uint8), 30)] * 4                       # gaps whose placement RIGHT changes
    t += [np.concatenate([np.tile(np.array([0, 1], np.uint8), 20), [0, 0], np.tile(np.array([0, 1], np.uint8), 20)]).astype(np.uint8)] * 4
    base = a.expected(q, t, mat, 4, 2, 5)
    differs = 0
    for flag in (0, a.RIGHT, a.REV_CIGAR, a.RIGHT | a.REV_CIGAR, a.SCORE_ONLY, a.SCORE_ONLY | a.RIGHT):
        exp = a.expected(q, t, mat, 4, 2, 5, flag)
        got = sim.ll_align_batch(q, t, mat, 4, 2, flag=flag, m=5)
        a.assert_same(got, exp, flag)
        for g, b in zip(got, base):
            assert all(g[f] == b[f] for f in ("score", "qb", "qe", "tb", "te"))          # flags never move the coordinates
            if flag & a.SCORE_ONLY:
                assert g["n_cigar"] == 0 and g["cigar"] == []
            differs += g["cigar"] != b["cigar"] and not flag & a.SCORE_ONLY
    assert differs > 0


def _raw(sim, q, t, mat, go, ge, flag, aln, m=5, km=None):
    keep = [np.ascontiguousarray(x, dtype=np.uint8) for x in list(q) + list(t)]
    n = len(q)
    pairs = (ksw2_amd.LocalPair * max(n, 1))()
    for i in range(n):
        pairs[i].query, pairs[i].target = keep[i].ctypes.data, keep[n + i].ctypes.data
        pairs[i].qlen, pairs[i].tlen = len(keep[i]), len(keep[n + i])
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    return sim.lib.ksw2amd_ll_align_batch(km, m, mat.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), go, ge, flag, n, pairs, aln), pairs


def test_sim_bad_arguments_and_degenerate_batches(sim, monkeypatch, capfd):
    mat = u.simple_mat(5, 2, 4, -1)
    x = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for kw in (dict(flag=0x40), dict(flag=0x800), dict(flag=0x04), dict(t=[np.array([0, 5], np.uint8)]), dict(go=128), dict(ge=-1)):
        capfd.readouterr()
        with pytest.raises(ksw2_amd.Ksw2Error, match="error -2"):
            sim.ll_align_batch([x], kw.get("t", [x]), mat, kw.get("go", 4), kw.get("ge", 2), flag=kw.get("flag", 0))
        err = capfd.readouterr().err
        assert "ll:" not in err and "ll-rev:" not in err                      # no trace line: nothing was staged
    # a NULL sequence with a positive length
    aln = (ksw2_amd.LocalAln * 1)()
    pairs = (ksw2_amd.LocalPair * 1)()
    pairs[0].query, pairs[0].target, pairs[0].qlen, pairs[0].tlen = None, x.ctypes.data, 3, 6
    capfd.readouterr()
    assert sim.lib.ksw2amd_ll_align_batch(None, 5, mat.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), 4, 2, 0, 1, pairs, aln) == -2
    assert "ll:" not in capfd.readouterr().err
    assert sim.ll_align_batch([], [], mat, 4, 2) == []
    r = sim.ll_align_batch([x, np.zeros(0, np.uint8)], [x, x], -np.abs(mat), 4, 2)                 # no positive entry / an empty query
    assert all((d["score"], d["qb"], d["qe"], d["tb"], d["te"], d["n_cigar"]) == (0, -1, -1, -1, -1, 0) for d in r)
    r = sim.ll_align_batch([np.zeros(0, np.uint8), x], [x, x], mat, 4, 2)
    assert r[0]["score"] == 0 and r[0]["qb"] == -1 and r[1] ["score"] == 12 and r[1]["cigar"] == [6 << 4]


def test_sim_cigar_buffer_reuse(sim):
    """A second call into the same records must not reallocate a buffer that is large enough."""
    rng = np.random.default_rng(41)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 40, 200, related=1.0)
    exp = a.expected(q, t, mat, 4, 2, 5)
    aln = (ksw2_amd.LocalAln * len(q))()
    rc, _ = _raw(sim, q, t, mat, 4, 2, 0, aln)
    assert rc == 0
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    assert all(p and mc >= x.n_cigar > 0 for (p, mc), x in zip(first, aln))
    rc, _ = _raw(sim, q[::-1], t[::-1], mat, 4, 2, 0, aln)                   # other alignments into the same buffers
    assert rc == 0
    for k, x in enumerate(aln):
        e = exp[len(q) - 1 - k]
        assert [int(x.cigar[j]) for j in range(x.n_cigar)] == e["cigar"] and x.score == e["score"]
        if x.n_cigar <= first[k][1]:
            assert (ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) == first[k]
    rc, _ = _raw(sim, q[::-1], t[::-1], mat, 4, 2, a.SCORE_ONLY, aln)        # score only: buffers kept, no CIGAR
    assert rc == 0 and all(x.n_cigar == 0 and x.m_cigar > 0 for x in aln)
    for x in aln:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ksw2_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ksw2_amd.EXPORTS
    assert "ksw2amd_laln_t" in src
    if not os.path.exists(ksw2_amd.DEFAULT_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ksw2_amd", "csrc")], check=True, capture_output=True)
    lib = ctypes.CDLL(ksw2_amd.DEFAULT_SO)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert ctypes.sizeof(ksw2_amd.LocalAln) == 40 and ksw2_amd.LocalAln.cigar.offset == 32


@pytest.mark.parametrize("pool", [False, True])
def test_c_caller_with_and_without_pool(tmp_path, pool):
    so = a.sim_library(str(tmp_path / "libksw2_amd.so"))
    exe = str(tmp_path / "lla_caller")
    subprocess.run(["gcc", "-O1", "-Wall", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "lla_caller.c"), "-L" + str(tmp_path), "-lksw2_amd", "-Wl,-rpath," + str(tmp_path)], check=True)
    assert os.path.exists(so)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 14, 5, 1, 500, related=0.8)
    q.append(np.zeros(3, np.uint8)); t.append(np.ones(4, np.uint8))          # a score of 0 among them
    for flag in (0, a.RIGHT | a.REV_CIGAR):
        inp = str(tmp_path / "pairs.txt")
        a.write_input(inp, q, t, mat, 5, 4, 2, flag)
        out = subprocess.run([exe, inp] + (["pool"] if pool else []), check=True, capture_output=True, text=True).stdout
        batch, single, reallocs = a.parse_caller(out)
        exp = a.expected(q, t, mat, 4, 2, 5, flag)
        a.assert_same(batch, exp, "batch")
        a.assert_same(single, exp, "single")
        assert (reallocs is not None and reallocs > len(q)) if pool else reallocs is None      # profiles and CIGARs really came from the pool
