"""GPU: the deterministic edge grid of tests/ll_edge_util.py on libksw2_amd.so -- the cases of tests/test_local_edges_cpu.py through the
pointer entries under every forced kernel form, through the flat entries from a host and a device arena and, the planted ones, singly
through ksw_ll_i16 and ksw2amd_ll_align -- against the scalar oracle, the contract's formula and the planted cells.  The driver's
four-step prefetch (k2a_ll_task) exists only in the device code: the shape grid's column counts 1..9 and 63..65 over one to three
generations are its test.  Two device-only cases reach the 16-bit column index of the packed form above 32 767."""
import functools
import re
import time

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_edge_util as e
from tests import ll_util as u
from tests import lla_util as la
from tests import llf_util as f

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@functools.lru_cache(maxsize=None)
def _set(name):
    """(set, queries, targets, oracle's (n, 3) array, the contract's dicts); the planted cells are the contract's"""
    s = [x for x in e.sets() if x["name"] == name][0]
    q, t = e.seqs(s)
    exp = u.oracle_batch(q, t, s["mat"], s["go"], s["ge"], s["m"])
    exp_aln = la.expected(q, t, s["mat"], s["go"], s["ge"], s["m"], which="oracle")
    for i, pl in e.planted_dicts(s).items():
        assert (exp_aln[i]["qb"], exp_aln[i]["qe"], exp_aln[i]["tb"], exp_aln[i]["te"]) == pl, s["cases"][i]["name"]
    return s, q, t, exp, exp_aln


def _same_aln(s, got, exp_aln, msg):
    for i, (g, x) in enumerate(zip(got, exp_aln)):
        assert all(g[k] == x[k] for k in la.FIELDS), (msg, s["cases"][i]["name"], {k: g[k] for k in la.FIELDS[:5]}, {k: x[k] for k in la.FIELDS[:5]})
    la.assert_same(got, exp_aln, msg)


def _combos(m):
    return [(form, lds) for form in ("0", "1", "2") for lds in (("0", "1") if m <= 5 else ("1",))]


@pytest.mark.parametrize("name", e.SET_NAMES)
def test_edge_set_pointer_entries(lib, monkeypatch, capfd, name):
    s, q, t, exp, exp_aln = _set(name)
    mat, m, go, ge = s["mat"], s["m"], s["go"], s["ge"]
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form, lds in _combos(m):
        monkeypatch.setenv("KSW2AMD_LL_FORM", form)
        monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
        capfd.readouterr()
        got = lib.ll_batch(q, t, mat, go, ge, m=m)
        err = capfd.readouterr().err
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert len(bad) == 0, (name, form, lds, [(s["cases"][i]["name"], got[i].tolist(), exp[i].tolist()) for i in bad[:4]])
        if mat.max() > 0:
            pk = int(re.search(r"pk_tasks=(\d+)", err).group(1))
            assert (pk == 0) if form == "0" else (pk >= e.twins(s)), (form, err)
            assert ("profile=lds" in err) == (lds == "1"), err
        _same_aln(s, lib.ll_align_batch(q, t, mat, go, ge, m=m), exp_aln, (name, form, lds))


@pytest.mark.parametrize("name", e.SET_NAMES)
def test_edge_set_flat_entries(lib, monkeypatch, name):
    s, q, t, exp, exp_aln = _set(name)
    mat, m, go, ge = s["mat"], s["m"], s["go"], s["ge"]
    arena = f.arena(q, t, lead=3, gap=2)
    d = lib.device_copy(arena[0])
    try:
        for form in ("1", "2"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            for kw in (dict(), dict(device_base=d)):
                got = lib.ll_batch_flat(*arena, mat, go, ge, m=m, **kw)
                bad = np.nonzero((got != exp).any(axis=1))[0]
                assert len(bad) == 0, (name, form, sorted(kw), [(s["cases"][i]["name"], got[i].tolist(), exp[i].tolist()) for i in bad[:4]])
                _same_aln(s, lib.ll_align_batch_flat(*arena, mat, go, ge, m=m, **kw), exp_aln, (name, form, sorted(kw)))
    finally:
        lib.device_free(d)


@pytest.mark.parametrize("name", [n for n in e.SET_NAMES if n.startswith("planted")])
def test_planted_cases_singly(lib, name):
    """every planted case alone through ksw_ll_i16 and ksw2amd_ll_align: an int32 task by itself (no partner to be packed with)"""
    s, q, t, exp, exp_aln = _set(name)
    mat, m, go, ge = s["mat"], s["m"], s["go"], s["ge"]
    ran = 0
    for i, pl in e.planted_dicts(s).items():
        assert lib.ll_i16(q[i], t[i], mat, go, ge, m=m, size=1 + i % 2) == tuple(int(x) for x in exp[i]), s["cases"][i]["name"]
        r = lib.ll_align(q[i], t[i], mat, go, ge, m=m)
        assert all(r[k] == exp_aln[i][k] for k in la.FIELDS), (s["cases"][i]["name"], r, exp_aln[i])
        assert (r["qb"], r["qe"], r["tb"], r["te"]) == pl
        ran += 1
    assert ran == len(s["cases"])          # every case of a planted set is planted: none left out


@pytest.mark.parametrize("form", ["1", "2"])
def test_packed_saturation_point(lib, monkeypatch, capfd, form):
    """(min + 1) * smax <= 65535 at equality: smax = 85, length 770 -- best 65 450, H + smax = 65 535 -- is packed and exact; 771 goes
    to int32.  The same at smax = 127 with every mismatch at pen = 255 (515 / 516)."""
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    for tag, mat, n, packed in e.saturation_cases():
        q, t = e.saturation_pair(n)
        exp = u.oracle_batch(q, t, mat, 5, 1)
        assert exp[0].tolist() == [int(mat.max()) * n, n - 1, n - 1]
        for lds in ("0", "1"):
            monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
            capfd.readouterr()
            got = lib.ll_batch(q, t, mat, 5, 1)
            err = capfd.readouterr().err
            np.testing.assert_array_equal(got, exp, err_msg=str((tag, n, lds)))
            assert ("pk_tasks=1 " in err) == packed, (tag, n, err)
            assert ("pk_tasks=0 " in err) == (not packed), (tag, n, err)
            _same = la.expected(q, t, mat, 5, 1, 4, which="oracle")
            la.assert_same(lib.ll_align_batch(q, t, mat, 5, 1), _same, (tag, n, lds))


def test_column_index_above_15_bits_identical_pair(lib, monkeypatch, capfd):
    """smax = 1, an identical pair of 65 534 x 65 534 in the packed form (form 2 packs the single pair): (65 534 + 1) * 1 = 65 535 is the
    last admissible length, the best cell is (65 533, 65 533) with score 65 534, so H + smax = 65 535 and the row maximum's u16 column
    runs through every value above 32 767 -- in the forward pass and, the alignment spanning both sequences, in the start-cell pass.
    ksw2amd_ll_align_batch runs with KSW_EZ_SCORE_ONLY: the subject is the two kernels' column index, and the CIGAR stage would be an
    unbanded 65 534 x 65 534 traceback.  The oracle is the scalar C one: 4.3e9 cells per direction, measured at 12 to 21 s forward and as much
    on the reversed prefixes on one host core, by the machine (printed again by the test)."""
    n = 65534
    mat = u.simple_mat(4, 1, 1)
    x = np.random.default_rng(65534).integers(0, 4, n, dtype=np.uint8)
    t0 = time.time()
    exp = u.oracle_batch([x], [x], mat, 1, 1, 4)
    t1 = time.time()
    cells = la.start_cells([x], [x], mat, 1, 1, 4, fwd=exp)
    with capfd.disabled():
        print("scalar oracle: forward %.1f s, reversed prefixes %.1f s" % (t1 - t0, time.time() - t1))
    assert exp[0].tolist() == [n, n - 1, n - 1] and cells[0].tolist() == [n, 0, n - 1, 0, n - 1, n]
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    for lds in ("0", "1"):
        monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
        capfd.readouterr()
        got = lib.ll_batch([x], [x], mat, 1, 1)
        err = capfd.readouterr().err
        assert "pk_tasks=1 int32_tasks=0" in err, err
        assert got.tolist() == exp.tolist(), lds
        a = lib.ll_align_batch([x], [x], mat, 1, 1, flag=la.SCORE_ONLY)[0]
        assert (a["score"], a["qb"], a["qe"], a["tb"], a["te"], a["n_cigar"]) == (n, 0, n - 1, 0, n - 1, 0), (lds, a)


def test_column_index_above_15_bits_planted_core(lib, monkeypatch, capfd):
    """smax = 1, 33 000 x 40 000 in either orientation, packed (form 2): a planted core of 300 residues that ends in column 32 899, so
    the winning row's u16 column has its top bit set and the rows before it do not.  The oracle is the scalar C one: 1.3e9 cells per
    pair and direction, measured at 14 to 25 s for the two pairs, both directions, on one host core (printed again by the test)."""
    mat = u.simple_mat(4, 1, 3)
    core = np.random.default_rng(33000).integers(2, 4, 300, dtype=np.uint8)
    cases = [e.plant("u16-core", mat, 4, 2, 1, sw, 40000, 33000, 39000 + 50 * sw, 32600, core) for sw in (0, 1)]
    q, t = [c["q"] for c in cases], [c["t"] for c in cases]
    t0 = time.time()
    exp = u.oracle_batch(q, t, mat, 2, 1, 4)
    cells = la.start_cells(q, t, mat, 2, 1, 4, fwd=exp)
    with capfd.disabled():
        print("scalar oracle: forward and reversed prefixes of both pairs %.1f s" % (time.time() - t0))
    for c, x in zip(cases, cells.tolist()):
        assert tuple(x[1:5]) == c["planted"] and x[0] == x[5] == 300, (c["name"], x)
        assert min(c["planted"][1], c["planted"][3]) == 32899
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    for lds in ("0", "1"):
        monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
        capfd.readouterr()
        got = lib.ll_batch(q, t, mat, 2, 1)
        err = capfd.readouterr().err
        assert "pk_tasks=2 int32_tasks=0" in err, err
        assert got.tolist() == exp.tolist(), lds
        for a, c in zip(lib.ll_align_batch(q, t, mat, 2, 1), cases):
            assert (a["score"], a["qb"], a["qe"], a["tb"], a["te"]) == (300,) + c["planted"], (lds, a)
            assert a["cigar"] == [300 << 4], (lds, a)
