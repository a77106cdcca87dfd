"""CPU: the deterministic edge grid of tests/ll_edge_util.py -- generation and strip seams, planted end and start cells, asymmetric
matrices at m = 1, 3, 4, 5, 6 and 127, the packed format's saturation point -- through ksw2amd_ll_batch, ksw2amd_ll_align_batch and the
flat entries on one simulator build (tests/llf_util.py: the product's host objects against the lock-step twins of the kernels), under
every forced kernel form and score lookup, against the scalar oracle, the contract's formula and the planted cells."""
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_edge_util as e
from tests import ll_util as u
from tests import lla_util as la
from tests import llf_util as f


@pytest.fixture(scope="module")
def sim():
    return ksw2_amd.Library(f.sim_library())       # the one build of this module: ll, lla and llf host objects and all three twins


def _combos(m):
    """(form, lds) switches: every form; both score lookups where the register profile exists (m <= 5: above it KSW2AMD_LL_LDS is moot)"""
    return [(form, lds) for form in ("0", "1", "2") for lds in (("0", "1") if m <= 5 else ("1",))]


def test_generator_covers_the_seams():
    """What the grid claims to hit, read back from the generated cases (sets() has already asserted that the scalar oracle returns the
    planted cells of every planted case).  Both orientations each."""
    sets = e.sets()
    assert [s["name"] for s in sets] == list(e.SET_NAMES)
    for name, seams, whole in (("planted-m5", e.SEAM_ROWS, True), ("planted-m6", (16, 1024), False), ("planted-m3", (16, 1024), False),
                               ("planted-m4", (16, 1024), False)):
        cases = [c for s in sets if s["name"] == name for c in s["cases"]]
        for sw in (0, 1):
            mine = [c for c in cases if c["name"].endswith("/sw%d" % sw) and "rows_end" in c]
            assert all((len(c["q"]) > len(c["t"])) == bool(sw) for c in mine)
            ends, spans = {c["rows_end"] for c in mine}, {c["rows_end"] - c["rows_start"] for c in mine}
            assert set(seams) <= ends and set(seams if whole else (16,)) <= spans, (name, sw)    # spans: the end row of the REV pass
            last = [c for c in mine if c["rows_end"] == max(len(c["q"]), len(c["t"])) - 1]
            assert any(c["planted"][1] == len(c["q"]) - 1 and c["planted"][3] == len(c["t"]) - 1 for c in last)
            assert any(min(c["planted"][1], c["planted"][3]) == 0 for c in mine)          # the end cell in column 0
            assert any(c["name"].startswith("vgap-row1023/") for c in mine) and any(c["name"].startswith("hgap-row1023/") for c in mine)
            if whole:
                assert any(c["name"].startswith("vgap-row15/") for c in mine) and any(c["name"].startswith("hgap-row15/") for c in mine)
                assert any(c["rows_start"] < 1024 and c["rows_end"] >= 2048 for c in mine)    # three generations
    grid = [c["name"] for s in sets if s["name"] == "grid-m5" for c in s["cases"]]
    for rows in e.GRID_ROWS:
        for cols in e.GRID_COLS:
            if cols <= rows:
                assert sum(n.startswith("grid-%dx%d/" % (rows, cols)) for n in grid) >= 2
    assert any("grid-1025x65/sw0" in n for n in grid) and any("grid-1025x65/sw1" in n for n in grid)


@pytest.mark.parametrize("name", e.SET_NAMES)
def test_edge_set_every_form(sim, monkeypatch, capfd, name):
    s = [x for x in e.sets() if x["name"] == name][0]
    q, t = e.seqs(s)
    mat, m, go, ge = s["mat"], s["m"], s["go"], s["ge"]
    exp = u.oracle_batch(q, t, mat, go, ge, m)
    exp_aln = la.expected(q, t, mat, go, ge, m, which="oracle")
    for i, pl in e.planted_dicts(s).items():
        assert (exp_aln[i]["qb"], exp_aln[i]["qe"], exp_aln[i]["tb"], exp_aln[i]["te"]) == pl, s["cases"][i]["name"]
    arena = f.arena(q, t, lead=3, gap=2)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    ran = 0
    for form, lds in _combos(m):
        monkeypatch.setenv("KSW2AMD_LL_FORM", form)
        monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
        capfd.readouterr()
        got = sim.ll_batch(q, t, mat, go, ge, m=m)
        err = capfd.readouterr().err
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert len(bad) == 0, (name, form, lds, [(s["cases"][i]["name"], got[i].tolist(), exp[i].tolist()) for i in bad[:4]])
        if mat.max() > 0:
            pk = int(re.search(r"pk_tasks=(\d+)", err).group(1))
            assert (pk == 0) if form == "0" else (pk >= e.twins(s)), (form, err)
            assert ("profile=lds" in err) == (lds == "1"), err
        aln = sim.ll_align_batch(q, t, mat, go, ge, m=m)
        for i, (g, x) in enumerate(zip(aln, exp_aln)):
            assert all(g[k] == x[k] for k in la.FIELDS), (name, form, lds, s["cases"][i]["name"], {k: g[k] for k in la.FIELDS[:5]},
                                                          {k: x[k] for k in la.FIELDS[:5]})
        la.assert_same(aln, exp_aln, (name, form, lds))
        ran += len(q)
    assert ran == len(s["cases"]) * len(_combos(m))          # no case of the set left out
    # the flat entries from a host arena, in the form the library picks by itself
    monkeypatch.delenv("KSW2AMD_LL_FORM")
    monkeypatch.delenv("KSW2AMD_LL_LDS")
    assert (sim.ll_batch_flat(*arena, mat, go, ge, m=m) == exp).all(), (name, "flat")
    la.assert_same(sim.ll_align_batch_flat(*arena, mat, go, ge, m=m), exp_aln, (name, "flat"))


@pytest.mark.parametrize("form", ["1", "2"])
def test_packed_saturation_point(sim, monkeypatch, capfd, form):
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
            got = sim.ll_batch(q, t, mat, 5, 1)
            err = capfd.readouterr().err
            np.testing.assert_array_equal(got, exp, err_msg=str((tag, n, lds)))
            assert ("pk_tasks=1 " in err) == packed, (tag, n, err)
            assert ("pk_tasks=0 " in err) == (not packed), (tag, n, err)
            aln = sim.ll_align_batch(q, t, mat, 5, 1, flag=la.SCORE_ONLY)
            assert [(a["score"], a["qb"], a["qe"], a["tb"], a["te"]) for a in aln] == [(int(exp[0][0]), 0, n - 1, 0, n - 1)] * 2


@pytest.mark.parametrize("m", [3, 4, 5])
def test_asymmetric_oracle_pinned_by_brute_force(sim, m):
    """The scalar oracle reads mat[t * m + q], not its transpose, at m <= 5: brute force on pairs of <= 12 residues, the longer sequence
    the query and the target in turn.  The simulator build agrees in both orientations."""
    rng = np.random.default_rng(300 + m)
    differ = 0
    for mixed in (False, True):
        mat = e.asym_mat(m, mixed)
        tr = np.ascontiguousarray(mat.reshape(m, m).T).reshape(-1)
        for k in range(120):
            a = rng.integers(0, m, int(rng.integers(1, 13)), dtype=np.uint8)
            b = u.mutate(rng, a, m, 0.15, 0.1)[:12] if k % 2 else rng.integers(0, m, int(rng.integers(1, 13)), dtype=np.uint8)
            go, ge = [(4, 2), (0, 1), (1, 1)][k % 3]
            for q, t in ((a, b), (b, a)):
                want = u.brute(q, t, mat, go, ge, m)
                assert tuple(int(x) for x in u.oracle_batch([q], [t], mat, go, ge, m)[0]) == want, (q, t, go, ge)
                assert tuple(int(x) for x in sim.ll_batch([q], [t], mat, go, ge, m=m)[0]) == want, (q, t, go, ge)
                differ += want != u.brute(q, t, tr, go, ge, m)
    assert differ >= 20           # ... and the transposed matrix gives another answer on these pairs: it would have been noticed


def test_packed_helpers_and_profile_bytes(tmp_path):
    """tests/llsim/ll_ops_check.cpp: the host twins of the saturating packed helpers against their plain definitions at the 16-bit
    limits, and no byte past the alphabet in the register column profile at m = 1 .. 5 -- what no admitted input can reach."""
    exe = str(tmp_path / "ll_ops_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-o", exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "llsim", "ll_ops_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
