"""CPU: the suboptimal local score under the two-piece gap cost and the two-piece single-pair entries (ksw2amd_lld_sub_batch / _flat,
ksw2amd_lld, ksw2amd_lld_align, ksw2amd_lld_sub; include/ksw2_amd.h).  The test oracle (tests/llds_oracle.c) is
pinned to a brute-force statement of the definition, to the two oracles it combines (tests/lld_oracle.c, tests/lls_oracle.c) and to the
compiled reference's scalar ksw_extd; the product's host code and lane code (K2aLaneLL<.., SUB = true, DUAL = true> and the reduction of
ksw2_lane_llsub.h) run on a test-local lock-step simulator build against that oracle over the grid of tests/llds_util.py, in every
(form, lookup) combination; a C caller compiled against include/ksw2_amd.h prints the oracle's numbers."""
import contextlib
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import lla_util as la
from tests import lld_util as d
from tests import lls_util as s
from tests import llds_util as x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ksw2amd_lld_sub_batch", "ksw2amd_lld_sub_batch_flat", "ksw2amd_lld", "ksw2amd_lld_align", "ksw2amd_lld_sub")
EXTZ_ONLY = 0x40


@pytest.fixture(scope="module")
def sim_so(tmp_path_factory):
    return x.sim_library(str(tmp_path_factory.mktemp("lldssim") / "libksw2_amd.so"))


@pytest.fixture(scope="module")
def sim(sim_so):
    return ksw2_amd.Library(sim_so)


@pytest.fixture(autouse=True)
def _env():
    keys = ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS", "KSW2AMD_TRACE")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _all_launches(sim):
    return sum(x.launches(sim)[:2])


# ---------------------------------------------------------------- the oracle itself

COST_SETS = ((4, 2, 24, 1), (1, 1, 3, 0), (0, 0, 0, 0), (127, 127, 127, 127), (3, 2, 1, 1), (6, 3, 2, 1), (2, 1, 2, 1), (5, 1, 0, 3))


def _tiny(rng, k):
    """pairs of at most 40 x 40 over two or three letters: repeats (ties), a query twice in its target, random strings"""
    a = 2 + k % 2
    q = rng.integers(0, a, int(rng.integers(1, 13)), dtype=np.uint8)
    if k % 4 == 0:
        return q, np.tile(q, 3)[:40]
    if k % 4 == 1:
        return q, np.concatenate([q, rng.integers(0, a, int(rng.integers(1, 15)), dtype=np.uint8), q])[:40]
    return q, rng.integers(0, a, int(rng.integers(1, 41)), dtype=np.uint8)


def test_oracle_is_the_definition_brute_force(sim):
    """tests/llds_oracle.c against every cell's H in plain Python with unclamped gap states, the tie rules on the sets of maxima and the
    window, over all-zero costs, all 127 and a second piece that is cheaper everywhere; the library (simulator build) returns the same"""
    rng = np.random.default_rng(5)
    mat = np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)
    total = 0
    for ci, costs in enumerate(COST_SETS):
        for excl in (-1, 0, 1, 3):
            qs, ts = zip(*[_tiny(rng, k) for k in range(8)])
            exp = np.array([x.brute(q, t, mat, costs, 3, excl) for q, t in zip(qs, ts)], dtype=np.int32)
            np.testing.assert_array_equal(x.oracle_batch(qs, ts, mat, costs, excl, 3), exp, str((costs, excl)))
            os.environ["KSW2AMD_LL_FORM"] = str((ci + excl) % 3)
            res, sub = sim.lld_sub_batch(list(qs), list(ts), mat, *costs, excl=excl, m=3)
            np.testing.assert_array_equal(np.hstack([res, sub]), exp, str((costs, excl)))
            total += len(qs)
    assert total >= 200


def test_oracle_equals_the_oracles_it_combines():
    """(score, qe, te) is tests/lld_oracle.c's; with equal pieces, or a second piece that never pays, all six values are tests/lls_oracle.c's"""
    rng = np.random.default_rng(8)
    for m, mat in ((5, x.M5), (20, u.random_mat(rng, 20))):
        q, t = u.ragged(rng, 120, m, 1, 160, related=0.6)
        for costs in (x.CROSS, x.CHEAP2, (0, 0, 0, 0), (0, 2, 3, 1)):
            for excl in (-1, 4):
                np.testing.assert_array_equal(x.oracle_batch(q, t, mat, costs, excl, m)[:, :3], d.oracle_batch(q, t, mat, costs, m))
        for excl in (-1, 0, 9):
            exp = s.oracle_batch(q, t, mat, 4, 2, excl, m)
            for go2, ge2 in ((4, 2), (4, 3), (9, 2), (127, 127)):
                np.testing.assert_array_equal(x.oracle_batch(q, t, mat, (4, 2, go2, ge2), excl, m), exp)


def test_oracle_pinned_to_reference_extd():
    """For the oracle's (score2, qe2, te2) with score2 > 0: the reference's scalar ksw_extd on reverse(query[0..qe2]), reverse(target[0..te2])
    (extension only, unbanded, no Z-drop) reaches a max equal to score2"""
    if not la.have_ref():
        pytest.skip("oracle/_ref/libksw2ref.so not built (build() makes it where the reference's sources exist)")
    from oracle import pyoracle as po
    rng = np.random.default_rng(12)
    total = 0
    for q, t, mat, m, costs in x.pin_sets(rng):
        exp = x.oracle_batch(q, t, mat, costs, -1, m)
        for i in range(len(q)):
            s2, qe2, te2 = map(int, exp[i, 3:])
            if s2 == 0:
                assert qe2 == -1 and te2 == -1
                continue
            total += 1
            r = po.align("ref", "extd", q[i][:qe2 + 1][::-1], t[i][:te2 + 1][::-1], mat, *costs, w=-1, zdrop=-1, flag=EXTZ_ONLY, m=m)
            assert r["max"] == s2, (costs, i, r["max"], exp[i])
    assert total >= 1200, total


# ---------------------------------------------------------------- header, ABI

def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ksw2_amd.h")).read(), flags=re.S)
    if not os.path.exists(ksw2_amd.DEFAULT_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ksw2_amd", "csrc")], check=True, capture_output=True)
    lib = ctypes.CDLL(ksw2_amd.DEFAULT_SO)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ksw2_amd.EXPORTS
        assert hasattr(lib, name), name
    for name in ("lld_sub_batch", "lld_sub_batch_flat", "lld", "lld_align", "lld_sub"):
        assert callable(getattr(ksw2_amd.Library, name))
    # only ksw2_host_llds.o names the new launch: the older simulator builds keep linking
    for obj in ("ll", "lla", "llf", "lls", "lld"):
        o = os.path.join(ROOT, "ksw2_amd", "csrc", "ksw2_host_%s.o" % obj)
        if os.path.exists(o):
            assert "k2a_shim_launch_lld_sub" not in subprocess.run(["nm", "-u", o], capture_output=True, text=True, check=True).stdout, obj


# ---------------------------------------------------------------- the simulator twin through the five entries, over the grid

def test_sim_item1_generation_boundary(sim, monkeypatch, capfd):
    x.check_boundary(sim, monkeypatch, capfd)


def test_sim_item2_window_follows_the_two_piece_score(sim, monkeypatch):
    x.check_window(sim, monkeypatch)


def test_sim_item3_shoulder(sim, monkeypatch):
    x.check_shoulder(sim, monkeypatch)


@pytest.mark.parametrize("name", ["generation_edges", "window_edges", "differing_halves", "tandem_repeats", "forced_orientation", "wide_score", "wide_query"])
def test_sim_item4_and_6_edge_grid(sim, monkeypatch, name):
    x.check_grid4(sim, monkeypatch, name)


def test_sim_item5_shape_grid(sim, monkeypatch):
    x.check_shape_grid(sim, monkeypatch)


def test_sim_item7_single_pair_entries(sim):
    x.check_single(sim)


def test_sim_trace_lines(sim, monkeypatch, capfd):
    """lld: then lld-sub:, the task split of every form, pk_profile=lds where packed tasks were asked for the register profile"""
    rng = np.random.default_rng(304)
    q, t = s.differing_halves(rng)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for m, mat, qq, tt in ((5, x.M5, q, t), (20, u.random_mat(rng, 20), *s.differing_halves(rng, 20))):
        for form, lds in x.forms(monkeypatch, m):
            capfd.readouterr()
            sim.lld_sub_batch(qq, tt, mat, *x.CROSS, excl=11, m=m)
            pk, i32, excl = x.trace_line(capfd.readouterr().err, m, lds)
            assert (pk, i32, excl) == {"0": (0, 7), "1": (3, 1), "2": (4, 0)}[form] + (11,)
    capfd.readouterr()
    sim.lld_sub_batch_flat(*x.lf.arena(q, t), x.M5, *x.CROSS)
    err = capfd.readouterr().err
    assert "arena=host" in err and x.trace_line(err, 5, "0")[2] == -1


@pytest.mark.parametrize("costs", [x.CROSS, x.CHEAP2, (0, 0, 0, 0)])
def test_sim_ragged_parity(sim, monkeypatch, costs):
    """the ragged sets of the GPU tier, thinned to what a lock-step simulator runs in seconds"""
    x.check_ragged(sim, costs, small=True, monkeypatch=monkeypatch)


@contextlib.contextmanager
def _placed(lib, base, kind):
    """the simulator's "device" arena is host memory used in place"""
    yield dict(device_base=base.ctypes.data) if kind == "device" else dict()


def test_sim_flat_entries(sim, monkeypatch):
    x.launches(sim, reset=True)
    x.check_flat(sim, _placed, ["host", "device"], monkeypatch, launches_fn=lambda: _all_launches(sim))
    n_new, n_other, n_chk = x.launches(sim)
    assert n_new > 0 and n_other == 0 and n_chk > 0      # nothing but the new launch and the check ran


def test_sim_bad_arguments_launch_nothing(sim):
    x.launches(sim, reset=True)
    x.check_bad_arguments(sim, ksw2_amd.Ksw2Error, launches_fn=lambda: _all_launches(sim))
    assert x.launches(sim)[:2] == (0, 0)


def test_sim_c_caller_public_header(sim_so, tmp_path):
    x.check_c_caller(os.path.dirname(sim_so), "ksw2_amd", tmp_path)


def test_golden_vectors_match_the_oracle(sim):
    sets, gen = x.load_golden(), x.golden_inputs()
    assert len(sets) == len(gen) and os.path.getsize(x.GOLDEN) < 100000
    for (q, t, mat, m, costs, excl, exp), g in zip(sets, gen):
        assert m == g[3] and costs == tuple(g[4]) and excl == g[5] and (np.asarray(mat) == g[2]).all()
        assert all((a == b).all() for a, b in zip(q + t, list(g[0]) + list(g[1])))
        np.testing.assert_array_equal(x.oracle_batch(q, t, mat, costs, excl, m), exp)
        res, sub = sim.lld_sub_batch(q, t, mat, *costs, excl=excl, m=m)
        np.testing.assert_array_equal(np.hstack([res, sub]), exp)
