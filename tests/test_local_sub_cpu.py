"""CPU: the suboptimal local score (ksw2amd_ll_sub_batch / _flat / ksw2amd_ll_sub; include/ksw2_amd.h).  The test
oracle (tests/lls_oracle.c) is pinned to the compiled reference's scalar ksw_extz and to a pure-Python statement of the definition; the
product's host code and both lane headers (ksw2_lane_ll.h with SUB, ksw2_lane_llsub.h) run on a test-local lock-step simulator build
against that oracle over the edge grid of tests/lls_util.py, in every (form, lookup) combination."""
import contextlib
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import lls_util as s
from tests.test_local_cpu import _ref, _ref_ext_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ksw2amd_ll_sub_batch", "ksw2amd_ll_sub_batch_flat", "ksw2amd_ll_sub")


@pytest.fixture(scope="module")
def sim_so():
    return s.sim_library()


@pytest.fixture(scope="module")
def sim(sim_so):
    return ksw2_amd.Library(sim_so)


def _pin_sets(rng):
    """the four set kinds of test_local_cpu._pin_sets with a second, weaker hit in most targets, so that score2 > 0"""
    m5, m20 = s.M5, u.random_mat(rng, 20)
    out = []
    for n, m, lo, hi, mat, go, ge in ((700, 5, 8, 160, m5, 4, 2), (600, 20, 8, 120, m20, 6, 1), (600, 4, 20, 200, m5, 4, 2), (600, 5, 8, 120, m5, 0, 1)):
        q = [rng.integers(0, m, int(rng.integers(lo, hi + 1)), dtype=np.uint8) for _ in range(n)]
        t = [np.concatenate([u.mutate(rng, x, m, 0.03, 0.02), rng.integers(0, m, int(rng.integers(1, 40)), dtype=np.uint8),
                             u.mutate(rng, x, m, 0.08, 0.02), rng.integers(0, m, int(rng.integers(0, 20)), dtype=np.uint8)]) for x in q]
        out.append((q, t, mat, 5 if m == 4 else m, go, ge))
    return out


def test_oracle_pinned_to_reference_extz(sim):
    """For the oracle's (score2, qe2, te2) with score2 > 0: the reference's scalar ksw_extz on reverse(query[0..qe2]), reverse(target[0..te2])
    (extension only, score only, unbanded, no Z-drop) reaches a max equal to score2.  The simulator build returns the same six numbers."""
    ref = _ref()
    rng = np.random.default_rng(12)
    total = 0
    for q, t, mat, m, go, ge in _pin_sets(rng):
        exp = s.check(sim, q, t, mat, go, ge, m=m)
        for i in range(len(q)):
            s2, qe2, te2 = map(int, exp[i, 3:])
            if s2 == 0:
                assert qe2 == -1 and te2 == -1
                continue
            total += 1
            assert _ref_ext_max(ref, q[i][:qe2 + 1], t[i][:te2 + 1], mat, m, go, ge) == s2, (i, exp[i], go, ge)
    assert total >= 2000, total


def test_definition_brute_force(sim):
    """400 tiny pairs over two letters, excl in {-1, 0, 1, 3}: the window, the smallest te2 and the smallest qe2 of the pure-Python
    definition, the oracle and the simulator agree."""
    rng = np.random.default_rng(6)
    mat = u.simple_mat(2, 1, 1)
    for k in range(400):
        q = rng.integers(0, 2, int(rng.integers(1, 9)), dtype=np.uint8)
        t = np.tile(q, 3) if k % 3 == 0 else rng.integers(0, 2, int(rng.integers(1, 14)), dtype=np.uint8)
        go, ge = [(1, 1), (0, 1), (0, 0), (2, 0)][k % 4]
        excl = (-1, 0, 1, 3)[(k // 4) % 4]
        b = s.brute(q, t, mat, go, ge, 2, excl)
        assert tuple(int(x) for x in s.oracle_batch([q], [t], mat, go, ge, excl, 2)[0]) == b, (q, t, go, ge, excl)
        res, sub = sim.ll_sub_batch([q], [t], mat, go, ge, excl=excl, m=2)
        assert tuple(int(x) for x in res[0]) + tuple(int(x) for x in sub[0]) == b, (q, t, go, ge, excl)


def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ksw2_amd.h")).read(), flags=re.S)
    if not os.path.exists(ksw2_amd.DEFAULT_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ksw2_amd", "csrc")], check=True, capture_output=True)
    lib = ctypes.CDLL(ksw2_amd.DEFAULT_SO)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ksw2_amd.EXPORTS
        assert hasattr(lib, name), name
    assert "ksw2amd_lsub_t" in src and ctypes.sizeof(ksw2_amd.LocalSub) == 12


def test_sim_generation_edges(sim, monkeypatch):
    s.check_generation_edges(sim, monkeypatch)


def test_sim_forced_orientation(sim, monkeypatch):
    s.check_forced_orientation(sim, monkeypatch)


def test_sim_window_edges(sim, monkeypatch):
    s.check_window_edges(sim, monkeypatch)


def test_sim_differing_halves(sim, monkeypatch, capfd):
    s.check_differing_halves(sim, monkeypatch, capfd)


def test_sim_ties(sim, monkeypatch):
    s.check_ties(sim, monkeypatch)


def test_sim_wide_query_takes_int32(sim, monkeypatch, capfd):
    s.check_wide_query(sim, monkeypatch, capfd)


def test_sim_wide_score_int32_words(sim, monkeypatch, capfd):
    s.check_wide_score(sim, monkeypatch, capfd)


@pytest.mark.parametrize("k", range(len(s.RAGGED)))
def test_sim_ragged_parity(sim, monkeypatch, k):
    """the ragged sets of the GPU tier, thinned to what a lock-step simulator runs in seconds (every 40th short pair, the two shortest
    long ones), in every (form, lookup) combination"""
    q, t, mat, m, go, ge = s.ragged_set(k)
    long2 = sorted(range(2000, 2050), key=lambda i: len(q[i]) * len(t[i]))[:2]
    idx = list(range(0, 2000, 40)) + long2
    for form, lds in s.forms(monkeypatch):
        if m > 5 and lds == "0":
            continue                                     # m = 20 takes the LDS lookup whatever the switch says
        s.check(sim, [q[i] for i in idx], [t[i] for i in idx], mat, go, ge, m=m)


@contextlib.contextmanager
def _placed(lib, base, kind):
    yield dict()


def test_sim_flat_entries(sim, monkeypatch):
    s.reset_counters(sim)
    s.check_flat(sim, _placed, ["host"], monkeypatch)
    assert s.sub_launches(sim) > 0


def test_sim_flat_bad_code_launches_nothing(sim):
    from tests import llf_util as f
    q, t = [np.array([0, 1, 2, 9], np.uint8)], [np.array([0, 1, 2, 3], np.uint8)]
    a = f.arena(q, t)
    s.reset_counters(sim)
    with pytest.raises(ksw2_amd.Ksw2Error, match="error -2"):
        sim.ll_sub_batch_flat(*a, s.M5, 4, 2)
    assert s.sub_launches(sim) == 0 and f.counters(sim)[0] == 0


def test_sim_bad_arguments_and_single_calls(sim):
    from tests import llf_util as f
    s.reset_counters(sim)
    s.check_bad_arguments(sim, ksw2_amd.Ksw2Error, launches=lambda: s.sub_launches(sim) + sum(f.counters(sim)[:2]))
    assert s.sub_launches(sim) > 0                       # the single-pair calls behind them did launch


def test_sim_c_caller_public_header(sim_so, tmp_path):
    s.check_c_caller(os.path.dirname(sim_so), "ksw2_amd_llssim", tmp_path)


def test_golden_vectors_match_the_oracle(sim):
    for q, t, mat, m, go, ge, excl, exp in s.load_golden():
        np.testing.assert_array_equal(s.oracle_batch(q, t, mat, go, ge, excl, m), exp)
        res, sub = sim.ll_sub_batch(q, t, mat, go, ge, excl=excl, m=m)
        np.testing.assert_array_equal(np.hstack([res, sub]), exp)
