"""GPU: the suboptimal local score (ksw2amd_ll_sub_batch / _flat / ksw2amd_ll_sub) on libksw2_amd.so: the golden vectors of
tests/golden/lls_cases.npz, and the edge grid of tests/lls_util.py against the scalar test oracle (tests/lls_oracle.c) -- generation
edges, forced orientation, window edges, packed halves that differ, ties, beyond 16 bits, ragged parity, the flat entries, bad arguments,
single calls and a C caller built against include/ksw2_amd.h.  Every case also asserts that res equals ksw2amd_ll_batch's."""
import os

import numpy as np
import pytest

import ksw2_amd as ka
from tests import lls_util as s
from tests.test_gpu_local_flat import KINDS, placed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def test_golden_vectors(lib):
    for q, t, mat, m, go, ge, excl, exp in s.load_golden():
        res, sub = lib.ll_sub_batch(q, t, mat, go, ge, excl=excl, m=m)
        np.testing.assert_array_equal(np.hstack([res, sub]), exp)
        np.testing.assert_array_equal(res, lib.ll_batch(q, t, mat, go, ge, m=m))


def test_generation_edges(lib, monkeypatch):
    s.check_generation_edges(lib, monkeypatch)


def test_forced_orientation(lib, monkeypatch):
    s.check_forced_orientation(lib, monkeypatch)


def test_window_edges(lib, monkeypatch):
    s.check_window_edges(lib, monkeypatch)


def test_differing_halves(lib, monkeypatch, capfd):
    s.check_differing_halves(lib, monkeypatch, capfd)


def test_ties(lib, monkeypatch):
    s.check_ties(lib, monkeypatch)


def test_beyond_16_bits_wide_query(lib, monkeypatch, capfd):
    s.check_wide_query(lib, monkeypatch, capfd)


def test_beyond_16_bits_score(lib):
    """one 20 000 x 20 000 near-identical pair: score above 65 535 (int32 form), excl = 3 000 leaves rows outside the window"""
    rng = np.random.default_rng(311)
    q = rng.integers(0, 4, 20000, dtype=np.uint8)
    t = q.copy()
    t[rng.integers(0, 20000, 150)] = 4                 # wildcard columns: -1 each
    mat = s.u.simple_mat(5, 4, 6, -1)
    exp = s.check(lib, [q], [t], mat, 6, 2, excl=3000, positive=True)
    assert exp[0, 0] > 65535 and exp[0, 3] > 65535 and abs(int(exp[0, 5]) - int(exp[0, 2])) > 3000


def test_beyond_16_bits_score_small(lib, monkeypatch, capfd):
    s.check_wide_score(lib, monkeypatch, capfd)


@pytest.mark.parametrize("k", range(len(s.RAGGED)))
def test_ragged_parity(lib, k):
    """2 000 pairs of lengths 1-600 plus 50 of lengths up to 5 000, for each gap cost with m = 5 and m = 20"""
    q, t, mat, m, go, ge = s.ragged_set(k)
    assert len(q) == 2050
    exp = s.check(lib, q, t, mat, go, ge, m=m)
    assert (exp[:, 3] > 0).sum() > len(q) // 4


def test_flat_entries(lib, monkeypatch):
    s.check_flat(lib, placed, KINDS, monkeypatch)


def test_bad_arguments_and_single_calls(lib):
    s.check_bad_arguments(lib, ka.Ksw2Error)


def test_c_caller_public_header(lib, tmp_path):
    s.check_c_caller(os.path.join(ROOT, "ksw2_amd"), "ksw2_amd", tmp_path)
