"""GPU: the suboptimal local score under the two-piece gap cost and the two-piece single-pair entries (ksw2amd_lld_sub_batch / _flat,
ksw2amd_lld, ksw2amd_lld_align, ksw2amd_lld_sub) on libksw2_amd.so: the golden vectors of tests/golden/llds_cases.npz and the grid of
tests/llds_util.py against the scalar test oracle (tests/llds_oracle.c), one test per grid item.  The shapes are the smallest at which
SUB x DUAL can go wrong: a two-piece gap across the generation boundary that moves score2 only, one that moves score and with it the
window, the shoulder of the best hit, the edge grid of the single-piece suboptimal score under two cost tuples, the lane hand-over rows,
equal pieces against ksw2amd_ll_sub_batch.  Every case also asserts that res equals ksw2amd_lld_batch's."""
import os

import numpy as np
import pytest

import ksw2_amd as ka
from tests import llds_util as x
from tests.test_gpu_local_flat import KINDS, placed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS", "KSW2AMD_TRACE"):
        monkeypatch.delenv(k, raising=False)


def test_golden_vectors(lib):
    for q, t, mat, m, costs, excl, exp in x.load_golden():
        res, sub = lib.lld_sub_batch(q, t, mat, *costs, excl=excl, m=m)
        np.testing.assert_array_equal(np.hstack([res, sub]), exp)
        np.testing.assert_array_equal(res, lib.lld_batch(q, t, mat, *costs, m=m))


def test_item1_generation_boundary(lib, monkeypatch, capfd):
    x.check_boundary(lib, monkeypatch, capfd)


def test_item2_window_follows_the_two_piece_score(lib, monkeypatch):
    x.check_window(lib, monkeypatch)


def test_item3_shoulder(lib, monkeypatch):
    x.check_shoulder(lib, monkeypatch)


@pytest.mark.parametrize("name", ["generation_edges", "window_edges", "differing_halves", "tandem_repeats", "forced_orientation", "wide_score", "wide_query"])
def test_item4_and_6_edge_grid(lib, monkeypatch, name):
    x.check_grid4(lib, monkeypatch, name)


def test_item5_shape_grid(lib, monkeypatch):
    x.check_shape_grid(lib, monkeypatch)


def test_item7_single_pair_entries(lib):
    x.check_single(lib)


@pytest.mark.parametrize("costs", [x.CROSS, x.CHEAP2, (0, 0, 0, 0)])
def test_ragged_parity(lib, costs):
    """300 pairs of lengths 1 - 600 plus 6 of up to 3 000 per cost tuple, m = 5 and m = 20"""
    x.check_ragged(lib, costs)


def test_flat_entries(lib, monkeypatch):
    x.check_flat(lib, placed, KINDS, monkeypatch)


def test_bad_arguments(lib):
    x.check_bad_arguments(lib, ka.Ksw2Error)


def test_c_caller_public_header(lib, tmp_path):
    x.check_c_caller(os.path.join(ROOT, "ksw2_amd"), "ksw2_amd", tmp_path)
