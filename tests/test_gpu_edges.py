"""GPU: the edge checks of tests/edge_util.py on libksw2_amd.so -- Z-drop at its critical threshold through every kernel family
(larger pairs than the simulator tier), the packed score window at its admission boundary with full-size shapes, the headline
10 k x 10 k shape with the plan's own deferred arg-max rule, and the reference's answers at those edges."""
import pytest

import ksw2_amd as ka
from tests import edge_util as eu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def test_zdrop_critical_families(lib, monkeypatch):
    out = eu.check_zdrop_edges(lib, monkeypatch.setenv, monkeypatch.delenv, scale=1.0, npairs=24)
    assert all(v for v in out.values()), out


def test_zdrop_critical_uniform(lib, monkeypatch):
    assert eu.check_zdrop_uniform(lib, monkeypatch.setenv, monkeypatch.delenv, n=8192, ql=150, tl=140, w=30) > 0


def test_zdrop_headline_shape(lib, monkeypatch):
    eu.check_headline_zdrop(lib, monkeypatch.setenv, monkeypatch.delenv)


def test_window_edges(lib, monkeypatch):
    seen = eu.check_window_edges(lib, monkeypatch.setenv, monkeypatch.delenv, max_len=20000, max_cells=40_000_000, npairs=16)
    assert seen.get("plain", 0) >= 128 and seen.get("solo", 0) >= 128 and seen.get("rb-C8", 0) >= 32 and seen.get("rb-C16", 0) >= 16, seen


def test_slide_edges_and_target_wildcards(lib, monkeypatch):
    assert eu.check_slide_edges(lib, monkeypatch.setenv, monkeypatch.delenv, L=4000, npairs=8) >= 1
    assert eu.check_target_wildcard_extremes(lib, monkeypatch.setenv, monkeypatch.delenv) == 36


def test_edge_golden_cases(lib):
    assert eu.check_edge_golden(lib) == len(eu.edge_cases())
