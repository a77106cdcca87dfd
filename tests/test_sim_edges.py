"""CPU: Z-drop at its critical threshold and the packed score window at its admission boundary (tests/edge_util.py) through the
simulator build, and the oracle against the reference's answers at those edges (tests/golden/edge_cases.npz)."""
import os
import subprocess

import pytest

import ksw2_amd as ka
from tests import edge_util as eu

SIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM_DIR], check=True, capture_output=True)
    L = ka.Library(os.path.join(SIM_DIR, "libksw2_amd_sim.so"))
    assert L.backend() == "sim"
    return L


@pytest.mark.parametrize("fam", eu.ZFAMILIES, ids=[f[0] for f in eu.ZFAMILIES])
def test_sim_zdrop_critical(sim, fam, monkeypatch):
    """Every pair at Z* (no drop) and Z* - 1 (drop) in one batch, pointer and flat entries, the family asserted from describe()."""
    n, ndrop = eu.check_zdrop_family(sim, monkeypatch.setenv, monkeypatch.delenv, fam, seed=100 + eu.ZFAMILIES.index(fam), scale=0.5)
    assert n >= 4


def test_sim_zdrop_critical_sse_exts_extf_small(sim, monkeypatch):
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {})
    assert eu.check_zdrop_sse(sim) >= 16
    assert eu.check_zdrop_exts(sim, monkeypatch.setenv, monkeypatch.delenv) >= 12
    assert eu.check_zdrop_extf(sim, monkeypatch.setenv, monkeypatch.delenv) >= 20
    eu.set_env(monkeypatch.setenv, monkeypatch.delenv, {})
    assert eu.check_zdrop_small_calls(sim) >= 9


def test_sim_zdrop_critical_uniform(sim, monkeypatch):
    assert eu.check_zdrop_uniform(sim, monkeypatch.setenv, monkeypatch.delenv) > 0


def test_sim_window_edges(sim, monkeypatch):
    seen = eu.check_window_edges(sim, monkeypatch.setenv, monkeypatch.delenv)
    assert seen.get("plain", 0) >= 64 and seen.get("solo", 0) >= 64 and seen.get("rb-C8", 0) >= 16 and seen.get("rb-C16", 0) >= 8, seen


def test_sim_slide_edges(sim, monkeypatch):
    assert eu.check_slide_edges(sim, monkeypatch.setenv, monkeypatch.delenv) >= 1


def test_sim_target_wildcard_extremes(sim, monkeypatch):
    assert eu.check_target_wildcard_extremes(sim, monkeypatch.setenv, monkeypatch.delenv) == 36


def test_sim_edge_golden(sim):
    assert eu.check_edge_golden(sim) == len(eu.edge_cases())


def test_oracle_edge_golden():
    assert eu.check_edge_golden_oracle() >= 400
