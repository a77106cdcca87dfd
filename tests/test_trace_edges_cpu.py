"""CPU: the path-shape grid of tests/trace_util.py for every traceback walk form through the simulator build -- planted gaps at
every phase against strip boundaries, lane wraps, generation boundaries, window refetches and the four-cell probe; every record and
CIGAR against the oracle, the form asserted from describe(), and every event of the form's table met by at least trace_util.NEED of
the oracle's paths.  The shapes of more than 2 000 rows run a thinned sweep here (every third offset and rotation); the event table
is the same."""
import os
import subprocess

import pytest

import ksw2_amd as ka
from tests import trace_util as tu

SIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM_DIR], check=True, capture_output=True)
    L = ka.Library(os.path.join(SIM_DIR, "libksw2_amd_sim.so"))
    assert L.backend() == "sim"
    return L


@pytest.mark.parametrize("form", tu.FORMS, ids=tu.FORM_IDS)
def test_sim_trace_grid(sim, form, monkeypatch):
    ev = tu.check_form(sim, monkeypatch.setenv, monkeypatch.delenv, form, thin=3)
    tu.assert_coverage(form, ev)


@pytest.mark.parametrize("dual", [False, True], ids=["1p", "2p"])
def test_sim_cigar_round(sim, dual, monkeypatch):
    """n_cigar of 1, 2, 63, 64, 65, 128, 129 and the dense-indel pair, with and without KSW_EZ_REV_CIGAR, through the simulator's
    own CIGAR assembly (k2a_compact_kernel itself exists on the GPU only)."""
    for env, kernels in (({"KSW2AMD_NO_PK": 1}, {"int32"}), ({}, {"pk", "solo"})):
        seen = tu.check_compaction(sim, monkeypatch.setenv, monkeypatch.delenv, env, dual, kernels)
        assert all(seen.get((n, r), 0) >= 2 for n in tu.COMPACT_NOPS + (300,) for r in (False, True)), seen


def test_oracle_trace_golden():
    assert tu.check_golden_oracle() >= 200


def test_sim_trace_golden(sim, monkeypatch):
    assert tu.check_golden(sim, monkeypatch.setenv, monkeypatch.delenv) >= 400
