"""CPU: a resident plan run more than once returns its first run's results (tests/rerun_util.py), through the simulator build.  This
tier pins the host half -- the first-run clears, the streamed flag, what a fetch writes into the plan's host records, the re-runs a
fetch does -- and the simulator twins of the kernels' own per-run initialisation.  One plan per kernel class, the class asserted from
the plan's description; the second-stream variant of the lifecycle belongs to the GPU tier."""
import os
import subprocess

import pytest

from tests import form_edge_util as fe
from tests import rerun_util as ru
from tests import trace_util as tu

import ksw2_amd as ka

SIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM_DIR], check=True, capture_output=True)
    L = ka.Library(os.path.join(SIM_DIR, "libksw2_amd_sim.so"))
    assert L.backend() == "sim"
    return L


@pytest.mark.parametrize("name", ru.PLAN_CASE_NAMES)
def test_sim_plan_rerun(sim, monkeypatch, name):
    ru.run_plan_cases(sim, monkeypatch.setenv, monkeypatch.delenv, [name])


def test_sim_case_names():
    assert sorted(ru.PLAN_CASE_NAMES) == sorted(c["name"] for c in ru.plan_cases())


@pytest.mark.parametrize("names", [("ragged-1p-fork", "ragged-2p-fork"), ("solo-cigar", "solo-2p-score"), ("pkmp-score", "pkmp-2p-cigar")],
                         ids=["ragged", "solo", "pkmp"])
def test_sim_two_plans_alive(sim, monkeypatch, names):
    """two plans on one thread, their steps interleaved: A's run, B's run, A's fetch, B's fetch"""
    ru.run_plan_cases(sim, monkeypatch.setenv, monkeypatch.delenv, list(names))


@pytest.mark.parametrize("want", fe.WANTS)
def test_sim_form_rerun(sim, monkeypatch, want):
    """one group per kernel form of the splice, X-drop and SSE-compatible plans"""
    ru.run_form_group(sim, monkeypatch.setenv, monkeypatch.delenv, want)


@pytest.mark.parametrize("form", tu.FORMS, ids=tu.FORM_IDS)
def test_sim_trace_rerun(sim, monkeypatch, form):
    """one group of the path-shape grid per walk form"""
    ru.run_trace_form(sim, monkeypatch.setenv, monkeypatch.delenv, form)
