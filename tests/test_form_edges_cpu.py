"""CPU: the kernel forms of ksw_exts2_sse, ksw_extf2_sse and the SSE-compatible mode on both sides of their admission limits
(tests/form_edge_util.py) through the simulator build -- one mode per shape, every limit shape -- and the oracle against the
reference's answers at those limits (tests/golden/form_edge_cases.npz)."""
import os
import subprocess

import pytest

import ksw2_amd as ka
from tests import form_edge_util as fe

SIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")
EXTS_KEYS = {"%s/%s" % (f, m) for f in ("exts-win8", "exts-win16", "exts-hbm") for m in ("score", "left", "right")}


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM_DIR], check=True, capture_output=True)
    L = ka.Library(os.path.join(SIM_DIR, "libksw2_amd_sim.so"))
    assert L.backend() == "sim"
    return L


def _run(sim, mp, cases):
    return fe.run_cases(sim, mp.setenv, mp.delenv, cases)


@pytest.mark.parametrize("ncols", [(447, 448, 449), (959, 960, 961)], ids=["8-slots", "16-slots"])
def test_sim_exts_window_grid(sim, monkeypatch, ncols):
    """Unforced: exts-win8 up to 448, exts-win16 up to 960, exts-hbm past it; every mode class of every form at a limit shape."""
    cases = fe.exts_cases(ncols)
    assert fe.check_zstar(cases) == 2 * len(ncols)
    seen = _run(sim, monkeypatch, fe.with_env(cases, fe.E_NONE))
    want = {k for k in EXTS_KEYS if k.split("/")[0] in {fe.EXTS_FORM[n] for n in ncols}}
    assert want <= set(seen) and sum(seen.values()) == len(cases), seen


def test_sim_exts_window_grid_forced_16_slots(sim, monkeypatch):
    """KSW2AMD_EXTS_REG=1: the shapes that fit eight slots through the 16-slot kernel."""
    cases = fe.exts_cases((447, 448))
    seen = _run(sim, monkeypatch, fe.with_env(cases, fe.E_REG))
    assert {"exts-win16/score", "exts-win16/left", "exts-win16/right"} == set(seen) and sum(seen.values()) == len(cases), seen


@pytest.mark.parametrize("ncols", [(447, 448, 449), (959, 960, 961)], ids=["8-slots", "16-slots"])
def test_sim_exts_window_grid_forced_hbm(sim, monkeypatch, ncols):
    """KSW2AMD_EXTS_BIG=1: every shape through the HBM-state kernel."""
    cases = fe.exts_cases(ncols)
    seen = _run(sim, monkeypatch, fe.with_env(cases, fe.E_BIG))
    assert {"exts-hbm/score", "exts-hbm/left", "exts-hbm/right"} == set(seen) and sum(seen.values()) == len(cases), seen


def test_sim_extf_lds_tiers(sim, monkeypatch):
    """tlen 1024 / 1025, 4096 / 4097, 21504 / 21505: extf-lds up to 21504, extf-hbm past it, unforced and with KSW2AMD_EXTF_LDS=1."""
    cases = fe.extf_tier_cases()
    seen = _run(sim, monkeypatch, cases)
    assert seen.get("extf-lds", 0) == sum(1 for c in cases if len(c["t"]) <= 21504) and seen.get("extf-hbm", 0) == sum(1 for c in cases if len(c["t"]) > 21504), seen
    assert seen["extf-hbm"] >= 8 and set(seen) == {"extf-lds", "extf-hbm"}, seen


def test_sim_extf_windows_and_span_128(sim, monkeypatch):
    seen = _run(sim, monkeypatch, fe.extf_window_cases())
    assert seen == {"extf-win4": 9, "extf-win8": 6, "extf-lds": 9}, seen


def test_sim_extf_group_forms(sim, monkeypatch):
    """Spans 160 / 161, 416 / 417, 928 / 929 through w, a short query and a short target."""
    seen = _run(sim, monkeypatch, fe.extf_group_cases(ntask={"extf-grp": 3, "extf-grp32": 1, "extf-grp64": 1, "extf-lds": 1}))
    assert seen == {"extf-grp": 9, "extf-grp32": 6, "extf-grp64": 6, "extf-lds": 3}, seen


def test_sim_extf_lane_ring_limit(sim, monkeypatch):
    seen = _run(sim, monkeypatch, fe.extf_lane_cases())
    assert seen == {"extf-lane": 20, "extf-lane/ldsring/64": 10, "extf-lane/hbm/0": 10}, seen


def test_sim_ssec_lds_limit(sim, monkeypatch):
    """KSW2AMD_SSEC_BLK=0: the last LDS target (896 single, 736 dual) and the first HBM one."""
    seen = _run(sim, monkeypatch, fe.ssec_lds_cases())
    assert seen == {"lds/1": 6, "hbm/1": 6, "lds/2": 6, "hbm/2": 6}, seen


def test_sim_ssec_register_form_limit(sim, monkeypatch):
    """Span 960 / 961 through w, qlen and tlen; KSW_EZ_GENERIC_SC and a 6-code matrix never take the register form."""
    seen = _run(sim, monkeypatch, fe.ssec_blk_cases())
    assert seen.get("blk/1") == 3 and seen.get("blk/2") == 3 and seen.get("hbm/1", 0) + seen.get("lds/1", 0) == 15 and \
        seen.get("hbm/2", 0) + seen.get("lds/2", 0) == 15, seen


def test_oracle_form_edge_golden():
    assert fe.check_golden_oracle() >= 100


def test_sim_form_edge_golden(sim, monkeypatch):
    n, seen = fe.check_golden(sim, monkeypatch.setenv, monkeypatch.delenv)
    assert n >= 100 and EXTS_KEYS <= set(seen), seen
    assert {"extf-lds", "extf-hbm", "extf-win4", "extf-win8", "extf-grp", "extf-grp32", "extf-grp64", "extf-lane", "hbm/1", "lds/1", "blk/1", "hbm/2", "lds/2",
            "blk/2"} <= set(seen), seen
