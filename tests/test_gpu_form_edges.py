"""GPU: the form-boundary checks of tests/form_edge_util.py on libksw2_amd.so -- the exts window grid with the full mode product, the
extf tiers, windows, group forms and lane class with every content variant, the SSE-compatible LDS / register limits, and the
reference's answers at those limits (tests/golden/form_edge_cases.npz)."""
import pytest

import ksw2_amd as ka
from tests import form_edge_util as fe

pytestmark = pytest.mark.gpu

EXTS_KEYS = {"%s/%s" % (f, m) for f in ("exts-win8", "exts-win16", "exts-hbm") for m in ("score", "left", "right")}


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


def _run(lib, mp, cases):
    return fe.run_cases(lib, mp.setenv, mp.delenv, cases)


@pytest.mark.parametrize("ncols", [(447, 448, 449), (959, 960, 961)], ids=["8-slots", "16-slots"])
def test_exts_window_grid(lib, monkeypatch, ncols):
    """Unforced, every mode on every shape: exts-win8 up to 448, exts-win16 up to 960, exts-hbm past it."""
    cases = fe.exts_cases(ncols, rots=range(6))
    assert fe.check_zstar(cases) == 2 * len(ncols)
    seen = _run(lib, monkeypatch, fe.with_env(cases, fe.E_NONE))
    want = {k for k in EXTS_KEYS if k.split("/")[0] in {fe.EXTS_FORM[n] for n in ncols}}
    assert want <= set(seen) and sum(seen.values()) == len(cases), seen


def test_exts_window_grid_forced_16_slots(lib, monkeypatch):
    cases = fe.exts_cases((447, 448), rots=range(6))
    seen = _run(lib, monkeypatch, fe.with_env(cases, fe.E_REG))
    assert {"exts-win16/score", "exts-win16/left", "exts-win16/right"} == set(seen) and sum(seen.values()) == len(cases), seen


@pytest.mark.parametrize("ncols", [(447, 448, 449), (959, 960, 961)], ids=["8-slots", "16-slots"])
def test_exts_window_grid_forced_hbm(lib, monkeypatch, ncols):
    cases = fe.exts_cases(ncols, rots=range(6))
    seen = _run(lib, monkeypatch, fe.with_env(cases, fe.E_BIG))
    assert {"exts-hbm/score", "exts-hbm/left", "exts-hbm/right"} == set(seen) and sum(seen.values()) == len(cases), seen


def test_extf_lds_tiers(lib, monkeypatch):
    cases = fe.extf_tier_cases(thin=False)
    seen = _run(lib, monkeypatch, cases)
    assert seen == {"extf-lds": 60, "extf-hbm": 12}, seen


def test_extf_windows_and_span_128(lib, monkeypatch):
    seen = _run(lib, monkeypatch, fe.extf_window_cases())
    assert seen == {"extf-win4": 9, "extf-win8": 6, "extf-lds": 9}, seen


def test_extf_group_forms(lib, monkeypatch):
    seen = _run(lib, monkeypatch, fe.extf_group_cases())
    assert seen == {"extf-grp": 21, "extf-grp32": 18, "extf-grp64": 18, "extf-lds": 6}, seen


def test_extf_lane_ring_limit(lib, monkeypatch):
    seen = _run(lib, monkeypatch, fe.extf_lane_cases())
    assert seen == {"extf-lane": 20, "extf-lane/ldsring/64": 10, "extf-lane/hbm/0": 10}, seen


def test_ssec_lds_limit(lib, monkeypatch):
    seen = _run(lib, monkeypatch, fe.ssec_lds_cases())
    assert seen == {"lds/1": 6, "hbm/1": 6, "lds/2": 6, "hbm/2": 6}, seen


def test_ssec_register_form_limit(lib, monkeypatch):
    seen = _run(lib, monkeypatch, fe.ssec_blk_cases())
    assert seen.get("blk/1") == 3 and seen.get("blk/2") == 3 and seen.get("hbm/1", 0) + seen.get("lds/1", 0) == 15 and \
        seen.get("hbm/2", 0) + seen.get("lds/2", 0) == 15, seen


def test_form_edge_golden_cases(lib, monkeypatch):
    n, seen = fe.check_golden(lib, monkeypatch.setenv, monkeypatch.delenv)
    assert n >= 100 and EXTS_KEYS <= set(seen), seen
    assert {"extf-lds", "extf-hbm", "extf-win4", "extf-win8", "extf-grp", "extf-grp32", "extf-grp64", "extf-lane", "hbm/1", "lds/1", "blk/1", "hbm/2", "lds/2",
            "blk/2"} <= set(seen), seen
