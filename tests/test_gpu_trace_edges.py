"""GPU: the path-shape grid of tests/trace_util.py on libksw2_amd.so -- every traceback walk form (k2a_trace_kernel for (16,8),
(64,8), (64,16), (64,32) and the generation-serial (64,16); k2a_trace_pk_kernel for (16,8), (64,8), (64,16), plain and re-based, and
the packed generation-serial layout; k2a_trace_solo_kernel; each under single and two-piece gaps) with the full sweeps, the CIGAR
round (k2a_compact_kernel), 1, 2 and 8 walks per wavefront, and the reference's answers on planted cases.  The packed (8,18)
geometry is score only: the plan never gives it a traceback, so it has no row here."""
import pytest

import ksw2_amd as ka
from tests import trace_util as tu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@pytest.mark.parametrize("form", tu.FORMS, ids=tu.FORM_IDS)
def test_trace_grid(lib, form, monkeypatch):
    ev = tu.check_form(lib, monkeypatch.setenv, monkeypatch.delenv, form, thin=1)
    tu.assert_coverage(form, ev)


@pytest.mark.parametrize("dual", [False, True], ids=["1p", "2p"])
def test_cigar_round(lib, dual, monkeypatch):
    for env, kernels in (({"KSW2AMD_NO_PK": 1}, {"int32"}), ({}, {"pk", "solo"})):
        seen = tu.check_compaction(lib, monkeypatch.setenv, monkeypatch.delenv, env, dual, kernels)
        assert all(seen.get((n, r), 0) >= 2 for n in tu.COMPACT_NOPS + (300,) for r in (False, True)), seen


@pytest.mark.parametrize("nwalks", [64, 4100, 32770])
@pytest.mark.parametrize("kernel,env", [("int32", {"KSW2AMD_NO_PK": 1}), ("pk", {"KSW2AMD_PK_FIRST": 1})], ids=["int32", "pk"])
def test_walks_per_wavefront(lib, kernel, env, nwalks, monkeypatch):
    """1, 2 and 8 walks per wavefront (64, 4 100 and 32 770 walks; the last block of the largest is partly filled), neighbouring
    threads on different paths, int32 and packed walks, single and two-piece gaps."""
    for dual in (False, True):
        assert tu.check_ppw(lib, monkeypatch.setenv, monkeypatch.delenv, env, dual, nwalks, kernel) == {64: 1, 4100: 2, 32770: 8}[nwalks]


def test_trace_golden(lib, monkeypatch):
    assert tu.check_golden(lib, monkeypatch.setenv, monkeypatch.delenv) >= 400
