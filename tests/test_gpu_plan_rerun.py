"""GPU: a resident plan run more than once returns its first run's results (tests/rerun_util.py), on libksw2_amd.so.  The resident
plan is what bench.py times -- runs 2 .. N of one plan -- so every kernel class goes through the lifecycle here: run, fetch, fetch
again, two more runs, a run on a second stream (created through the library's own HIP runtime), and a run after ksw2amd_plan_scrub has taken every record away; each step against
the oracle on every field and CIGAR and against the first run on every raw column.  One plan per kernel class, the class asserted from
the plan's description."""
import pytest

import ksw2_amd as ka
from tests import form_edge_util as fe
from tests import rerun_util as ru
from tests import trace_util as tu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@pytest.fixture(scope="module")
def second_stream(lib):
    """A non-null stream for the lifecycle's run on another stream, and the wait for the first one: from the HIP runtime the library
    itself is linked against (found among this process's mappings).  Not torch.cuda.Stream(): torch brings a HIP runtime of its own,
    and initialised in a process after the library's it finds no device (hipErrorNoDevice) -- bench.py initialises torch first."""
    import ctypes
    paths = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})
    assert paths, "the library's HIP runtime is not mapped"
    hip = ctypes.CDLL(paths[0])
    s = ctypes.c_void_p()
    rc = hip.hipStreamCreate(ctypes.byref(s))
    assert rc == 0 and s.value, rc

    def sync():
        assert hip.hipDeviceSynchronize() == 0
    yield dict(sync=sync, stream2=s.value)
    hip.hipStreamDestroy(s)


def _kw(ss):
    return dict(sync=ss["sync"], stream2=ss["stream2"])


@pytest.mark.parametrize("name", ru.PLAN_CASE_NAMES)
def test_plan_rerun(lib, monkeypatch, second_stream, name):
    ru.run_plan_cases(lib, monkeypatch.setenv, monkeypatch.delenv, [name], **_kw(second_stream))


@pytest.mark.parametrize("names", [("ragged-1p-fork", "ragged-2p-fork"), ("solo-cigar", "solo-2p-score"), ("pkmp-score", "pkmp-2p-cigar")],
                         ids=["ragged", "solo", "pkmp"])
def test_two_plans_alive(lib, monkeypatch, second_stream, names):
    """two plans on one thread, their steps interleaved: A's run, B's run, A's fetch, B's fetch"""
    ru.run_plan_cases(lib, monkeypatch.setenv, monkeypatch.delenv, list(names), **_kw(second_stream))


@pytest.mark.parametrize("want", fe.WANTS)
def test_form_rerun(lib, monkeypatch, second_stream, want):
    """one group per kernel form of the splice, X-drop and SSE-compatible plans"""
    ru.run_form_group(lib, monkeypatch.setenv, monkeypatch.delenv, want, **_kw(second_stream))


@pytest.mark.parametrize("form", tu.FORMS, ids=tu.FORM_IDS)
def test_trace_rerun(lib, monkeypatch, second_stream, form):
    """one group of the path-shape grid per walk form"""
    ru.run_trace_form(lib, monkeypatch.setenv, monkeypatch.delenv, form, **_kw(second_stream))
