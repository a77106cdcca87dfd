"""GPU: the code that prepares bytes for the alignment kernels (tests/wire_util.py): dense escape entries of the 2-bit wire format
through every expansion path of a uniform plan -- the whole-arena expansion behind an abandoned streamed launch among them, whose four
wavefronts per workgroup must not store a chunk on top of an escape byte -- and single wildcards at the boundaries of the look a
wavefront-task takes at its targets (k2a_scan_codes).  Bit-exact against the general path and the oracle."""
import pytest

import ksw2_amd as ka
from oracle import pyoracle as po
from tests import wire_util as wu

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _small_batches_stay_packed(monkeypatch):
    """(tests/test_gpu_parity.py: without this the host sends small packed classes back to the int32 kernels)"""
    monkeypatch.setenv("KSW2AMD_SIMDS", "0")


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@pytest.mark.parametrize("ql,tl,rem,flag", [(300, 290, 16, po.SCORE_ONLY), (320, 330, 64, po.SCORE_ONLY | po.EXTZ_ONLY)])
def test_dense_escapes_through_every_expansion_path(lib, monkeypatch, ql, tl, rem, flag):
    """wire_util.check_dense_escapes: 4 106 pairs (256 full workgroups of the whole-arena expansion and a partial one), every pair with
    wildcard runs, at two strides on the edge where only wavefront 0 of a workgroup runs the last round of chunk stores (stride mod 256
    = 16: the last 16 chunks of pair 15; = 64: the last 64)."""
    assert wu.wire2_stride(ql, tl) % 256 == rem
    wu.check_dense_escapes(lib, monkeypatch.setenv, monkeypatch.delenv, 4106, ql, tl, seed=9300 + rem, flag=flag)


def test_more_escapes_than_a_slot_holds(lib, monkeypatch):
    wu.check_escape_overflow(lib, monkeypatch.setenv, monkeypatch.delenv, 4106, 300, 290, seed=9316)


@pytest.mark.parametrize("ci", range(len(wu.SCAN_CASES)))
def test_scan_boundaries(lib, monkeypatch, ci):
    wu.check_scan_boundaries(lib, monkeypatch.setenv, monkeypatch.delenv, ci)
