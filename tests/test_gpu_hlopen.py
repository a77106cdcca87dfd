"""GPU: the packed kernels with H - q in their row registers and q + e + s in the column profiles (K2A_HL_OPEN, ksw2_lane_pk.h "Open
form"), under the scorings of tests/hlopen_util.py that sit on the boundaries of a profile byte, against the oracle on all fields and
CIGARs, at the smallest shapes that reach each form.  The geometry is forced through KSW2AMD_PK_FIRST and asserted, like the form,
from the plan's description; every case asserts that every pair is packed.

(64, 16): targets of 64 * 16 + 1 and 2 * 64 * 16 + 5 rows (more than one, more than two rounds of strips), bands 0, 16, 17 and the
widest the geometry admits (under the "deep" scoring the widest the re-based window admits of 100, 200, 536: 100 -- that scoring is the
one that runs re-based, the others run plain); deferred arg-max on and off, row selectors in LDS and in registers; plus one pair of
tests/edge_util.zdrop_pairs at its critical Z-drop minus one (drops: in a deferred fill its book is frozen and the second and third
passes read the checkpoint stream) and at the critical one (does not).  (8, 18) at 512 x 512, w 64.  Solo (an odd number of pairs) and
generation-serial at the shapes the CPU tier uses.  The two scorings with gap costs of 155 and more fit short pairs on a plain window
only and run there, score only and with CIGAR.

The oracle's records depend on the pair and its parameters only, so they are computed once and shared by the forms."""
import numpy as np
import pytest

import ksw2_amd as ka
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import hlopen_util as hu

pytestmark = pytest.mark.gpu

G, C = 64, 16
GI = 3                                               # KSW2AMD_PK_FIRST index of (64, 16)
GC = G * C
WMAX = (G * (C + 1) - C) // 2
LONG = [s for s in hu.SCORINGS if s not in hu.SHORT]
ZW = 40


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


_MEMO = {}


@pytest.fixture
def shared_oracle(monkeypatch):
    """oracle.pyoracle.align with a memo per (sequences, every argument): one reference per pair and parameter set for all forms"""
    real = po.align

    def align(impl, func, q, t, *a, **kw):
        key = (impl, func, np.asarray(q).tobytes(), np.asarray(t).tobytes(), tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in a),
               tuple(sorted(kw.items())))
        if key not in _MEMO:
            _MEMO[key] = real(impl, func, q, t, *a, **kw)
        return _MEMO[key]

    monkeypatch.setattr(po, "align", align)


_B = {}


def batch_64x16(scoring):
    """(queries, targets, w per pair, zdrop per pair): two pairs per (tlen, w), one of them under a Z-drop, and the critical pair twice"""
    if scoring in _B:
        return _B[scoring]
    mat, m, q, e, _, _, xflag, _, _, wild = hu.SCORINGS[scoring]
    qs, ts, ws, zs = [], [], [], []
    for tl in (GC + 1, 2 * GC + 5):
        for w in (0, C, C + 1, 100 if scoring == "deep" else WMAX):
            a, b = hu.pairs(8200 + tl + w, 2, tl, tl, m, wild, 60)
            qs += a; ts += b; ws += [w, w]; zs += [-1, 60]
    # a pair that drops at Z* - 1 and not at Z*, padded to the first shape; the builders without wildcards for the four-letter matrix
    zq, zt = eu.zdrop_pairs(8300, 6, 1.0)
    zq, zt = eu.same_shape(zq, zt, GC + 1)
    for k in range(len(zq)):
        if m == 4 and (zq[k] > 3).any():
            continue
        run = lambda zz: po.align("oracle", "extz2", zq[k], zt[k], mat, q, e, w=ZW, zdrop=zz, flag=po.SCORE_ONLY | xflag, m=m)["zdropped"] == 1      # noqa: E731
        z = eu.critical_zdrop(run)
        if z:
            qs += [zq[k], zq[k]]; ts += [zt[k], zt[k]]; ws += [ZW, ZW]; zs += [z - 1, z]
            break
    else:
        raise AssertionError("no pair with a critical Z-drop under " + scoring)
    _B[scoring] = (qs, ts, np.array(ws), np.array(zs))
    return _B[scoring]


@pytest.mark.parametrize("defer,ldscodes", [(1, 1), (0, 1), (0, 0)], ids=["defer", "ldscodes", "registers"])
@pytest.mark.parametrize("scoring", LONG)
def test_hlopen_64x16(lib, monkeypatch, shared_oracle, scoring, defer, ldscodes):
    qs, ts, ws, zs = batch_64x16(scoring)
    want = "defer" if defer else "ldscodes" if ldscodes else "registers"
    env = {"KSW2AMD_PK_FIRST": GI, "KSW2AMD_SOLO": 0, "KSW2AMD_DEFER": defer, "KSW2AMD_LDSCODES": ldscodes}
    rb = 1 if scoring == "deep" else 0
    check = lambda d: all(c["kernel"] == "pk" and (c["G"], c["C"]) == (G, C) and c["mode"] == "score" and c["form"] == want and c["nomax"] == 0 and      # noqa: E731
                          c["rebased"] == rb for c in d)
    hu.run_case(lib, monkeypatch.setenv, monkeypatch.delenv, scoring, env, False, po.SCORE_ONLY, qs, ts, ws, zs, check)
    # the critical pair: the last two of the batch
    mat, m, q, e, _, _, xflag, _, _, _ = hu.SCORINGS[scoring]
    exp = [po.align("oracle", "extz2", qs[i], ts[i], mat, q, e, w=ZW, zdrop=int(zs[i]), flag=po.SCORE_ONLY | xflag, m=m)["zdropped"] for i in (-2, -1)]
    assert exp == [1, 0], exp


@pytest.mark.parametrize("scoring", LONG)
def test_hlopen_8x18_solo_serial(lib, monkeypatch, shared_oracle, scoring):
    m, wild = hu.SCORINGS[scoring][1], hu.SCORINGS[scoring][9]
    qs, ts = hu.pairs(8400, 4, 512, 512, m, wild, 100)
    hu.run_case(lib, monkeypatch.setenv, monkeypatch.delenv, scoring, {"KSW2AMD_PK_FIRST": 0, "KSW2AMD_SOLO": 0}, False, po.SCORE_ONLY, qs, ts, 64, 100,
                lambda d: all(c["kernel"] == "pk" and (c["G"], c["C"]) == (8, 18) for c in d))
    for dual, flag in ((False, 0), (True, po.SCORE_ONLY)):
        qs, ts = hu.pairs(8410, 3, 300, 290, m, wild, 100)
        hu.run_case(lib, monkeypatch.setenv, monkeypatch.delenv, scoring, {"KSW2AMD_SOLO": "all"}, dual, flag, qs, ts, 64, 100,
                    lambda d: all(c["kernel"] == "solo" for c in d))
    if scoring != "deep":                 # (a row maximum may drift too far between two re-bases under that scoring: int32 before and now)
        for dual, flag, zd in ((False, po.SCORE_ONLY, -1), (True, 0, 300)):
            qs, ts = hu.pairs(8420, 2, 2300, 2337, m, wild, zd)
            hu.run_case(lib, monkeypatch.setenv, monkeypatch.delenv, scoring, {}, dual, flag, qs, ts, -1, zd, lambda d: all(c["kernel"] == "pkmp" for c in d))


@pytest.mark.parametrize("scoring", hu.SHORT)
def test_hlopen_byte_range_top(lib, monkeypatch, shared_oracle, scoring):
    for dual, flag, env in ((False, po.SCORE_ONLY, {"KSW2AMD_DEFER": 1}), (False, po.SCORE_ONLY, {"KSW2AMD_DEFER": 0}), (False, po.SCORE_ONLY | po.APPROX_MAX, {}),
                            (False, 0, {}), (False, po.RIGHT, {}), (True, 0, {})):
        qs, ts = hu.pairs(8500, 8, 40, 44, 5, False, 400)
        d = hu.run_case(lib, monkeypatch.setenv, monkeypatch.delenv, scoring, dict(env, KSW2AMD_SOLO=0), dual, flag, qs, ts, 10, 400,
                        lambda d: all(c["kernel"] == "pk" and c["rebased"] == 0 for c in d))
        assert d
