"""CPU: the code that prepares bytes for the alignment kernels -- the wire-format expansion of a uniform plan's upload, the span
arithmetic of that expansion, and the look a wavefront-task takes at its targets (k2a_scan_codes) -- on the simulator build
(tests/sim), which shares k2a_span_end and k2a_scan_codes with the kernels (ksw2_lane.h).  The same checks run on the device from
tests/test_gpu_wire.py."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import wire_util as wu
from tests.parity_util import check_batch
from tests.test_sim_parity import sim  # noqa: F401  (the simulator build's fixture)


@pytest.fixture(autouse=True)
def _small_batches_stay_packed(monkeypatch):
    monkeypatch.setenv("KSW2AMD_SIMDS", "0")


def test_sim_dense_escapes_through_every_expansion_path(sim, monkeypatch):
    """wire_util.check_dense_escapes on the simulator (its expansion is serial: it pins the host's packing of the escape entries, the
    slot layout and the routing of every path, not the order of the device's stores)."""
    wu.check_dense_escapes(sim, monkeypatch.setenv, monkeypatch.delenv, 2058, 300, 290, seed=9300)


def test_span_end_at_the_32_bit_wrap(sim):
    """k2a_span_end (ksw2_lane.h): the end of the span of arena bytes a workgroup of the whole-arena expansion (16 pairs) or a
    wavefront-task of a streamed launch (2 * NG pairs) expands, at the last three blocks of the largest arena a uniform plan admits
    (0xffef0000 bytes).  A 2-bit stride is below 2^20: 0xffff0 at the most.  The 4-bit format has no such limit, but a uniform plan
    holds at least 2048 pairs: its stride is at most 0xffef0000 / 2048 (rounded down to 16) and its span 2 * 8 of them (the (8, 18)
    class, eight tasks per wavefront).  And an arena as a plan lays it out: 8188 pairs of stride 0x80000, whose last workgroup of 16
    pairs ends at 8192 * 0x80000 = 2^32 exactly -- the sum wraps to 0, and min() of it left the last 12 pairs unexpanded."""
    f = sim.lib.k2a_sim_span_end
    f.argtypes, f.restype = [ctypes.c_uint32] * 3, ctypes.c_uint32
    top = 0xffef0000
    stride4 = top // 2048 // 16 * 16
    wraps = 0
    for total, span in ((top, 16 * 0xffff0), (top, 2 * 0xffff0), (top, 16 * stride4), (top, 2 * stride4), (8188 * 0x80000, 16 * 0x80000), (top, 0x1ffde00 + 16)):
        assert total <= top
        nblk = (total + span - 1) // span
        for blk in (nblk - 3, nblk - 2, nblk - 1):
            b0 = blk * span
            assert 0 <= b0 < total
            end = f(b0, span, total)
            print("total %#x span %#x block %d: [%#x, %#x)" % (total, span, blk, b0, end))
            assert b0 < end <= total, (hex(total), hex(span), blk, hex(end))
            if b0 + span <= total:                                   # (Python integers: the sum as it is meant)
                assert end == b0 + span
            else:
                assert end == total
            wraps += b0 + span >= 1 << 32
    assert wraps >= 1
    assert f(0, 16, 16) == 16 and f(0, 32, 16) == 16 and f(0xfffffff0, 0x20, 0xfffffff8) == 0xfffffff8


def _plain_scan(t, n):
    """What a wavefront-task's look at target bytes [0, n) has to report, byte by byte: bit 0 = a byte with bit 2 set (the wildcard; the
    codes 5-7 select the TN body too, and are handed back anyway), bit 1 = a code above 4."""
    b = np.asarray(t[:n], dtype=np.uint8)
    return int(np.bitwise_or.reduce(((b & 4) >> 2) | ((b > 4) << 1).astype(np.uint8)))


@pytest.mark.parametrize("G", [8, 16, 64])
def test_scan_codes_at_every_length_and_position(sim, G):
    """k2a_scan_codes for a group of G lanes (each lane's call, ORed as the kernels' ballot does), n = 1 .. 3 * 16 * G + 5 (three rounds
    of the group and a tail): a clean target reports nothing although bytes 4 and 5 lie at n, n + 1 and n + 2, just past its end; a
    single code 4 at EVERY position is seen as the wildcard and nothing else; code 5 at the last byte is seen as a code above 4.  The
    expected value is _plain_scan's byte loop (for the one-wildcard sweep: of the clean bytes, ORed with the loop's value for the one
    byte that differs)."""
    f = sim.lib.k2a_sim_scan_sweep
    f.argtypes, f.restype = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int
    nmax = 3 * 16 * G + 5
    clean = np.random.default_rng(G).integers(0, 4, nmax + 16, dtype=np.uint8)
    out = np.zeros(nmax, dtype=np.uint8)
    for n in range(1, nmax + 1):
        t = clean.copy()
        t[n:n + 3] = (4, 5, 4) if n % 2 else (5, 4, 5)
        base = _plain_scan(t, n)
        assert base == 0
        assert f(G, t.ctypes.data, n, 0, 4, out.ctypes.data) == 0
        bad = np.flatnonzero(out[:n] != (base | _plain_scan(np.array([4], dtype=np.uint8), 1)))
        assert not len(bad), (G, n, "wildcard at", bad[:5], out[bad[:5]])
        for code, p0 in ((5, n - 1), (0, n - 1), (4, n - 1), (7, max(0, n - 2)), (8, max(0, n - 3)), (5, max(0, n - 4))):
            assert f(G, t.ctypes.data, n, p0, code, out.ctypes.data) == 0
            for p in range(p0, n):
                x = t.copy()
                x[p] = code
                assert out[p - p0] == _plain_scan(x, n), (G, n, p, code, out[p - p0])


def test_sim_takes_the_plain_or_the_tn_body(sim, monkeypatch):
    """The simulator picks the build of a wavefront-task's body as the kernels do: from k2a_scan_codes of the task's targets.  A batch
    without a target wildcard runs plain bodies only, one with a wildcard in every target TN bodies only, and with KSW2AMD_TN=0 nothing
    runs a TN body; all against the oracle.  pk (score only and with CIGAR), solo, generation-serial."""
    def counts():
        c = (ctypes.c_ulonglong * 2)()
        sim.lib.k2a_sim_body_counts(c)
        return int(c[0]), int(c[1])

    cases = [(24, 120, 128, 16, -1, po.SCORE_ONLY, False, {}), (24, 128, 120, 16, 60, 0, False, {}),
             (6, 500, 490, 64, 100, 0, True, {"KSW2AMD_SOLO": "all"}), (4, 2300, 2337, -1, 300, po.SCORE_ONLY, True, {})]
    for ci, (n, ql, tl, w, zd, flag, dual, env) in enumerate(cases):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        q, t = wu.synth.fixed_batch(7400 + ci, n, ql, tl, sub=0.05, ind=0.06)
        qs, ts = [np.array(x, dtype=np.uint8) for x in q], [np.array(x, dtype=np.uint8) for x in t]
        qs[1][7] = 4                                          # (a query wildcard asks for no TN body)
        c0 = counts()
        check_batch(sim, dual, qs, ts, wu.MAT, 4, 2, 24, 1, w=w, zdrop=zd, flag=flag)
        c1 = counts()
        assert c1[0] > c0[0] and c1[1] == c0[1], (ci, c0, c1)
        for x in ts:
            x[tl - 1] = 4
        check_batch(sim, dual, qs, ts, wu.MAT, 4, 2, 24, 1, w=w, zdrop=zd, flag=flag)
        c2 = counts()
        assert c2[0] == c1[0] and c2[1] > c1[1], (ci, c1, c2)
        monkeypatch.setenv("KSW2AMD_TN", "0")
        check_batch(sim, dual, qs, ts, wu.MAT, 4, 2, 24, 1, w=w, zdrop=zd, flag=flag)
        assert counts()[1] == c2[1], (ci, c2, counts())
        monkeypatch.delenv("KSW2AMD_TN")
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("ci", range(len(wu.SCAN_CASES)))
def test_sim_scan_boundaries(sim, monkeypatch, ci):
    wu.check_scan_boundaries(sim, monkeypatch.setenv, monkeypatch.delenv, ci)
