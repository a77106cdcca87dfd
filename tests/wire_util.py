"""Shared checks of the code that prepares bytes for the alignment kernels, for the product library (tests/test_gpu_wire.py) and the
simulator build (tests/test_wire_cpu.py): the wire-format expansion of a uniform plan's upload into the arena (k2a_wire2_task,
k2a_wire4_expand, the whole-arena expansion behind an abandoned streamed launch) and the look a wavefront-task takes at its targets
(k2a_scan_codes) to pick the plain or the TN build of its body.  A mistake there raises no error: a wildcard becomes code 0, or a
wildcard row is scored as an ordinary one, and a score is wrong."""
import numpy as np

from ksw2_amd import synth
from oracle import pyoracle as po
from tests.parity_util import check_batch, diff, oracle_batch

WIRE2_ESC = 7                         # K2A_WIRE2_ESC (ksw2_types.h): escape entries per pair
WIRE2_PAD = 4 * 4 * WIRE2_ESC         # K2A_WIRE2_PAD: arena bytes of extra target padding that make room for them
MAT, GAPO, GAPE, BAND, END_BONUS = synth.simple_mat(5, 2, 4, -1), 4, 2, 30, 7
ENV_KEYS = ("KSW2AMD_UNIFORM", "KSW2AMD_STREAM_PIECE_KB", "KSW2AMD_STREAM_SLEEP_US", "KSW2AMD_STREAM_FAULT", "KSW2AMD_STREAM_TIMEOUT_MS",
            "KSW2AMD_DEFER", "KSW2AMD_WIRE4", "KSW2AMD_WIRE2", "KSW2AMD_TN")


def _a16(x):
    return (x + 15) // 16 * 16


def wire2_stride(ql, tl):
    """A pair's region in a uniform plan's arena under the 2-bit format (ksw2_host_plan.c, uniform batches: u->stride)."""
    return _a16(ql) + _a16(tl + 64 + WIRE2_PAD)


def _oracle(q, t, flag):
    return po.align("oracle", "extz2", q, t, MAT, GAPO, GAPE, w=BAND, zdrop=-1, end_bonus=END_BONUS, flag=flag)


def _put(seq, at, ln):
    seq[at:at + ln] = 4


_batches = {}


def dense_escape_batch(seed, n, ql, tl, flag):
    """One uniform score-only batch in which EVERY pair carries wildcard runs (escape entries of the 2-bit format), by i mod 16:
      0       all seven entries of the pair's slot: four runs in the target, three in the query
      1 / 2   a run at q[0] / one that ends at q[qlen - 1]
      3 / 4   a run at t[0] / one that ends at t[tlen - 1]
      5       a run longer than an entry's length field holds (255): two entries
      6       runs in both sequences
      7, 15   an earlier run, and a FINAL run of four within the last 60 target bytes -- the chunk a late store of the whole-arena
              expansion can put back on top of the escape bytes (pair 15 of a workgroup: its last chunks are stored by wavefront 0's extra
              round while wavefront 1 writes its escapes; pair 7: wavefront 0's escapes under the chunks of wavefronts 2 and 3)
      others  one to three random runs
    The final run of a 7 / 15 pair is placed where LOSING it shows: the oracle's record for the input with that run replaced by code 0
    differs from its record for the true input (start positions are tried in a seeded order until one does; each such pair must have
    one).  Returns (queries, targets, {pair: oracle record} for the 7 / 15 pairs)."""
    key = (seed, n, ql, tl, flag)
    if key in _batches:
        return _batches[key]
    assert ql - 20 > 255 and tl >= 100
    q, t = synth.fixed_batch(seed, n, ql, tl, sub=0.05, ind=0.06)
    qs, ts = [np.array(x) for x in q], [np.array(x) for x in t]
    rng = np.random.Generator(np.random.PCG64(seed))
    exp = {}
    for i in range(n):
        k, qi, ti = i % 16, qs[i], ts[i]
        if k == 0:
            for j in range(4):
                _put(ti, (2 * j + 1) * tl // 9, 1 + j % 3)
            for j in range(3):
                _put(qi, (2 * j + 1) * ql // 7, 2)
        elif k == 1:
            _put(qi, 0, 3)
        elif k == 2:
            _put(qi, ql - 2, 2)
        elif k == 3:
            _put(ti, 0, 2)
        elif k == 4:
            _put(ti, tl - 3, 3)
        elif k == 5:
            _put(qi, 10, ql - 20)
        elif k == 6:
            _put(qi, ql // 3, 5)
            _put(ti, tl // 2, 6)
        elif k in (7, 15):
            _put(ti, int(rng.integers(0, tl - 90)), 4 if k == 7 else 2)
            if k == 15:
                _put(qi, int(rng.integers(0, ql - 3)), 3)
            for at in rng.permutation(np.arange(tl - 60, tl - 3)):
                true, lost = ti.copy(), ti.copy()
                _put(true, int(at), 4)
                lost[at:at + 4] = 0
                e = _oracle(qi, true, flag)
                if diff(e, _oracle(qi, lost, flag)):
                    ts[i], exp[i] = true, e
                    break
            assert i in exp, ("no place for a final run whose loss shows", i)
        else:
            for _ in range(int(rng.integers(1, 4))):
                s = qi if rng.random() < 0.5 else ti
                ln = int(rng.integers(1, 13))
                _put(s, int(rng.integers(0, len(s) - ln + 1)), ln)
    _batches[key] = (qs, ts, exp)
    return _batches[key]


def check_dense_escapes(lib, setenv, delenv, n, ql, tl, seed, flag=po.SCORE_ONLY, whole_arena=True):
    """The dense-escape batch through every expansion path of a uniform plan, every record against the general path's and the 7 / 15
    pairs (plus every 64th pair) against the oracle:
      (a) KSW2AMD_UNIFORM=0                      the general path
      (b) WIRE2=1, 64 KB pieces                  2-bit format, expanded by the wavefront that needs the pairs (k2a_queue_wait)
      (c) (b) + the fault hook, 20 ms timeout    2-bit format, whole-arena expansion of the repeated run (k2a_wire2_expand_kernel)
      (d) (c) without WIRE2                      4-bit format, whole-arena expansion
      (e) WIRE4=0                                no wire format
    A decoy batch of the same shape goes through the same buffers in front of every run: the recycled arena then holds other bytes.
    (The fault hook is the host's: it withholds the upload's last watermark, the kernels leave through their bounded wait.)
    The shape sits on the edge the whole-arena expansion can lose escapes at: 16 pairs per workgroup of 256 lanes make
    16 * stride / 16 = stride chunks, and with stride mod 256 in 16 .. 64 only wavefront 0 runs the last round."""
    stride = wire2_stride(ql, tl)
    assert stride % 256 in (16, 32, 48, 64), (ql, tl, stride)
    assert n >= 2048 and n % 2 == 0 and n % 16 != 0, n
    qs, ts, exp = dense_escape_batch(seed, n, ql, tl, flag)
    assert sorted(exp) == [i for i in range(n) if i % 16 in (7, 15)]
    drng = np.random.default_rng(seed + 1)
    decoy = (drng.integers(0, 4, (n, ql), dtype=np.uint8), drng.integers(0, 4, (n, tl), dtype=np.uint8))

    def run(q_, t_, env):
        for k in ENV_KEYS:
            delenv(k, raising=False)
        for k, v in env.items():
            setenv("KSW2AMD_" + k, str(v))
        s0 = lib.stream_stats()
        res = lib.extz_batch(q_, t_, MAT, GAPO, GAPE, w=BAND, zdrop=-1, end_bonus=END_BONUS, flag=flag)
        s1 = lib.stream_stats()
        return res, s1["streamed_plans"] - s0["streamed_plans"], s1["aborted_runs"] - s0["aborted_runs"]

    b = dict(UNIFORM=1, WIRE2=1, STREAM_PIECE_KB=64)
    c = dict(b, STREAM_FAULT=1, STREAM_TIMEOUT_MS=20)
    d = dict(UNIFORM=1, STREAM_PIECE_KB=64, STREAM_FAULT=1, STREAM_TIMEOUT_MS=20)
    e = dict(UNIFORM=1, STREAM_PIECE_KB=64, WIRE4=0)
    runs = [("general", dict(UNIFORM=0), 0, 0), ("wire2", b, 1, 0)] + ([("wire2 whole arena", c, 1, 1), ("wire4 whole arena", d, 1, 1)] if whole_arena else []) + [("no wire format", e, 1, 0)]
    ref = None
    try:
        for name, env, streamed, aborted in runs:
            run(decoy[0], decoy[1], dict(env, STREAM_FAULT=0))      # (the decoy never takes the fault hook: one abandoned launch per case)
            res, ns, na = run(qs, ts, env)
            assert (ns, na) == (streamed, aborted), (name, ns, na)
            if ref is None:
                ref = res
                continue
            bad = [i for i in range(n) if diff(ref[i], res[i])]
            print("dense escapes %dx%d %s: %d of %d pairs differ from the general path" % (ql, tl, name, len(bad), n))
            assert not bad, (name, len(bad), bad[:8], [i % 16 for i in bad[:8]])
        for i in sorted(set(exp) | set(range(0, n, 64))):
            x = exp[i] if i in exp else _oracle(qs[i], ts[i], flag)
            assert not diff(x, ref[i]), ("oracle", i, diff(x, ref[i]))
    finally:
        for k in ENV_KEYS:
            delenv(k, raising=False)


def check_escape_overflow(lib, setenv, delenv, n, ql, tl, seed, flag=po.SCORE_ONLY):
    """One pair with eight runs -- more than its slot's seven entries -- sends the whole dense-escape batch to the general path: same records."""
    qs, ts, _ = dense_escape_batch(seed, n, ql, tl, flag)
    qs = list(qs)
    qs[20] = qs[20].copy()
    qs[20][qs[20] > 3] = 0
    for k in range(8):
        _put(qs[20], 4 + 11 * k, 2)
    out = []
    try:
        for env in (dict(UNIFORM=0), dict(UNIFORM=1, WIRE2=1, STREAM_PIECE_KB=64)):
            for k in ENV_KEYS:
                delenv(k, raising=False)
            for k, v in env.items():
                setenv("KSW2AMD_" + k, str(v))
            out.append(lib.extz_batch(qs, ts, MAT, GAPO, GAPE, w=BAND, zdrop=-1, end_bonus=END_BONUS, flag=flag))
    finally:
        for k in ENV_KEYS:
            delenv(k, raising=False)
    assert not [i for i in range(n) if diff(out[0][i], out[1][i])]
    assert not diff(_oracle(qs[20], ts[20], flag), out[1][20])


# (pairs, qlen, tlen, w, zdrop, flag, dual, G, C): the shapes of parity_util.check_target_wildcards cases 0-2, and a fourth whose
# (8, 18) targets are longer than one round of the scan (16 * G = 128 bytes)
SCAN_CASES = [(24, 120, 128, 16, -1, po.SCORE_ONLY, False, 8, 18),
              (24, 128, 120, 16, 60, 0, False, 16, 8),
              (12, 400, 420, 100, 100, po.RIGHT, True, 64, 8),
              (24, 130, 140, 16, -1, po.SCORE_ONLY, False, 8, 18)]


def scan_positions(G, tl):
    """Where k2a_scan_codes can go wrong: the first and last byte of a lane's sixteen, the last byte of a round of G lanes and the first
    of the next, and the four tail lengths (the dword that holds the target's last bytes is masked by what is left of it)."""
    return sorted({p for p in (0, 15, 16, 16 * G - 1, 16 * G, tl - 4, tl - 3, tl - 2, tl - 1) if 0 <= p < tl})


def check_scan_boundaries(lib, setenv, delenv, ci):
    """Batches of one kernel class whose targets hold exactly ONE wildcard each, all at the same position (one batch per position of
    scan_positions): a look that misses that byte sends the wavefront-task to the plain body, which scores the row as an ordinary
    one.  Through make_batch and the flat entry.  Pair 5 of a flat batch holds no wildcard and the sequence behind its target in the
    arena (the next pair's query) starts with one: nothing past a target's end may count.  The plan says packed kernels with tn == 1,
    nothing is handed back, every pair equals the oracle."""
    n, ql, tl, w, zd, flag, dual, G, C = SCAN_CASES[ci]
    keys = ("KSW2AMD_DEFER", "KSW2AMD_LDSCODES", "KSW2AMD_SOLO", "KSW2AMD_TN", "KSW2AMD_SIMDS")
    for k in keys:
        delenv(k, raising=False)
    setenv("KSW2AMD_SIMDS", "0")
    q, t = synth.fixed_batch(7300 + ci, n, ql, tl, sub=0.05, ind=0.06)
    try:
        for at in scan_positions(G, tl):
            qs, ts = [np.array(x, dtype=np.uint8) for x in q], [np.array(x, dtype=np.uint8) for x in t]
            for x in ts:
                x[at] = 4
            r0 = lib.rerun_count()
            p = lib.make_batch(qs, ts, MAT, 4, 2, 24, 1, w=w, zdrop=zd, flag=flag).plan(dual)
            d = p.describe()
            p.close()
            assert d and all(k["kernel"] == "pk" and k["tn"] == 1 and (k["G"], k["C"]) == (G, C) for k in d), (ci, at, d)
            check_batch(lib, dual, qs, ts, MAT, 4, 2, 24, 1, w=w, zdrop=zd, flag=flag)
            ts[5][at] = t[5][at]
            qs[6][0] = 4
            fb = lib.make_flat_batch(qs, ts, MAT, 4, 2, 24, 1, w=w, zdrop=zd, end_bonus=0, flag=flag)
            assert fb.arena[int(fb.toff[5]) + tl] == 4 and not (fb.arena[int(fb.toff[5]):int(fb.toff[5]) + tl] > 3).any()
            p = fb.plan(dual)
            d = p.describe()
            p.close()
            assert d and all(k["kernel"] == "pk" and k["tn"] == 1 and (k["G"], k["C"]) == (G, C) for k in d), (ci, at, "flat", d)
            fres = fb.run_oneshot(dual)
            exp = oracle_batch(dual, qs, ts, MAT, 4, 2, 24, 1, w, zd, 0, flag)
            bad = [(i, diff(exp[i], fres[i])) for i in range(n) if diff(exp[i], fres[i])]
            assert not bad, (ci, at, "flat", bad[:3])
            assert lib.rerun_count() == r0, (ci, at, lib.rerun_count() - r0)
    finally:
        for k in keys:
            delenv(k, raising=False)
