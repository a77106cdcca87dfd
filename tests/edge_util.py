"""Shared edge checks for the simulator tier and the GPU tier: Z-drop at its critical threshold through every kernel family, and
the packed-int16 score window at the plan's own admission boundary.  Everything is compared with the oracle, every ksw_extz_t
field and the CIGAR; which kernel ran is read from the plan's description, never assumed.

Z* (critical_zdrop) is the smallest zdrop >= 0 for which the oracle does not drop, found by bisection on the oracle alone (dropping
is monotone in the threshold).  At Z* the deciding row sits exactly on the threshold, so a `>` that became `>=` in any copy of the
test `max - H > zdrop + skew * slope` shows up as a different record.  The boundaries of part B are found by bisection on
plan.describe() / packed_pairs(), so that the test follows the host's proofs instead of restating them."""
import numpy as np

import ksw2_amd as ka
from ksw2_amd import synth
from oracle import pyoracle as po
from tests.parity_util import diff, CMP_FIELDS

COMPAT = ka.KSW2AMD_EZ_SSE_COMPAT
ENV_KEYS = ("KSW2AMD_NO_PK", "KSW2AMD_NO_RB", "KSW2AMD_DEFER", "KSW2AMD_SOLO", "KSW2AMD_NO_PKMP", "KSW2AMD_SIMDS", "KSW2AMD_UNIFORM",
            "KSW2AMD_STREAM_PIECE_KB", "KSW2AMD_EXTF_GRP", "KSW2AMD_EXTF_LDS", "KSW2AMD_EXTF_WIN", "KSW2AMD_EXTF_HBM", "KSW2AMD_EXTS_BIG",
            "KSW2AMD_EXTS_REG", "KSW2AMD_TN", "KSW2AMD_PK_FIRST", "KSW2AMD_EXTF_LANE", "KSW2AMD_EXTF_RING", "KSW2AMD_SSEC_BLK", "KSW2AMD_SSEC_HBM")


def set_env(setenv, delenv, env):
    for k in ENV_KEYS:
        delenv(k, raising=False)
    setenv("KSW2AMD_SIMDS", "0")
    for k, v in env.items():
        setenv(k, str(v))


# ---------------------------------------------------------------- Z*: bisection on the oracle

def critical_zdrop(dropped, hi=1 << 12, cache=None, key=None):
    """Smallest z >= 0 with dropped(z) false, or None when the pair does not drop at z = 0 (nothing to decide) or still drops at
    2**20.  dropped(z) -> bool runs the oracle; `cache` (a dict, per test) keeps the answer under `key`."""
    if cache is not None and key in cache:
        return cache[key]
    z = None
    if dropped(0):
        while dropped(hi) and hi < (1 << 20):
            hi *= 2
        if not dropped(hi):
            lo = 0                                  # dropped(lo), not dropped(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if dropped(mid):
                    lo = mid
                else:
                    hi = mid
            z = hi
    if cache is not None:
        cache[key] = z
    return z


def oracle_ext(func, qs, ts, mat, q, e, q2, e2, w, flag, end_bonus=0, m=None):
    """one-argument oracle runner per pair: run(i, zdrop) -> record of po.align(\"oracle\", func, ...)"""
    return lambda i, z: po.align("oracle", func, qs[i], ts[i], mat, q, e, q2, e2, w=int(np.broadcast_to(w, len(qs))[i]), zdrop=int(z),
                                 end_bonus=end_bonus, flag=int(np.broadcast_to(flag, len(qs))[i]), m=m)


def zstar_pairs(run, qs, ts, cache, tag, need=None):
    """Z* of every pair (None dropped); returns (qs, ts, zs) of the pairs that have one, each pair twice: at Z* and at Z* - 1."""
    oq, ot, oz = [], [], []
    for i in range(len(qs)):
        z = critical_zdrop(lambda zz: run(i, zz)["zdropped"] == 1, cache=cache, key=(tag, i))
        if z is None or z == 0:
            continue
        oq += [qs[i], qs[i]]; ot += [ts[i], ts[i]]; oz += [z, z - 1]
    if need is not None:
        assert len(oz) >= 2 * need, (tag, len(oz) // 2, need)
    return oq, ot, np.array(oz, dtype=np.int64)


# ---------------------------------------------------------------- pairs whose deciding row lies off the maximum's diagonal

def _rand(rng, n):
    return rng.integers(0, 4, int(n), dtype=np.uint8)


def indel_pair(rng, pre, indel, tail, run=20, in_target=None, sub=0.0):
    """A matching prefix, an indel of `indel` bases, a short matching run (too short to pay for the gap: the maximum stays at the
    prefix's end), then unrelated tails."""
    base = _rand(rng, pre + run)
    ins = _rand(rng, indel)
    q = np.concatenate([base[:pre], base[pre:], _rand(rng, tail)])
    t = np.concatenate([base[:pre], ins, base[pre:], _rand(rng, tail + int(rng.integers(-5, 6)))])
    if sub:
        mm = rng.random(len(q)) < sub
        q[mm] = rng.integers(0, 4, int(mm.sum()), dtype=np.uint8)
    if in_target is None:
        in_target = rng.random() < 0.5
    return (q, t) if in_target else (t, q)


def tandem_pair(rng, pre, unit, copies_q, copies_t, tail):
    """A prefix, then a tandem repeat of a short unit with different copy numbers in query and target (tied row maxima), then
    unrelated tails."""
    p, u = _rand(rng, pre), _rand(rng, unit)
    q = np.concatenate([p, np.tile(u, copies_q), _rand(rng, tail)])
    t = np.concatenate([p, np.tile(u, copies_t), _rand(rng, tail + int(rng.integers(-3, 4)))])
    return q, t


def wildcard_pair(rng, pre, tail):
    """A matching prefix with runs of the query wildcard (4), an indel, then unrelated tails."""
    q, t = indel_pair(rng, pre, int(rng.integers(1, 12)), tail, in_target=True, sub=0.02)
    for _ in range(int(rng.integers(1, 4))):
        at, ln = int(rng.integers(0, max(1, len(q) - 8))), int(rng.integers(1, 8))
        q[at:at + ln] = 4
    return q, t


def zdrop_pairs(seed, n, scale=1.0):
    """n pairs of the three builders, lengths about `scale` times 100 .. 600."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for k in range(n):
        pre, tail = int(rng.integers(60, 400) * scale) + 10, int(rng.integers(40, 200) * scale) + 10
        kind = k % 3
        if kind == 0:
            out.append(indel_pair(rng, pre, int(rng.integers(1, 21)), tail, run=int(rng.integers(4, 30))))
        elif kind == 1:
            out.append(tandem_pair(rng, pre, int(rng.integers(2, 7)), int(rng.integers(3, 12)), int(rng.integers(3, 12)), tail))
        else:
            out.append(wildcard_pair(rng, pre, tail))
    return [p[0] for p in out], [p[1] for p in out]


def same_shape(qs, ts, minlen=0):
    """The same pairs padded with unrelated bases to one square shape (at least `minlen`): the packed classes need pairs of one shape,
    and a square one keeps the corner inside every band."""
    rng = np.random.Generator(np.random.PCG64(len(qs)))
    ql = tl = max([minlen] + [len(x) for x in qs] + [len(x) for x in ts])
    pad = lambda x, L: np.concatenate([x, _rand(rng, L - len(x))])[:L]       # noqa: E731
    return np.stack([pad(x, ql) for x in qs]), np.stack([pad(x, tl) for x in ts])


# ---------------------------------------------------------------- part A: Z-drop families

def _pk(d, **kv):
    return any(c["kernel"] == "pk" and all(c[k] == v for k, v in kv.items()) for c in d)


SMALL = (synth.simple_mat(5, 2, 4, -1), 4, 2, 24, 1)
BIG = (synth.simple_mat(5, 10, 12, 0), 12, 4, 40, 2)         # scores too large for the plain kernels from about 900 rows on: re-based
# (name, env, dual, flag, w, scoring, minimum length, check of the plan's description)

ZFAMILIES = [
    ("int32", {"KSW2AMD_NO_PK": 1}, True, 0, 60, SMALL, 0, lambda d: all(c["kernel"] in ("int32", "mp") for c in d)),
    ("int32-so", {"KSW2AMD_NO_PK": 1}, False, po.SCORE_ONLY, 30, SMALL, 0, lambda d: all(c["kernel"] in ("int32", "mp") for c in d)),
    ("pk-plain", {"KSW2AMD_NO_RB": 1, "KSW2AMD_DEFER": 0}, False, po.SCORE_ONLY, 40, SMALL, 0, lambda d: _pk(d, rebased=0)),
    ("pk-plain-cigar", {"KSW2AMD_NO_RB": 1}, True, po.RIGHT, 100, SMALL, 0, lambda d: _pk(d, rebased=0)),
    ("pk-rebased", {"KSW2AMD_DEFER": 0}, True, 0, 60, BIG, 1000, lambda d: _pk(d, rebased=1)),
    ("pk-rebased-so", {"KSW2AMD_DEFER": 0}, False, po.SCORE_ONLY, 150, BIG, 1000, lambda d: _pk(d, rebased=1)),
    ("defer", {"KSW2AMD_DEFER": 1}, False, po.SCORE_ONLY, 100, SMALL, 0, lambda d: _pk(d, form="defer")),
    ("defer-8-18", {"KSW2AMD_DEFER": 1}, False, po.SCORE_ONLY | po.EXTZ_ONLY, 20, SMALL, 0, lambda d: _pk(d, form="defer", G=8)),
    ("defer-rebased", {"KSW2AMD_DEFER": 1}, False, po.SCORE_ONLY, 100, BIG, 1000, lambda d: _pk(d, form="defer", rebased=1)),
    ("solo", {"KSW2AMD_SOLO": "all"}, True, 0, 64, SMALL, 0, lambda d: any(c["kernel"] == "solo" for c in d)),
    ("solo-so", {"KSW2AMD_SOLO": "all"}, False, po.SCORE_ONLY, 40, SMALL, 0, lambda d: any(c["kernel"] == "solo" for c in d)),
    ("pkmp", {}, True, po.SCORE_ONLY, -1, SMALL, 2100, lambda d: any(c["kernel"] == "pkmp" for c in d)),
    ("mp", {"KSW2AMD_NO_PKMP": 1}, False, 0, -1, SMALL, 2100, lambda d: any(c["kernel"] == "mp" for c in d)),
    ("approx", {}, False, po.APPROX_MAX | po.SCORE_ONLY, 40, SMALL, 0, lambda d: any(c["nomax"] == 1 for c in d)),
    ("approx-cigar", {}, True, po.APPROX_MAX, 60, SMALL, 0, lambda d: any(c["nomax"] == 1 for c in d)),
]


def check_zdrop_family(lib, setenv, delenv, fam, seed=1, npairs=12, scale=1.0, cache=None, flat=True):
    """One family of ZFAMILIES: every pair with a Z* at Z* and Z* - 1 in ONE batch (per-pair zdrop), through the pointer batch
    entry and (flat=True) the flat one.  Returns (#pairs at Z*, #of those the oracle drops at Z* - 1)."""
    name, env, dual, flag, w, scoring, minlen, want = fam
    cache = {} if cache is None else cache
    set_env(setenv, delenv, env)
    mat, q, e, q2, e2 = scoring
    if not dual:
        q2 = e2 = 0
    if minlen >= 2000:
        npairs = max(3, npairs // 2)
    qs, ts = zdrop_pairs(seed, npairs, scale)
    qs, ts = same_shape(qs, ts, minlen)
    func = "extd2" if dual else "extz2"
    zflag = flag & ~po.APPROX_MAX                        # APPROX_MAX ignores zdrop (the exact mode's Z* is the edge it must ignore)
    run = oracle_ext(func, qs, ts, mat, q, e, q2, e2, w, zflag)
    qq, tt, zs = zstar_pairs(run, qs, ts, cache, (name, seed, npairs, scale), need=npairs // 3)
    if zs.size % 4:                                      # an even number of pairs of one shape: nobody is left without a partner
        qq, tt, zs = qq[:-2], tt[:-2], zs[:-2]
    qq, tt = np.stack(qq), np.stack(tt)
    b = lib.make_batch(qq, tt, mat, q, e, q2, e2, w=w, zdrop=zs, flag=flag)
    p = b.plan(dual)
    d = p.describe()
    p.close()
    assert want(d), (name, d)
    exp = [po.align("oracle", func, qq[i], tt[i], mat, q, e, q2, e2, w=w, zdrop=int(zs[i]), flag=flag) for i in range(len(zs))]
    res = b.run_oneshot(dual)
    bad = [(i, int(zs[i]), diff(exp[i], res[i])) for i in range(len(zs)) if diff(exp[i], res[i])]
    assert not bad, (name, "batch", bad[:4])
    if flat:
        fres = lib.make_flat_batch(qq, tt, mat, q, e, q2, e2, w=w, zdrop=zs, end_bonus=0, flag=flag).run_oneshot(dual)
        bad = [(i, int(zs[i]), diff(exp[i], fres[i])) for i in range(len(zs)) if diff(exp[i], fres[i])]
        assert not bad, (name, "flat", bad[:4])
    ndrop = sum(exp[i]["zdropped"] for i in range(1, len(zs), 2))
    assert all(exp[i]["zdropped"] == 0 for i in range(0, len(zs), 2)) and (flag & po.APPROX_MAX or ndrop == len(zs) // 2), (name, ndrop)
    return len(zs) // 2, ndrop


def check_zdrop_sse(lib, seed=3, npairs=12, scale=1.0, cache=None):
    """SSE-compatible mode: the reference's anti-diagonal Z-drop, its own Z*, both gap models, score-only and CIGAR."""
    cache = {} if cache is None else cache
    mat = synth.simple_mat(5, 2, 4, -1)
    qs, ts = zdrop_pairs(seed, npairs, scale)
    n = 0
    for dual, flag, w in ((False, 0, 50), (True, po.SCORE_ONLY, 80), (True, po.RIGHT, -1), (False, po.SCORE_ONLY, 20)):
        func = "extd2_sse" if dual else "extz2_sse"
        run = oracle_ext(func, qs, ts, mat, 4, 2, 24, 1, w, flag)
        qq, tt, zs = zstar_pairs(run, qs, ts, cache, ("sse", dual, flag, seed), need=npairs // 3)
        fl = np.full(len(zs), flag | COMPAT)
        d = lib.make_batch(qq, tt, mat, 4, 2, 24, 1, w=w, zdrop=zs, flag=fl).sse_plan(dual)
        assert any(c["kernel"] == "ssec" for c in d.describe()), d.describe()
        d.close()
        res = lib.extd_batch(qq, tt, mat, 4, 2, 24, 1, w=w, zdrop=zs, flag=fl) if dual else lib.extz_batch(qq, tt, mat, 4, 2, w=w, zdrop=zs, flag=fl)
        for i in range(len(zs)):
            exp = po.align("oracle", func, qq[i], tt[i], mat, 4, 2, 24, 1, w=w, zdrop=int(zs[i]), flag=flag)
            assert exp["zdropped"] == i % 2 and not diff(exp, res[i]), ("sse", dual, flag, i, int(zs[i]), diff(exp, res[i]))
        n += len(zs) // 2
    return n


def check_zdrop_exts(lib, setenv, delenv, seed=5, npairs=12, scale=1.0, cache=None):
    """ksw_exts2_sse: Z* of the splice-aware extension under each of its kernel forms."""
    cache = {} if cache is None else cache
    mat = synth.simple_mat(5, 1, 2, 0)
    qs, ts = zdrop_pairs(seed, npairs, scale)
    n = 0
    for env, flag, forms in (({}, po.SPLICE_FOR, {"exts-win8", "exts-win16"}), ({"KSW2AMD_EXTS_BIG": 1}, 0, {"exts-hbm"}),
                             ({"KSW2AMD_EXTS_REG": 1}, po.SPLICE_REV | po.SCORE_ONLY, {"exts-win16"})):
        set_env(setenv, delenv, env)
        run = lambda i, z: po.exts2("oracle", qs[i], ts[i], mat, 2, 1, 32, 4, zdrop=int(z), flag=flag)      # noqa: E731
        qq, tt, zs = zstar_pairs(run, qs, ts, cache, ("exts", flag, seed), need=npairs // 3)
        p = lib.make_splice_batch(qq, tt, mat, 2, 1, 32, 4, zdrop=zs, flag=flag).plan()
        kinds = {c["kernel"] for c in p.describe()}
        p.close()
        assert kinds and kinds <= forms, (env, kinds)
        res = lib.exts_batch(qq, tt, mat, 2, 1, 32, 4, zdrop=zs, flag=flag)
        for i in range(len(zs)):
            exp = po.exts2("oracle", qq[i], tt[i], mat, 2, 1, 32, 4, zdrop=int(zs[i]), flag=flag)
            assert exp["zdropped"] == i % 2 and not diff(exp, res[i]), ("exts", env, i, int(zs[i]), diff(exp, res[i]))
        n += len(zs) // 2
    return n


def check_zdrop_extf(lib, setenv, delenv, seed=7, npairs=12, scale=1.0, cache=None):
    """ksw_extf2_sse: the critical X-drop under each form its tests force."""
    cache = {} if cache is None else cache
    qs, ts = zdrop_pairs(seed, npairs, scale)
    qs = [np.minimum(x, 3) for x in qs]                 # (extf: no wildcard code)
    forms = (({"KSW2AMD_EXTF_GRP": 2}, 40, "extf-grp"), ({"KSW2AMD_EXTF_GRP": 0, "KSW2AMD_EXTF_LDS": 1}, 60, "extf-lds"),
             ({"KSW2AMD_EXTF_GRP": 0, "KSW2AMD_EXTF_WIN": 1}, 20, "extf-win"), ({"KSW2AMD_EXTF_GRP": 0, "KSW2AMD_EXTF_HBM": 1}, 100, "extf-hbm"),
             ({}, -1, "extf"))
    n = 0
    for env, w, kind in forms:
        set_env(setenv, delenv, env)
        run = lambda i, z: po.extf2("oracle", qs[i], ts[i], 2, -4, 2, w, int(z))       # noqa: E731
        qq, tt, zs = zstar_pairs(run, qs, ts, cache, ("extf", w, seed), need=npairs // 3)
        p = lib.make_linear_batch(qq, tt, 2, -4, 2, w=w, xdrop=zs).plan()
        kinds = {c["kernel"] for c in p.describe()}
        p.close()
        assert kinds and all(k.startswith(kind) for k in kinds), (kind, kinds)
        res = lib.extf_batch(qq, tt, 2, -4, 2, w=w, xdrop=zs)
        for i in range(len(zs)):
            exp = po.extf2("oracle", qq[i], tt[i], 2, -4, 2, w, int(zs[i]))
            assert exp["zdropped"] == i % 2 and not diff(exp, res[i], [f for f in CMP_FIELDS if f != "cigar"]), ("extf", kind, i, int(zs[i]))
        n += len(zs) // 2
    return n


def check_zdrop_small_calls(lib, seed=9, npairs=9, cache=None):
    """The host path for tiny single calls (KSW2AMD_SMALL_CELLS / ksw2amd_set_small_call_cells) at Z* and Z* - 1."""
    cache = {} if cache is None else cache
    mat = synth.simple_mat(5, 2, 4, -1)
    qs, ts = zdrop_pairs(seed, npairs, 0.5)
    lib.set_small_call_cells(1 << 40)
    n0, n = lib.small_call_count(), 0
    try:
        for dual, flag, w in ((False, 0, 40), (True, po.SCORE_ONLY, -1), (True, po.RIGHT, 60)):
            func = "extd2" if dual else "extz2"
            run = oracle_ext(func, qs, ts, mat, 4, 2, 24, 1, w, flag)
            qq, tt, zs = zstar_pairs(run, qs, ts, cache, ("small", dual, flag, seed), need=npairs // 3)
            for i in range(len(zs)):
                r = lib.extd2(qq[i], tt[i], mat, 4, 2, 24, 1, w=w, zdrop=int(zs[i]), flag=flag) if dual else lib.extz2(qq[i], tt[i], mat, 4, 2, w=w, zdrop=int(zs[i]), flag=flag)
                exp = po.align("oracle", func, qq[i], tt[i], mat, 4, 2, 24, 1, w=w, zdrop=int(zs[i]), flag=flag)
                assert exp["zdropped"] == i % 2 and not diff(exp, r), ("small", dual, i, int(zs[i]), diff(exp, r))
                n += 1
        assert lib.small_call_count() - n0 == n, (lib.small_call_count() - n0, n)
    finally:
        lib.set_small_call_cells(0)
    return n // 2


def check_zdrop_uniform(lib, setenv, delenv, n=2048, ql=150, tl=140, w=30, seed=11, sample=64):
    """A uniform plan has one zdrop: one pair's Z* and Z* - 1 for the whole batch, the deferred arg-max forced on and off; every
    pair against the oracle at `sample` positions and against the general path (KSW2AMD_UNIFORM=0) on all."""
    mat = synth.simple_mat(5, 2, 4, -1)
    rng = np.random.Generator(np.random.PCG64(seed))
    base = [indel_pair(rng, 100, 3 + k % 9, 60, run=12, in_target=k % 2 == 0) for k in range(16)]
    qs, ts = same_shape([b[0] for b in base], [b[1] for b in base])
    qs, ts = np.ascontiguousarray(qs[:, :ql]), np.ascontiguousarray(ts[:, :tl])
    fl = po.SCORE_ONLY
    z = None
    for k in range(16):
        z = critical_zdrop(lambda zz: po.align("oracle", "extz2", qs[k], ts[k], mat, 4, 2, w=w, zdrop=zz, flag=fl)["zdropped"] == 1)
        if z:
            break
    assert z, "no pair drops"
    reps = -(-n // 16)
    QS, TS = np.tile(qs, (reps, 1))[:n], np.tile(ts, (reps, 1))[:n]
    idx = sorted(set(range(0, n, max(1, n // sample))) | set(range(16)))
    ndrop = 0
    for zd in (z, z - 1):
        for defer in (1, 0):
            set_env(setenv, delenv, {"KSW2AMD_UNIFORM": 0, "KSW2AMD_DEFER": defer})
            off = lib.extz_batch(QS, TS, mat, 4, 2, w=w, zdrop=zd, flag=fl)
            set_env(setenv, delenv, {"KSW2AMD_UNIFORM": 1, "KSW2AMD_STREAM_PIECE_KB": 64, "KSW2AMD_DEFER": defer})
            s0 = lib.stream_stats()
            on = lib.extz_batch(QS, TS, mat, 4, 2, w=w, zdrop=zd, flag=fl)
            assert lib.stream_stats()["streamed_plans"] - s0["streamed_plans"] == 1, "the uniform plan did not run"
            bad = [i for i in range(n) if diff(off[i], on[i])]
            assert not bad, (zd, defer, bad[:4])
            for i in idx:
                exp = po.align("oracle", "extz2", QS[i], TS[i], mat, 4, 2, w=w, zdrop=zd, flag=fl)
                assert not diff(exp, on[i]), (zd, defer, i, diff(exp, on[i]))
                ndrop += exp["zdropped"]
    return ndrop


def check_zdrop_edges(lib, setenv, delenv, scale=1.0, npairs=12):
    """Part A on one library: every family of ZFAMILIES, SSE-compatible, exts, extf, small calls."""
    cache, out = {}, {}
    for k, fam in enumerate(ZFAMILIES):
        out[fam[0]] = check_zdrop_family(lib, setenv, delenv, fam, seed=100 + k, npairs=npairs, scale=scale, cache=cache)
    set_env(setenv, delenv, {})
    out["sse"] = check_zdrop_sse(lib, npairs=npairs, scale=scale, cache=cache)
    out["exts"] = check_zdrop_exts(lib, setenv, delenv, npairs=npairs, scale=scale, cache=cache)
    out["extf"] = check_zdrop_extf(lib, setenv, delenv, npairs=npairs, scale=scale, cache=cache)
    set_env(setenv, delenv, {})
    out["small"] = check_zdrop_small_calls(lib, cache=cache)
    return out


# ---------------------------------------------------------------- part B: the packed score window at the plan's own boundary

# (match, mismatch, q, e, q2, e2): assembly-like scorings, e2 = 0, int8 extremes the SSE signatures' early rejects let through,
# e = 0, q = 0, smax + e = 0, and an all-zero matrix (no score bound: only the length bound keeps reads out)
WINDOW_SCORINGS = [(2, 4, 4, 2, 24, 1), (1, 19, 39, 3, 81, 1), (1, 9, 16, 2, 41, 1), (1, 4, 6, 2, 26, 1), (2, 8, 12, 2, 24, 1),
                   (1, 2, 2, 1, 32, 0), (100, 100, 50, 10, 100, 5), (2, 4, 4, 0, 24, 0), (2, 4, 0, 2, 0, 1), (0, 3, 4, 0, 10, 0),
                   (0, 0, 5, 0, 10, 0)]


def bisect_last(pred, lo, hi):
    """Largest x in [lo, hi] with pred(x), given pred(lo) and pred monotone (true, then false); hi if pred(hi)."""
    assert pred(lo), lo
    if pred(hi):
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def extreme_pairs(rng, n, ql, tl, w):
    """Pairs of one shape that drive H to the window's ends: identical, all-mismatch, a long match run followed by a gap of about w,
    a matching head with a random tail."""
    qs, ts = [], []
    for k in range(n):
        kind = k % 4
        t = rng.integers(0, 4, tl, dtype=np.uint8)
        if kind == 0:
            q = np.resize(t, ql)
        elif kind == 1:
            q, t = np.full(ql, 0, np.uint8), np.full(tl, 1, np.uint8)
        elif kind == 2:
            g = max(1, min(abs(w) if w >= 0 else tl // 4, tl // 2))
            head = int(rng.integers(tl // 4, tl // 2 + 1))
            q = np.resize(np.concatenate([t[:head], t[head + g:]]), ql)
        else:
            q = np.concatenate([t[:ql // 2], rng.integers(0, 4, ql, dtype=np.uint8)])[:ql]
        qs.append(q); ts.append(t)
    return np.stack(qs), np.stack(ts)


def _plan_info(lib, dual, qs, ts, mat, q, e, q2, e2, w, flag):
    p = lib.make_batch(qs, ts, mat, q, e, q2, e2, w=w, zdrop=-1, flag=flag).plan(dual)
    d, npk = p.describe(), p.packed_pairs()
    p.close()
    return d, npk


def _rb_ok(d, npk, n):
    return npk == n and bool(d) and all(c["kernel"] == "pk" and c["rebased"] == 1 for c in d)


def _run_both(lib, dual, qs, ts, mat, q, e, q2, e2, w, flag, tag):
    res = lib.extd_batch(qs, ts, mat, q, e, q2, e2, w=w, flag=flag) if dual else lib.extz_batch(qs, ts, mat, q, e, w=w, flag=flag)
    func = "extd2" if dual else "extz2"
    for i in range(len(qs)):
        exp = po.align("oracle", func, qs[i], ts[i], mat, q, e, q2, e2, w=w, flag=flag)
        assert not diff(exp, res[i]), (tag, i, diff(exp, res[i]))


def check_window_edges(lib, setenv, delenv, scorings=WINDOW_SCORINGS, max_len=2000, max_cells=3_000_000, npairs=8, seed=5):
    """For every scoring: the plain packed boundary in length (KSW2AMD_NO_RB=1), the re-based boundary in w with the first geometry
    forced to each of (16,8) / (64,8) / (64,16) (KSW2AMD_PK_FIRST), the solo boundary in w; at the boundary and one past it the form
    is asserted from the plan and every pair is compared with the oracle.  Shapes over max_len / band cells over max_cells are left to
    the GPU tier.  Returns {form: #pairs run at the boundary in that form}."""
    rng = np.random.Generator(np.random.PCG64(seed))
    seen = {}
    for si, (a, b, q, e, q2, e2) in enumerate(scorings):
        mat = synth.simple_mat(5, a, b, 0 if a == b == 0 else -1)
        for dual in (False, True):
            qq2, ee2 = (q2, e2) if dual else (0, 0)
            flag = [po.SCORE_ONLY, 0, po.RIGHT][(si + dual) % 3]
            # plain packed: bisect on the length (w = 16)
            set_env(setenv, delenv, {"KSW2AMD_NO_RB": 1, "KSW2AMD_DEFER": 0})
            probe = lambda L: _plan_info(lib, dual, *extreme_pairs(rng, 2, L, L, 16), mat, q, e, qq2, ee2, 16, flag)[1] == 2    # noqa: E731
            if probe(8):
                L = bisect_last(probe, 8, 70000)
                for LL, on in ((L, True), (L + 1, False)):
                    if LL * 33 > max_cells:
                        continue
                    qs, ts = extreme_pairs(rng, npairs, LL, LL, 16)
                    d, npk = _plan_info(lib, dual, qs, ts, mat, q, e, qq2, ee2, 16, flag)
                    assert (npk == npairs and _pk(d, rebased=0)) if on else npk == 0, (si, dual, "plain", LL, d)
                    _run_both(lib, dual, qs, ts, mat, q, e, qq2, ee2, 16, flag, (si, dual, "plain", LL))
                    if on:
                        seen["plain"] = seen.get("plain", 0) + npairs
                lreb = L + 1
            else:
                lreb = 600
            # re-based: bisect on w (from 16 up) at a length the plain kernels refuse at w = 16, each first geometry
            for first in (1, 2, 3):
                set_env(setenv, delenv, {"KSW2AMD_PK_FIRST": first, "KSW2AMD_DEFER": 0})
                Lr = lreb
                if Lr > max_len:
                    continue
                probe = lambda w: _rb_ok(*_plan_info(lib, dual, *extreme_pairs(rng, 2, Lr, Lr, w), mat, q, e, qq2, ee2, w, flag), 2)    # noqa: E731
                if not probe(16):
                    continue
                W = bisect_last(probe, 16, Lr)
                for ww, on in ((W, True), (W + 1, False)):
                    if Lr * (2 * ww + 1) > max_cells:
                        continue
                    qs, ts = extreme_pairs(rng, npairs, Lr, Lr, ww)
                    d, npk = _plan_info(lib, dual, qs, ts, mat, q, e, qq2, ee2, ww, flag)
                    assert _rb_ok(d, npk, npairs) == on, (si, dual, first, Lr, ww, d)
                    if on:
                        key = "rb-C%d" % max(c["C"] for c in d if c["kernel"] == "pk")
                        seen[key] = seen.get(key, 0) + npairs
                    _run_both(lib, dual, qs, ts, mat, q, e, qq2, ee2, ww, flag, (si, dual, "rebased", first, ww))
            # solo: bisect on w
            set_env(setenv, delenv, {"KSW2AMD_SOLO": "all"})
            Ls = min(max(lreb, 300), max_len)
            probe = lambda w: any(c["kernel"] == "solo" for c in _plan_info(lib, dual, *extreme_pairs(rng, 2, Ls, Ls, w), mat, q, e, qq2, ee2, w, flag)[0])   # noqa: E731
            if probe(1):
                W = bisect_last(probe, 1, Ls)
                for ww, on in ((W, True), (W + 1, False)):
                    if Ls * (2 * ww + 1) > max_cells:
                        continue
                    qs, ts = extreme_pairs(rng, npairs, Ls, Ls, ww)
                    d, npk = _plan_info(lib, dual, qs, ts, mat, q, e, qq2, ee2, ww, flag)
                    assert any(c["kernel"] == "solo" for c in d) == on, (si, dual, "solo", ww, d)
                    if on:
                        seen["solo"] = seen.get("solo", 0) + npairs
                    _run_both(lib, dual, qs, ts, mat, q, e, qq2, ee2, ww, flag, (si, dual, "solo", ww))
    set_env(setenv, delenv, {})
    return seen


def check_slide_edges(lib, setenv, delenv, L=2100, npairs=4, seed=9):
    """Generation-serial packed class (pkmp): bisect along a scoring ladder (k, 2k, 2k, k, 12k, 1) for the last k the plan admits;
    run k and k + 1 (the int32 generation-serial kernels) against the oracle."""
    rng = np.random.Generator(np.random.PCG64(seed))
    set_env(setenv, delenv, {})
    sc = lambda k: (synth.simple_mat(5, k, 2 * k, -1), 2 * k, k, 12 * k, 1)           # noqa: E731
    probe = lambda k: any(c["kernel"] == "pkmp" for c in _plan_info(lib, True, *extreme_pairs(rng, 2, L, L, -1), *sc(k), -1, 0)[0])    # noqa: E731
    K = bisect_last(probe, 1, 10)
    assert K < 10, K
    for kk, on in ((K, True), (K + 1, False)):
        qs, ts = extreme_pairs(rng, npairs, L, L + 7, -1)
        mat, q, e, q2, e2 = sc(kk)
        d, _ = _plan_info(lib, True, qs, ts, mat, q, e, q2, e2, -1, po.SCORE_ONLY)
        assert any(c["kernel"] == "pkmp" for c in d) == on, (kk, d)
        _run_both(lib, True, qs, ts, mat, q, e, q2, e2, -1, po.SCORE_ONLY, ("pkmp", kk))
    return K


def check_target_wildcard_extremes(lib, setenv, delenv, seed=13):
    """A generic matrix with smax = 127 and a constant target-wildcard row of -128 (smax - sN = 255, the largest constant
    k2a_tn_fix takes off a candidate), targets with wildcard runs; plain packed kernels (asserted), every field against the oracle."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gm = np.full((5, 5), -20, dtype=np.int8)
    np.fill_diagonal(gm, [127, 90, 100, 60, 0])
    gm[4, :] = -128
    gm[:, 4] = gm[4, :]
    gm[3, 4] = gm[4, 3] = -128
    mat = gm.reshape(-1).copy()
    set_env(setenv, delenv, {})
    n = 0
    for dual, flag, L, w in ((False, po.SCORE_ONLY | po.GENERIC_SC, 40, 8), (True, po.GENERIC_SC, 60, 20), (False, po.GENERIC_SC | po.RIGHT, 70, 70)):
        qs = rng.integers(0, 4, (12, L), dtype=np.uint8)
        ts = qs.copy()
        for i in range(12):
            at = int(rng.integers(0, L - 3))
            ts[i, at:at + int(rng.integers(1, 4))] = 4
            if i % 3 == 0:
                ts[i, 0] = 4
            if i % 4 == 1:
                ts[i, -1] = 4
        q2, e2 = (80, 1) if dual else (0, 0)
        d, npk = _plan_info(lib, dual, qs, ts, mat, 62, 2, q2, e2, w, flag)        # (q + e = 64: the signatures' early reject lets -128 through)
        assert npk == 12 and d and all(c["kernel"] in ("pk", "solo") and c["tn"] == 1 for c in d), d
        _run_both(lib, dual, qs, ts, mat, 62, 2, q2, e2, w, flag, ("tn255", dual, flag))
        n += 12
    return n


# ---------------------------------------------------------------- part C: the reference's own answers at these edges

EDGE_KINDS = ["extz", "extd", "extz2_sse", "extd2_sse", "exts2", "extf2"]          # = oracle/gen_golden_edges.KINDS
EDGE_FIELDS = ["score", "max", "max_t", "max_q", "mqe", "mqe_t", "mte", "mte_q", "zdropped", "reach_end", "n_cigar"]


def edge_cases():
    """tests/golden/edge_cases.npz (oracle/gen_golden_edges.py) as a list of dicts."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_cases.npz"))
    out = []
    for k in range(len(z["params"])):
        kind, a, b, sc_n, gq, ge, gq2, ge2, w, zd, flag, zs = (int(v) for v in z["params"][k])
        so = z["seq_off"]
        exp = dict(zip(EDGE_FIELDS, (int(v) for v in z["expect"][k])))
        exp["cigar"] = [int(c) for c in z["cigar"][z["cigar_off"][k]:z["cigar_off"][k + 1]]]
        out.append(dict(kind=EDGE_KINDS[kind], a=a, b=b, mat=po.simple_mat(5, a, b, sc_n), gq=gq, ge=ge, gq2=gq2, ge2=ge2, w=w, zdrop=zd, flag=flag,
                        zstar=zs, q=z["seq"][so[2 * k]:so[2 * k + 1]], t=z["seq"][so[2 * k + 1]:so[2 * k + 2]], expect=exp))
    return out


def _edge_oracle(c):
    k = c["kind"]
    if k in ("extz", "extd"):
        return po.align("oracle", k, c["q"], c["t"], c["mat"], c["gq"], c["ge"], c["gq2"], c["ge2"], w=c["w"], zdrop=c["zdrop"], flag=c["flag"])
    if k in ("extz2_sse", "extd2_sse"):
        return po.align("oracle", k, c["q"], c["t"], c["mat"], c["gq"], c["ge"], c["gq2"], c["ge2"], w=c["w"], zdrop=c["zdrop"], flag=c["flag"])
    if k == "exts2":
        return po.exts2("oracle", c["q"], c["t"], c["mat"], c["gq"], c["ge"], c["gq2"], c["ge2"], zdrop=c["zdrop"], flag=c["flag"])
    return po.extf2("oracle", c["q"], c["t"], c["a"], -c["b"], c["ge"], c["w"], c["zdrop"])


def check_edge_golden_oracle():
    """The oracle against the reference's answers at Z* and Z* - 1 (every field and the CIGAR); returns #cases."""
    cs = edge_cases()
    for i, c in enumerate(cs):
        fields = EDGE_FIELDS if c["kind"] == "extf2" else EDGE_FIELDS + ["cigar"]
        got = _edge_oracle(c)
        assert not diff(c["expect"], got, fields), (i, c["kind"], c["zdrop"], diff(c["expect"], got, fields))
    assert len({c["kind"] for c in cs}) == 6 and sum(c["expect"]["zdropped"] for c in cs) == len(cs) // 2
    return len(cs)


def check_edge_golden(lib):
    """The library on the same cases: ksw_extz / ksw_extd through the scalar-named entry points, the ..2_sse cases as batches in the
    SSE-compatible mode, exts and extf batches per scoring."""
    groups = {}
    for c in edge_cases():
        groups.setdefault((c["kind"], c["a"], c["b"], c["gq"], c["ge"], c["gq2"], c["ge2"], c["mat"].tobytes()), []).append(c)
    n = 0
    for (kind, a, b, gq, ge, gq2, ge2, _), cs in groups.items():
        qs, ts, mat = [c["q"] for c in cs], [c["t"] for c in cs], cs[0]["mat"]
        w, zd = np.array([c["w"] for c in cs]), np.array([c["zdrop"] for c in cs])
        fields = EDGE_FIELDS + ["cigar"]
        if kind in ("extz", "extd"):                    # the scalar-named entry points (the ..2_sse signature would swap the pieces)
            res = [lib.extd(c["q"], c["t"], mat, gq, ge, gq2, ge2, w=c["w"], zdrop=c["zdrop"], flag=c["flag"]) if kind == "extd" else
                   lib.extz(c["q"], c["t"], mat, gq, ge, w=c["w"], zdrop=c["zdrop"], flag=c["flag"]) for c in cs]
        elif kind in ("extz2_sse", "extd2_sse"):
            fl = np.array([c["flag"] | COMPAT for c in cs])
            res = lib.extd_batch(qs, ts, mat, gq, ge, gq2, ge2, w=w, zdrop=zd, flag=fl) if kind.startswith("extd") else \
                lib.extz_batch(qs, ts, mat, gq, ge, w=w, zdrop=zd, flag=fl)
        elif kind == "exts2":
            res = lib.exts_batch(qs, ts, mat, gq, ge, gq2, ge2, zdrop=zd, flag=np.array([c["flag"] for c in cs]))     # (ge2: non-canonical penalty)
        else:
            res = lib.extf_batch(qs, ts, a, -b, ge, w=w, xdrop=zd)
            fields = EDGE_FIELDS
        for c, r in zip(cs, res):
            assert not diff(c["expect"], r, fields), (kind, a, b, c["w"], c["zdrop"], hex(c["flag"]), diff(c["expect"], r, fields))
            n += 1
    return n


# ---------------------------------------------------------------- GPU only: the headline shape

def check_headline_zdrop(lib, setenv, delenv, n=4096, L=10000, w=500, npairs=4, seed=17):
    """10 k x 10 k, w = 500, score only, single gap: a few pairs with their own Z* / Z* - 1, replicated to n pairs so that the plan's
    own rule (KSW2AMD_DEFER unset: at least 1.5 wavefronts per SIMD) picks the deferred arg-max; asserted from describe(), every pair
    against the oracle.
    """
    set_env(setenv, delenv, {})
    delenv("KSW2AMD_SIMDS", raising=False)
    mat = synth.simple_mat(5, 2, 4, -1)
    rng = np.random.Generator(np.random.PCG64(seed))
    base = [indel_pair(rng, int(rng.integers(4000, 8000)), int(rng.integers(1, 21)), L, run=int(rng.integers(4, 30)), in_target=k % 2 == 0, sub=0.02)
            for k in range(npairs)]
    qs, ts = same_shape([np.resize(b[0], L) for b in base], [np.resize(b[1], L) for b in base])
    fl = po.SCORE_ONLY
    zs = []
    for k in range(npairs):
        z = critical_zdrop(lambda zz: po.align("oracle", "extz2", qs[k], ts[k], mat, 4, 2, w=w, zdrop=zz, flag=fl)["zdropped"] == 1)
        assert z, k
        zs += [z, z - 1]
    reps = -(-n // (2 * npairs))
    QS = np.tile(np.repeat(qs, 2, axis=0), (reps, 1))[:n]
    TS = np.tile(np.repeat(ts, 2, axis=0), (reps, 1))[:n]
    ZD = np.tile(np.array(zs), reps)[:n]
    p = lib.make_batch(QS, TS, mat, 4, 2, w=w, zdrop=ZD, flag=fl).plan(False)
    d = p.describe()
    p.close()
    assert _pk(d, form="defer"), d
    res = lib.extz_batch(QS, TS, mat, 4, 2, w=w, zdrop=ZD, flag=fl)
    exp = {}
    for i in range(n):
        key = (i % (2 * npairs))
        if key not in exp:
            exp[key] = po.align("oracle", "extz2", QS[i], TS[i], mat, 4, 2, w=w, zdrop=int(ZD[i]), flag=fl)
        assert not diff(exp[key], res[i]), (i, int(ZD[i]), diff(exp[key], res[i]))
    assert sum(exp[k]["zdropped"] for k in exp) == npairs
    return d
