"""Shared by tests/test_plan_rerun_cpu.py (simulator build) and tests/test_gpu_plan_rerun.py (the real kernels): a resident plan
(ksw2amd_plan_create / _run / _fetch) run more than once must return what its first run returned.

lifecycle() takes plans that have been created and not run, with the oracle's records for them, through

  A  run, fetch, fetch_raw              every field (and the CIGAR where the mode has one) equals the oracle
  B  fetch again                        equals A: a fetch changes nothing a later fetch reads; rerun_count grows by the same amount again
  C  run, run, fetch, fetch_raw         equals A; the raw records on all 16 columns (rows_done, ti, tj included); timing() is sane
  C' (a second stream is given)         the first stream synchronised, one more run on the second stream, fetch, fetch_raw: equals A
  D  scrub, run, fetch, fetch_raw       equals A: one run alone writes everything a fetch reads
  E  scrub, fetch_raw                   the score column differs from A for every valid pair: the scrub took the records away, so D and
                                        C would have failed had a run done nothing.  (Asserted first, on the oracle's records: the score
                                        is non-zero -- for every pair where the case chooses its pairs, for nine in ten (three in four
                                        of a path-shape group) where the batch is a given one: ragged lengths from 1, 60-base pairs with
                                        random tails, planted paths; a pair whose true score is 0 must then differ from A in another
                                        column.)

With several plans every step is done plan by plan before the next step starts: every plan's run, then every plan's fetch -- the order in
which a caller that keeps one plan resident and pushes other batches through the same thread uses them.  describe() is read before A
and after C and must not change, except that a streamed plan whose launch gave up may have become an ordinary one (then the library's
aborted-run counter has grown; the helper returns that).

The cases: one plan per kernel class, at the smallest shapes the suite already uses for that class, each asserting its class from
describe().  Oracle records are computed once per case and process and shared by the tests (_ORACLE)."""
import numpy as np

import ksw2_amd as ka
from ksw2_amd import synth
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import form_edge_util as fe
from tests import hlopen_util as hu
from tests import trace_util as tu
from tests.parity_util import diff

FIELDS = list(ka.FIELDS)
RAW_SCORE = 8                                   # column of ksw2amd_plan_fetch_raw's records
NEG_INF = -0x40000000                           # KSW_NEG_INF
PRESET = (synth.simple_mat(5, 2, 4, -1), 4, 2, 24, 1)

_ORACLE = {}


def _memo(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


# ---------------------------------------------------------------- the lifecycle

def _same(tag, step, exp, got, fields, ref="oracle"):
    bad = [(i, diff(exp[i], got[i], fields)) for i in range(len(exp)) if diff(exp[i], got[i], fields)]
    assert not bad, (tag, "step " + step, "against " + ref, len(bad), bad[:4], [{k: (exp[i][k], got[i][k]) for k in d if k != "cigar"} for i, d in bad[:2]])


def _same_raw(tag, step, a, b):
    bad = np.flatnonzero((a != b).any(axis=1))
    assert len(bad) == 0, (tag, "step " + step, "raw records", len(bad), [(int(i), np.flatnonzero(a[i] != b[i]).tolist(), a[i].tolist(), b[i].tolist()) for i in bad[:3]])


def lifecycle(lib, plans, sync=None, stream2=None):
    """plans: [dict(tag=, plan=, expected=[oracle records], fields=[...], valid=[pairs that reach a kernel])].  Returns, per plan, whether
    a streamed launch was abandoned and the plan went on as an ordinary one."""
    for c in plans:
        assert c["valid"], c["tag"]
        zero = [i for i in c["valid"] if c["expected"][i]["score"] == 0]
        assert len(zero) <= c.get("zero_ok", 0) * len(c["valid"]), (c["tag"], "the oracle's score is 0: step E could not tell a scrubbed record from a written one", zero)
    ab0 = lib.stream_stats()["aborted_runs"]
    st = []
    for c in plans:
        st.append(dict(d0=c["plan"].describe()))
    # A
    for c in plans:
        c["plan"].run()
    for c, s in zip(plans, st):
        r0 = lib.rerun_count()
        s["A"] = c["plan"].fetch()
        s["nrerun"] = lib.rerun_count() - r0
        s["rawA"] = c["plan"].fetch_raw()
        _same(c["tag"], "A", c["expected"], s["A"], c["fields"])
        score = np.array([x["score"] for x in c["expected"]])[c["valid"]]
        raw = s["rawA"][c["valid"], RAW_SCORE]
        assert (raw == score).all(), (c["tag"], "step A raw score", np.flatnonzero(raw != score)[:5])
    # B
    for c, s in zip(plans, st):
        r0 = lib.rerun_count()
        again = c["plan"].fetch()
        assert lib.rerun_count() - r0 == s["nrerun"], (c["tag"], "step B: pairs run again by the fetch", lib.rerun_count() - r0, s["nrerun"])
        _same(c["tag"], "B", s["A"], again, c["fields"], "step A")
    # C
    for _ in range(2):
        for c in plans:
            c["plan"].run()
    for c, s in zip(plans, st):
        r0 = lib.rerun_count()
        got = c["plan"].fetch()
        assert lib.rerun_count() - r0 == s["nrerun"], (c["tag"], "step C: pairs run again by the fetch", lib.rerun_count() - r0, s["nrerun"])
        _same(c["tag"], "C", c["expected"], got, c["fields"])
        _same(c["tag"], "C", s["A"], got, c["fields"], "step A")
        _same_raw(c["tag"], "C", s["rawA"], c["plan"].fetch_raw())
        fill_ms, total_ms = c["plan"].timing()
        assert 0 <= fill_ms <= total_ms, (c["tag"], "timing after step C", fill_ms, total_ms)
    out = []
    aborted = lib.stream_stats()["aborted_runs"] - ab0
    for c, s in zip(plans, st):
        d1 = c["plan"].describe()
        if d1 != s["d0"]:
            assert aborted > 0, (c["tag"], "describe() changed without an abandoned streamed launch", s["d0"], d1)
        out.append(d1 != s["d0"])
    # C': the same plans on another stream
    if stream2 is not None:
        sync()
        for c in plans:
            c["plan"].run(stream2)
        for c, s in zip(plans, st):
            got = c["plan"].fetch()
            _same(c["tag"], "C'", s["A"], got, c["fields"], "step A")
            _same_raw(c["tag"], "C'", s["rawA"], c["plan"].fetch_raw())
    # D
    for c in plans:
        c["plan"].scrub()
    for c in plans:
        c["plan"].run(stream2)
    for c, s in zip(plans, st):
        got = c["plan"].fetch()
        _same(c["tag"], "D", c["expected"], got, c["fields"])
        _same_raw(c["tag"], "D", s["rawA"], c["plan"].fetch_raw())
        c["last"] = got
    # E
    for c in plans:
        c["plan"].scrub()
    for c, s in zip(plans, st):
        raw = c["plan"].fetch_raw()
        same = [i for i in c["valid"] if (raw[i, RAW_SCORE] == s["rawA"][i, RAW_SCORE] and c["expected"][i]["score"] != 0) or (raw[i] == s["rawA"][i]).all()]
        assert not same, (c["tag"], "step E: records that survived the scrub", same[:8])
    return out


# ---------------------------------------------------------------- cases of ksw2amd_plan_create / _create_flat

def _oracle_batch(key, dual, qs, ts, sc, w, zdrop, end_bonus, flag, m=None):
    mat, q, e, q2, e2 = sc
    if not dual:
        q2 = e2 = 0
    n = len(qs)
    bc = lambda v: np.array(np.broadcast_to(np.asarray(v), (n,)))      # noqa: E731
    w, zdrop, end_bonus, flag = bc(w), bc(zdrop), bc(end_bonus), bc(flag)

    def run():
        out = []
        for i in range(n):
            x = po.align("oracle", "extd2" if dual else "extz2", qs[i], ts[i], mat, q, e, q2, e2, w=int(w[i]), zdrop=int(zdrop[i]), end_bonus=int(end_bonus[i]),
                         flag=int(flag[i]), m=m)
            out.append(x)
        return out
    return _memo(key, run)


def _case(name, env, dual, qs, ts, w, zdrop, flag, want, sc=PRESET, end_bonus=0, m=None, flat=False, device=False, packed=None, note=""):
    """One batch for ksw2amd_plan_create (or _create_flat: flat, from a host arena or a device copy of it).  want(d): the class check on
    describe(); packed: every pair must be a packed one."""
    return dict(name=name, env=env, dual=dual, qs=qs, ts=ts, w=w, zdrop=zdrop, flag=flag, want=want, sc=sc, end_bonus=end_bonus, m=m, flat=flat, device=device,
                packed=packed, note=note)


def _kern(kernel, **kv):
    return lambda d: bool(d) and all(c["kernel"] == kernel and all(c[k] == v for k, v in kv.items()) for c in d)


_GI = 3                                         # KSW2AMD_PK_FIRST index of (64, 16)
_PK64 = {"KSW2AMD_PK_FIRST": _GI, "KSW2AMD_SOLO": 0}
_ZW = 40                                        # the band of the critical Z-drop pair (tests/test_gpu_hlopen.py)


def _batch_64x16(scoring):
    from tests.test_gpu_hlopen import batch_64x16
    return batch_64x16(scoring)


def pk64_case(form):
    """(64, 16) score only under the preset scoring: targets of 1 025 and 2 053 rows, bands 0, 16, 17 and the widest, half of the pairs
    under Z-drop 60, wildcard runs in every second target, and the pair that drops at Z* - 1 and not at Z* (frozen book / third pass
    of the deferred fill)."""
    qs, ts, ws, zs = _batch_64x16("preset")
    defer, ldscodes = {"defer": (1, 1), "ldscodes": (0, 1), "registers": (0, 0)}[form]
    c = _case("pk64x16-" + form, dict(_PK64, KSW2AMD_DEFER=defer, KSW2AMD_LDSCODES=ldscodes), False, qs, ts, ws, zs, po.SCORE_ONLY,
              _kern("pk", G=64, C=16, mode="score", form=form, rebased=0, nomax=0), packed=True)
    c["critical"] = True
    return c


def pk_rebased_case():
    """the "deep" scoring (1 / -36, q 18, e 1) on the 1 025-row shape at w 100: the re-based (64, 16) kernel"""
    qs, ts, ws, zs = _batch_64x16("deep")
    idx = [i for i in range(len(qs) - 2) if len(ts[i]) == 1025 and ws[i] == 100]
    assert len(idx) == 2
    mat, m, q, e, q2, e2 = hu.SCORINGS["deep"][:6]
    return _case("pk64x16-rebased", dict(_PK64), False, [qs[i] for i in idx], [ts[i] for i in idx], 100, zs[idx], po.SCORE_ONLY,
                 _kern("pk", G=64, C=16, mode="score", rebased=1), sc=(mat, q, e, q2, e2), m=m, packed=True)


PK8_MODES = {"score": (False, po.SCORE_ONLY), "cigar": (False, 0), "right": (False, po.RIGHT), "right-rev": (False, po.RIGHT | po.REV_CIGAR),
             "2p-eqx": (True, po.EQX)}


def pk8_case(mode):
    """4 pairs of 512 x 512, w 64, KSW2AMD_PK_FIRST=0.  Score only that is (8, 18); that geometry has no traceback, so with a CIGAR the plan
    takes the first packed geometry that has one for this band, (16, 8) -- asserted as such."""
    dual, flag = PK8_MODES[mode]
    qs, ts = hu.pairs(8400, 4, 512, 512, 5, True, 100)
    want = _kern("pk", G=8, C=18, mode="score") if mode == "score" else _kern("pk", G=16, C=8, gaps=2 if dual else 1, mode="right" if flag & po.RIGHT else "left")
    return _case("pk8x18-" + mode, {"KSW2AMD_PK_FIRST": 0, "KSW2AMD_SOLO": 0}, dual, qs, ts, 64, 100, flag, want, packed=True)


SOLO_MODES = {"score": (False, po.SCORE_ONLY), "cigar": (False, 0), "2p-score": (True, po.SCORE_ONLY), "2p-cigar": (True, 0)}


def solo_case(mode):
    dual, flag = SOLO_MODES[mode]
    qs, ts = hu.pairs(8410, 3, 300, 290, 5, True, 100)
    return _case("solo-" + mode, {"KSW2AMD_SOLO": "all"}, dual, qs, ts, 64, 100, flag, _kern("solo", gaps=2 if dual else 1), packed=True)


# (KSW2AMD_NO_PK=1 at this shape: no int32 strip geometry holds an unbanded 2 300-column pair, the plan takes the int32 family's
#  generation-serial kernel, "mp", as under KSW2AMD_NO_PKMP=1 -- there with the packed classes' wildcard rule, here without;
#  the int32 strip kernels are int32_small_case)
SERIAL_KERNELS = {"pkmp": ("pkmp", {}), "mp": ("mp", {"KSW2AMD_NO_PKMP": 1}), "mp-nopk": ("mp", {"KSW2AMD_NO_PK": 1})}


def serial_case(kernel, mode):
    """2 pairs of 2 300 x 2 337, unbanded: the generation-serial classes, whose boundary scratch (d_bnd) is filled once, before the
    first run; score only, and two-piece with CIGAR under Z-drop 300"""
    dual, flag, zd = {"score": (False, po.SCORE_ONLY, -1), "2p-cigar": (True, 0, 300)}[mode]
    qs, ts = hu.pairs(8420, 2, 2300, 2337, 5, True, zd)
    return _case("%s-%s" % (kernel, mode), SERIAL_KERNELS[kernel][1], dual, qs, ts, -1, zd, flag, _kern(SERIAL_KERNELS[kernel][0]), packed=kernel == "pkmp")


def int32_small_case(mode):
    """KSW2AMD_NO_PK=1 at 512 x 512, w 64: the int32 strip kernels"""
    dual, flag = {"score": (False, po.SCORE_ONLY), "cigar": (False, 0)}[mode]
    qs, ts = hu.pairs(8400, 4, 512, 512, 5, True, 100)
    return _case("int32-512-" + mode, {"KSW2AMD_NO_PK": 1}, dual, qs, ts, 64, 100, flag, _kern("int32"))


def ragged_case(dual, serial):
    """the ragged batch of tests/test_host_pipeline.py (lengths 1 .. 260, mixed w, zdrop and flags) plus a pair without a query and one
    without a target: several classes in one plan, forked over the side streams (or in order under KSW2AMD_SERIAL=1), and two records
    that no kernel writes"""
    from tests.test_host_pipeline import _ragged
    qs, ts, w, zd, fl = _ragged(31, 60)
    qs = list(qs) + [np.zeros(0, np.uint8), np.array(qs[3])]
    ts = list(ts) + [np.array(ts[2]), np.zeros(0, np.uint8)]
    w, zd, fl = np.append(w, [20, -1]), np.append(zd, [-1, 50]), np.append(fl, [0, po.SCORE_ONLY])
    c = _case("ragged-%s-%s" % ("2p" if dual else "1p", "serial" if serial else "fork"), {"KSW2AMD_SERIAL": 1} if serial else {}, dual, qs, ts, w, zd, fl,
              lambda d: len(d) > 1, end_bonus=5)
    c["invalid"] = [60, 61]
    c["zero_ok"] = 0.1
    return c


STREAM_SHAPES = [(512, 60, 64, 10, -1, None), (96, 300, 290, 30, 40, 1)]      # the first two of test_uniform_plans, fewer pairs


def streamed_case(si, flat):
    """KSW2AMD_STREAM=1: a one-shape score-only batch as a streamed plan (the packed class as one queue launch whose wavefronts wait
    for the pieces of the upload), from host pointers and from a flat host arena; wildcards in a few queries and targets.
    (A uniform plan -- uniform=1, the 4-bit / 2-bit wire formats -- is built inside the batch entry points only and never handed to a
    caller: it runs once by construction and is no case here.)"""
    n, ql, tl, w, zd, defer = STREAM_SHAPES[si]
    qs, ts = synth.fixed_batch(9100 + si, n, ql, tl, sub=0.05, ind=0.06, tail_random_frac=0.3, tail_pairs=0.2)
    qs, ts = [np.array(x) for x in qs], [np.array(x) for x in ts]
    qs[5][ql // 2] = 4; ts[n // 2][tl // 3] = 4; ts[n - 1][0] = 4; qs[n - 2][0] = 4; qs[n - 2][ql - 1] = 4
    env = {"KSW2AMD_STREAM": 1, "KSW2AMD_STREAM_PIECE_KB": 64}
    if defer is not None:
        env["KSW2AMD_DEFER"] = defer
    c = _case("streamed-%dx%d-%s" % (ql, tl, "flat" if flat else "ptr"), env, False, qs, ts, w, zd, po.SCORE_ONLY | (po.EXTZ_ONLY if si % 2 else 0),
              _kern("pk", mode="score", uniform=0), end_bonus=7, flat=flat)
    c["streamed"] = True
    c["zero_ok"] = 0.1
    return c


def flat_device_case(mode):
    """FlatBatch.plan over a device copy of the arena: 512 x 512 with wildcards in every third query and every second target.  The
    arena goes up unscanned.  Query wildcards are scored in place, and so are target wildcards under the packed classes' wildcard-row
    rule; with that rule off (KSW2AMD_TN=0) the packed kernels hand the pairs with a target wildcard back and every fetch runs them
    again (rerun_count grows at every fetch)"""
    dual, flag = {"score": (False, po.SCORE_ONLY), "cigar": (False, 0)}[mode]
    qs, ts = hu.pairs(8400, 4, 512, 512, 5, True, 100)
    assert any((q > 3).any() for q in qs) and any((t > 3).any() for t in ts)
    c = _case("flat-device-" + mode, {"KSW2AMD_SOLO": 0, "KSW2AMD_TN": 0}, dual, qs, ts, 64, 100, flag, _kern("pk", tn=0), flat=True, device=True)
    c["reruns"] = True
    return c


def plan_cases():
    out = [pk64_case(f) for f in ("defer", "ldscodes", "registers")] + [pk8_case(m) for m in PK8_MODES] + [pk_rebased_case()]
    out += [solo_case(m) for m in SOLO_MODES]
    out += [serial_case(k, m) for k in SERIAL_KERNELS for m in ("score", "2p-cigar")] + [int32_small_case(m) for m in ("score", "cigar")]
    out += [ragged_case(False, False), ragged_case(False, True), ragged_case(True, False)]
    out += [streamed_case(si, flat) for si in (0, 1) for flat in (False, True)]
    out += [flat_device_case(m) for m in ("score", "cigar")]
    return out


PLAN_CASES = {}


def plan_case(name):
    if not PLAN_CASES:
        PLAN_CASES.update({c["name"]: c for c in plan_cases()})
    return PLAN_CASES[name]


# names only (parametrize ids): building the batches is left to the test that runs them
PLAN_CASE_NAMES = (["pk64x16-" + f for f in ("defer", "ldscodes", "registers")] + ["pk8x18-" + m for m in PK8_MODES] + ["pk64x16-rebased"] +
                   ["solo-" + m for m in SOLO_MODES] + ["%s-%s" % (k, m) for k in SERIAL_KERNELS for m in ("score", "2p-cigar")] +
                   ["int32-512-score", "int32-512-cigar", "ragged-1p-fork", "ragged-1p-serial", "ragged-2p-fork"] +
                   ["streamed-%dx%d-%s" % (s[1], s[2], f) for s in STREAM_SHAPES for f in ("ptr", "flat")] + ["flat-device-score", "flat-device-cigar"])


def open_plan(lib, setenv, delenv, c):
    """the case's switches set (they stay set: ksw2amd_plan_run reads them again), its oracle records, its plan with the class asserted
    from describe(); returns the entry for lifecycle() and a function that releases what the plan borrowed"""
    exp = _oracle_batch(("plan", c["name"]), c["dual"], c["qs"], c["ts"], c["sc"], c["w"], c["zdrop"], c["end_bonus"], c["flag"], c["m"])
    n = len(c["qs"])
    invalid = c.get("invalid", [])
    valid = [i for i in range(n) if i not in invalid]
    assert all(len(c["qs"][i]) == 0 or len(c["ts"][i]) == 0 for i in invalid) and all(len(c["qs"][i]) and len(c["ts"][i]) for i in valid)
    if c.get("critical"):                          # the last two pairs: a drop at Z* - 1, none at Z*
        assert [exp[-2]["zdropped"], exp[-1]["zdropped"]] == [1, 0], (c["name"], exp[-2], exp[-1])
    eu.set_env(setenv, delenv, c["env"])
    for k in ("KSW2AMD_SERIAL", "KSW2AMD_STREAM", "KSW2AMD_LDSCODES"):
        if k not in c["env"]:
            delenv(k, raising=False)
    for k, v in c["env"].items():
        setenv(k, str(v))
    mat, q, e, q2, e2 = c["sc"]
    if not c["dual"]:
        q2 = e2 = 0
    dev = None
    if c["flat"]:
        b = lib.make_flat_batch(c["qs"], c["ts"], mat, q, e, q2, e2, w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"], m=c["m"])
        if c["device"]:
            dev = lib.device_copy(b.arena)
            b = lib.make_flat_batch(c["qs"], c["ts"], mat, q, e, q2, e2, w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"], m=c["m"], device_base=dev)
    else:
        b = lib.make_batch(c["qs"], c["ts"], mat, q, e, q2, e2, w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"], m=c["m"])
    p = b.plan(c["dual"])

    def close():
        p.close()
        if dev is not None:
            lib.device_free(dev)
    try:
        d = p.describe()
        assert c["want"](d), (c["name"], d)
        if c["packed"]:
            assert p.packed_pairs() == n, (c["name"], p.packed_pairs(), n, d)
    except BaseException:
        close()
        raise
    return dict(tag=c["name"], plan=p, expected=exp, fields=FIELDS + ["cigar"], valid=valid, zero_ok=c.get("zero_ok", 0)), close


def run_plan_cases(lib, setenv, delenv, names, sync=None, stream2=None):
    """the lifecycle over the named cases, their plans alive together (one name: the usual case); the cases must agree on their switches"""
    cs = [plan_case(n) for n in names]
    assert all(c["env"] == cs[0]["env"] for c in cs), names
    ents, closers = [], []
    try:
        for c in cs:
            ent, close = open_plan(lib, setenv, delenv, c)
            ents.append(ent); closers.append(close)
        s0, r0 = lib.stream_stats()["streamed_plans"], lib.rerun_count()
        changed = lifecycle(lib, ents, sync, stream2)
        for c, ch in zip(cs, changed):
            if c.get("streamed"):
                assert lib.stream_stats()["streamed_plans"] > s0, (c["name"], "no run of the plan was a streamed one")
            else:
                assert not ch, c["name"]
            if c.get("reruns"):
                assert lib.rerun_count() > r0, c["name"]
        return changed
    finally:
        for close in closers:
            close()
        eu.set_env(setenv, delenv, {})
        for k in ("KSW2AMD_SERIAL", "KSW2AMD_STREAM", "KSW2AMD_LDSCODES"):
            delenv(k, raising=False)


# ---------------------------------------------------------------- exts / extf / ssec: one group per kernel form (form_edge_util)

def form_groups():
    """{form of form_edge_util.WANTS: the cases of its smallest group (by cells)}"""
    def build():
        exts = fe.exts_cases(zstar=False)
        cases = fe.with_env(exts, fe.E_NONE) + fe.with_env([c for c in exts if c["ncol"] <= 448], fe.E_REG) + fe.with_env([c for c in exts if c["ncol"] <= 448], fe.E_BIG)
        cases += fe.extf_tier_cases() + fe.extf_window_cases() + fe.extf_group_cases(ntask={"extf-grp": 3, "extf-grp32": 1, "extf-grp64": 1, "extf-lds": 1})
        cases += fe.extf_lane_cases() + fe.ssec_lds_cases() + fe.ssec_blk_cases()
        groups = {}
        for c in cases:
            groups.setdefault((c["fam"], c["env"], c["want"], c["grp"], c["jb"], c["dual"], c["m"], c["sc"]), []).append(c)
        best = {}
        for key, cs in groups.items():
            cost = sum(len(c["q"]) * len(c["t"]) for c in cs)
            if key[2] not in best or cost < best[key[2]][0]:
                best[key[2]] = (cost, cs)
        assert set(best) == set(fe.WANTS), sorted(set(fe.WANTS) - set(best))
        return {k: v[1] for k, v in best.items()}
    return _memo("form-groups", build)


def run_form_group(lib, setenv, delenv, want, sync=None, stream2=None):
    """The form's group as form_edge_util.run_cases handles one group -- its switches, ONE plan from form_edge_util._plan, the form
    asserted from that plan's describe(), expected() as the reference, the same fields -- with the lifecycle where run_cases runs
    and fetches once.  (run_cases itself is left as it is; its single-run callers are unchanged.)  Returns {form key: #pairs}."""
    cs = form_groups()[want]
    c0 = cs[0]
    fam, env = c0["fam"], c0["env"]
    exp = [fe.expected(c) for c in cs]
    fields = fe.FIELDS if fam == "extf" else fe.FIELDS + ["cigar"]
    valid = [i for i in range(len(cs)) if exp[i]["score"] != 0]
    assert len(valid) * 2 >= len(cs), (want, "too few pairs with a score for step E", [x["score"] for x in exp])
    eu.set_env(setenv, delenv, fe.ENVS[env])
    try:
        p = fe._plan(lib, cs)
        try:
            seen = fe._assert_form(fam, want, p.describe(), cs, (fam, fe.ENVS[env], c0["grp"]))
            assert lifecycle(lib, [dict(tag=want, plan=p, expected=exp, fields=fields, valid=valid)], sync, stream2) == [False]
        finally:
            p.close()
    finally:
        eu.set_env(setenv, delenv, {})
    assert sum(seen.values()) >= len(cs), (want, seen)
    return seen


# ---------------------------------------------------------------- the traceback walks: one group of the path-shape grid per walk form

def run_trace_form(lib, setenv, delenv, form, sync=None, stream2=None):
    """The "halves" group of the form's grid (thinned: a long insertion and a long deletion against a pure diagonal, both orders in a
    task) as trace_util.run_batch handles a group -- one pointer batch, its plan's describe() against trace_util.form_ok, the oracle
    on every field and the CIGAR -- with the lifecycle where run_batch runs and fetches once.  (run_batch closes its plan between
    the fetch and the comparison and takes no other "run and fetch" step; trace_util.py is left as it is.)"""
    eu.set_env(setenv, delenv, form["env"])
    try:
        tag, qs, ts, flag, zd, eb = [g for g in tu.grid_cases(form, thin=3) if g[0] == "halves"][0]
        gq, ge, gq2, ge2 = form["gaps"] if form["dual"] else (form["gaps"][0], form["gaps"][1], 0, 0)
        exp = _oracle_batch(("trace", form["name"]), form["dual"], qs, ts, (form["mat"], gq, ge, gq2, ge2), form["w"], zd, eb, flag)
        n = len(qs)
        fl = np.array(np.broadcast_to(np.asarray(flag), (n,)))
        b = lib.make_batch(qs, ts, form["mat"], gq, ge, gq2, ge2, w=form["w"], zdrop=zd, end_bonus=eb, flag=fl)
        p = b.plan(form["dual"])
        try:
            d = p.describe()
            assert tu.form_ok(form, d, qs, ts, fl), (form["name"], d)
            ent = dict(tag="trace-" + form["name"], plan=p, expected=exp, fields=FIELDS + ["cigar"], valid=list(range(n)), zero_ok=0.25)
            assert lifecycle(lib, [ent], sync, stream2) == [False]
        finally:
            p.close()
    finally:
        eu.set_env(setenv, delenv, {})
