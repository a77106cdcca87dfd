"""Shared form-boundary checks for the simulator tier and the GPU tier: the launch-time kernel forms of ksw_exts2_sse, ksw_extf2_sse
and the SSE-compatible mode, each run on both sides of the length / band threshold that admits it (ksw2_host_ext.c).

Every case names the switches it runs under and the form it expects.  run_cases() builds ONE plan per group of cases, reads the form
from that plan's describe(), asserts it, runs and fetches THAT plan, and compares every ksw_extz_t field (and the CIGAR where there is
one) with the oracle -- or, for the committed subset (tests/golden/form_edge_cases.npz, oracle/gen_golden_forms.py), with the
reference's own answers.  It returns {form: #pairs}; the callers assert the keys they expect.

Contents are seeded per case (never by draw order), so the CPU tier, the GPU tier and the generator see the same pairs.  Oracle
answers are kept in one module-level cache and shared by every test of a session."""
import os

import numpy as np

import ksw2_amd as ka
from oracle import pyoracle as po
from oracle.gen_golden_exts import SPLICE
from tests import edge_util as eu
from tests.parity_util import diff

COMPAT = ka.KSW2AMD_EZ_SSE_COMPAT
FIELDS = eu.EDGE_FIELDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "form_edge_cases.npz")
FAMS = ["exts", "extf", "ssec"]
# the switch sets a case may run under (index = env id in the committed file)
ENVS = [{}, {"KSW2AMD_EXTS_REG": 1}, {"KSW2AMD_EXTS_BIG": 1}, {"KSW2AMD_EXTF_LDS": 1}, {"KSW2AMD_EXTF_WIN": 1}, {"KSW2AMD_EXTF_GRP": 0},
        {"KSW2AMD_EXTF_LANE": 1, "KSW2AMD_EXTF_RING": 1}, {"KSW2AMD_SSEC_BLK": 0}]
E_NONE, E_REG, E_BIG, E_LDS, E_WIN, E_GRP0, E_LANE, E_BLK0 = range(8)
# what a case may expect (index = form id in the committed file); "!blk": any SSE-compatible form but the register one
WANTS = ["exts-win8", "exts-win16", "exts-hbm", "extf-lds", "extf-hbm", "extf-win4", "extf-win8", "extf-grp", "extf-grp32", "extf-grp64",
         "extf-lane/ldsring/64", "extf-lane/hbm/0", "hbm", "lds", "blk", "!blk"]

_ORACLE = {}


def _rng(*key):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(k) & 0xffffffff for k in key])))


def _rand(rng, n):
    return rng.integers(0, 4, int(n), dtype=np.uint8)


def _subs(rng, x, rate):
    x = np.array(x, dtype=np.uint8)
    mm = rng.random(len(x)) < rate
    x[mm] = rng.integers(0, 4, int(mm.sum()), dtype=np.uint8)
    return x


def _fit(rng, x, n):
    """x cut or padded with unrelated bases to n"""
    return np.concatenate([x, _rand(rng, max(0, n - len(x)))])[:n].astype(np.uint8)


# ---------------------------------------------------------------- 1. exts: the register windows

EXTS_SC = (1, 2, 0, 2, 1, 32, 4)                      # a, b, sc_n, q, e, q2, noncan
EXTS_NCOL = (447, 448, 449, 959, 960, 961)            # K2A_DM_DIAG(8) = 448, K2A_DM_DIAG(16) = 960: one below, at, one past
EXTS_D = (0, 1, 63, 64, 65, 200)                      # the longer sequence is ncol + d: from d >= 64 the window slides at full diagonal length
EXTS_FORM = {447: "exts-win8", 448: "exts-win8", 449: "exts-win16", 959: "exts-win16", 960: "exts-win16", 961: "exts-hbm"}
EXTS_MODES = [po.SCORE_ONLY, 0, po.RIGHT, po.RIGHT | po.REV_CIGAR, po.EXTZ_ONLY, po.GENERIC_SC]
EXTS_KINDS = ["copy", "intron", "lowc", "wild", "junc"]
EXTS_JB = 3


def exts_want(ncol, env):
    if env == E_BIG:
        return "exts-hbm"
    if env == E_REG and ncol <= 960:
        return "exts-win16"
    return EXTS_FORM[ncol]


def _copy_pair(rng, ncol, d):
    """(short, long): a noisy copy without the k bases after its middle, k chosen (up to d) so that the short sequence's last base
    aligns with position 64 * j of the long one: the last cell of the last full diagonal then sits where the window has just slid"""
    long_ = _rand(rng, ncol + d)
    k = min(d, (-(ncol - 1)) % 64)
    h = ncol // 2
    return _subs(rng, np.concatenate([long_[:h], long_[h + k:ncol + k]]), 0.03), long_


def _intron(rng, ql, tl, ncol):
    """target = exon, GT .. AG intron of more than 64 bases, exon; query = the two exons (then unrelated bases up to ql)"""
    t = _rand(rng, tl)
    ex1, intr = ncol // 3, 65 + int(rng.integers(0, 60))
    b = ex1 + intr
    t[ex1], t[ex1 + 1], t[b - 2], t[b - 1] = 2, 3, 0, 2
    return _fit(rng, _subs(rng, np.concatenate([t[:ex1], t[b:]]), 0.03), ql), t, ex1, b


def exts_content(kind, ncol, d, orient):
    """(query, target, junc or None) of one shape: orient 0 = the query is the shorter sequence, 1 = the target is"""
    rng = _rng(1, EXTS_KINDS.index(kind) if kind in EXTS_KINDS else 9, ncol, d, orient)
    ql, tl = (ncol, ncol + d) if orient == 0 else (ncol + d, ncol)
    junc = None
    if kind in ("copy", "wild"):
        short, long_ = _copy_pair(rng, ncol, d)
        q, t = (short, long_) if orient == 0 else (long_, short)
        if kind == "wild":
            for x in (q, t):
                for _ in range(3):
                    at, ln = int(rng.integers(0, len(x) - 8)), int(rng.integers(1, 8))
                    x[at:at + ln] = 4
            t[-1] = 4 if d % 2 else t[-1]
    elif kind in ("intron", "junc"):
        q, t, don, acc = _intron(rng, ql, tl, ncol)
        if kind == "junc":
            junc = (rng.integers(0, 16, tl, dtype=np.uint8) * (rng.random(tl) < 0.05)).astype(np.uint8)
            junc[don] |= 1
            junc[acc - 1] |= 2
    elif kind == "lowc":
        q, t = (rng.integers(0, 2, ql, dtype=np.uint8) * 2).astype(np.uint8), (rng.integers(0, 2, tl, dtype=np.uint8) * 2).astype(np.uint8)
    else:                                               # "drop": a matching head, then unrelated tails (has a Z*)
        long_ = _rand(rng, ncol + d)
        short = _fit(rng, _subs(rng, long_[:ncol * 11 // 20], 0.02), ncol)
        q, t = (short, long_) if orient == 0 else (long_, short)
    assert len(q) == ql and len(t) == tl and min(ql, tl) == ncol
    return q, t, junc


def _exts_case(kind, ncol, d, orient, flag, zdrop, gold=False):
    q, t, junc = exts_content(kind, ncol, d, orient)
    a, b, scn, gq, ge, gq2, nc = EXTS_SC
    return dict(fam="exts", q=q, t=t, junc=junc, jb=EXTS_JB if junc is not None else 0, flag=int(flag), zdrop=int(zdrop), w=-1, dual=0, m=5,
                sc=(a, b, scn, gq, ge, gq2, nc), ncol=ncol, gold=gold, grp=0, key=("exts", kind, ncol, d, orient, int(flag), int(zdrop)))


def exts_zstar(kind, ncol, d, orient, flag):
    """Z* of a shape (bisection on the oracle, edge_util.critical_zdrop)"""
    q, t, junc = exts_content(kind, ncol, d, orient)
    a, b, scn, gq, ge, gq2, nc = EXTS_SC
    mat = po.simple_mat(5, a, b, scn)
    return eu.critical_zdrop(lambda z: po.exts2("oracle", q, t, mat, gq, ge, gq2, nc, zdrop=int(z), flag=flag)["zdropped"] == 1,
                             cache=_ORACLE, key=("exts-z*", kind, ncol, d, orient, flag))


def exts_cases(ncols=EXTS_NCOL, rots=(0,), zstar=True):
    """The window grid: every shape of ncols x both orientations x EXTS_D, with `rots` rotations of (mode, splice flags, zdrop) per
    shape -- one rotation walks all six modes over the six d of every (ncol, orientation), six rotations are the full mode product --
    the five contents rotated over the shapes; with zstar, one diverging pair per ncol and orientation at its own Z* and Z* - 1."""
    out = []
    for ncol in ncols:
        ni = EXTS_NCOL.index(ncol)
        for oi in (0, 1):
            for di, d in enumerate(EXTS_D):
                k = (ni * 2 + oi) * 6 + di
                for rot in rots:
                    mode = EXTS_MODES[(di + oi + ni + rot) % 6]
                    flag = mode | SPLICE[(k // 2 + rot) % len(SPLICE)]
                    # committed subset: every mode at the two limits and one past them (d = 65: a sliding window), one mode elsewhere
                    gold = (d == 65 and oi == 0 and ncol in (448, 449, 960, 961)) or (rot == 0 and d in (0, 65))
                    out.append(_exts_case(EXTS_KINDS[(k + rot) % 5], ncol, d, oi, flag, (-1, 100)[(k + k // 6 + rot) % 2], gold))
            if zstar:
                flag = EXTS_MODES[(ni + oi) % 3] | po.SPLICE_FOR
                z = exts_zstar("drop", ncol, 65, oi, flag)
                assert z, ("no Z*", ncol, oi)
                out += [_exts_case("drop", ncol, 65, oi, flag, z, oi == 0), _exts_case("drop", ncol, 65, oi, flag, z - 1, oi == 0)]
    return out


def with_env(cases, env, want=None):
    """the same cases under another switch set; want: a form, or a function of the case"""
    out = []
    for c in cases:
        c = dict(c)
        c["env"] = env
        c["want"] = exts_want(c["ncol"], env) if want is None else want
        out.append(c)
    return out


# ---------------------------------------------------------------- 2. extf: LDS tiers, register windows, group forms, lane class

EXTF_SC = (2, -4, 2)
EXTF_XDROP = 60
EXTF_TIERS = (1024, 1025, 4096, 4097, 21504, 21505)   # EXTF_LDS_T0 / T1 / T2 and one past each


def extf_content(kind, ql, tl, tag):
    """a noisy copy with two small indels (kind "copy": runs to the end) or the same with an unrelated last 40 % (kind "tail": drops)"""
    rng = _rng(2, ql, tl, tag, kind == "tail")
    base = _rand(rng, max(ql, tl) + 8)
    t = base[:tl].copy()
    q = _subs(rng, base, 0.04)
    a, b = max(1, ql // 3), max(2, 2 * ql // 3)
    q = _fit(rng, np.concatenate([q[:a], q[a + 2:b], _rand(rng, 2), q[b:]]), ql)
    if kind == "tail":
        q[ql * 3 // 5:] = _rand(rng, ql - ql * 3 // 5)
    return q, t


def _extf_case(kind, ql, tl, w, xdrop, env, want, grp, tag=0, gold=False):
    q, t = extf_content(kind, ql, tl, tag)
    return dict(fam="extf", q=q, t=t, junc=None, jb=0, flag=0, zdrop=int(xdrop), w=int(w), dual=0, m=4, sc=(2, 4, 0, 0, 2, 0, 0), env=env, want=want,
                gold=gold, grp=grp, key=("extf", kind, ql, tl, int(w), int(xdrop), tag))


def _extf_variants(n):
    """n (content, xdrop) variants: both contents at X-drop -1 and at a value that drops the diverging one"""
    v = [("copy", -1), ("tail", EXTF_XDROP), ("tail", -1), ("copy", EXTF_XDROP)]
    return [v[i % 4] for i in range(n)]


def extf_tier_cases(tiers=EXTF_TIERS, thin=True):
    """tlen at every LDS tier limit and one past it, query of about the same length: unforced at w = 1000 (span 1001: no group form, no
    register window), KSW2AMD_EXTF_LDS=1 at w = 1000 and at w = 16.  thin: above 4097 two variants at w = 1000 instead of four."""
    out = []
    for ti, tl in enumerate(tiers):
        want = "extf-hbm" if tl > 21504 else "extf-lds"
        ql = tl + (5 if ti % 2 else -7)
        for env, w in ((E_NONE, 1000), (E_LDS, 1000), (E_LDS, 16)):
            nv = 2 if (thin and w == 1000 and tl > 5000) else 4
            for vi, (kind, xd) in enumerate(_extf_variants(nv)):
                out.append(_extf_case(kind, ql, tl, w, xd, env, want, ("tier", tl, env, w), vi, gold=(env == E_NONE and vi == 0) or (w == 16 and vi == 1)))
    return out


def extf_window_cases():
    """KSW2AMD_EXTF_WIN=1: spans 147 / 148 (K2A_EXTF_WIN_SPAN(4)) and 403 / 404 (.. (8)) through w, targets long enough for the window
    to slide; KSW2AMD_EXTF_GRP=0: the span-128 rule on a target of the first LDS tier, through w and through a short query."""
    out = []
    for span, want in ((147, "extf-win4"), (148, "extf-win8"), (403, "extf-win8"), (404, "extf-lds")):
        for vi, (kind, xd) in enumerate(_extf_variants(3)):
            out.append(_extf_case(kind, 3000 + vi, 3100, span - 1, xd, E_WIN, want, ("win", span), vi, gold=vi == 0))
    for span, want in ((128, "extf-lds"), (129, "extf-win4")):
        for vi, (kind, xd) in enumerate(_extf_variants(3)):
            out.append(_extf_case(kind, 990 + vi, 1000, span - 1, xd, E_GRP0, want, ("s128-w", span), vi, gold=vi == 0))
            out.append(_extf_case(kind, span, 1000 - vi, -1, xd, E_GRP0, want, ("s128-q", span), vi, gold=vi == 1))
    return out


EXTF_GROUPS = ((160, "extf-grp"), (161, "extf-grp32"), (416, "extf-grp32"), (417, "extf-grp64"), (928, "extf-grp64"), (929, "extf-lds"))


def extf_group_cases(ntask={"extf-grp": 7, "extf-grp32": 3, "extf-grp64": 3, "extf-lds": 2}):
    """Unforced: spans 160 / 161, 416 / 417, 928 / 929 (K2A_EXTFB_SPAN(16 / 32 / 64)), each reached through w, through a short query
    and through a short target (w = -1), the long side several rings long; one plan per (span, way) whose task count leaves the last
    wavefront's last group empty (four / two extensions per wavefront in extf-grp / extf-grp32)."""
    out = []
    for span, want in EXTF_GROUPS:
        for way in ("w", "q", "t"):
            for vi, (kind, xd) in enumerate(_extf_variants(ntask[want])):
                long_ = 3000 + 17 * vi
                ql, tl, w = {"w": (long_, 3050, span - 1), "q": (span, long_ + 50, -1), "t": (long_ + 50, span, -1)}[way]
                out.append(_extf_case(kind, ql, tl, w, xd, E_NONE, want, ("grp", span, way), vi, gold=vi == 0))
    return out


def extf_lane_cases():
    """KSW2AMD_EXTF_LANE=1, KSW2AMD_EXTF_RING=1: K2A_EXTF_RING_ROWS(span) rounded up to 4 crosses 64 rows between span 217 and 218,
    span = min(min(qlen, tlen) - 1, w): through w and through the shorter sequence; the other lanes of the group hold narrower bands."""
    out = []
    for span, want in ((217, "extf-lane/ldsring/64"), (218, "extf-lane/hbm/0")):
        for way in ("w", "q"):
            for vi, (kind, xd) in enumerate(_extf_variants(5)):
                ql, tl, w = (600 + vi, 640, span - 9 * vi) if way == "w" else (span + 1 - 7 * vi, 500 + vi, -1)
                out.append(_extf_case(kind, ql, tl, w, xd, E_LANE, want, ("lane", span, way), vi, gold=vi == 0))
    return out


# ---------------------------------------------------------------- 3. ssec: LDS / HBM, the register form and its exclusions

SSEC_SC = (2, 4, -1, 4, 2, 24, 1)


def ssec_content(ql, tl, tag, m=5):
    rng = _rng(3, ql, tl, tag, m)
    base = _rand(rng, max(ql, tl) + 16)
    t = base[:tl].copy()
    q = _subs(rng, base, 0.05)
    a, b = max(1, ql // 4), max(2, ql // 2)
    q = np.concatenate([q[:a], q[a + 3:b], _rand(rng, 5), q[b:]])
    q = _fit(rng, q, ql)
    if tag % 3 == 1:
        q[ql * 7 // 10:] = _rand(rng, ql - ql * 7 // 10)              # a diverging tail: Z-drop has something to decide
    if tag % 2:
        q[ql // 5:ql // 5 + 3] = m - 1                                # wildcards
        t[tl // 2] = m - 1
    if m > 5:
        t[tl // 3] = 4                                                # a sixth code: an ordinary residue of the 6-code matrix
    return q, t


def _ssec_case(dual, ql, tl, w, flag, zdrop, env, want, grp, tag=0, m=5, gold=False):
    q, t = ssec_content(ql, tl, tag, m)
    return dict(fam="ssec", q=q, t=t, junc=None, jb=0, flag=int(flag), zdrop=int(zdrop), w=int(w), dual=int(dual), m=m, sc=SSEC_SC, env=env, want=want,
                gold=gold, grp=grp, key=("ssec", dual, ql, tl, int(w), int(flag), int(zdrop), tag, m))


SSEC_MODES = (po.SCORE_ONLY, 0, po.RIGHT)


def ssec_lds_cases():
    """KSW2AMD_SSEC_BLK=0: (dual ? 11 : 9) * round_up(tlen, 16) <= 8192 -- the last LDS target is 896 (single) / 736 (dual); bands 20
    and -1; score only, CIGAR and right-aligned CIGAR."""
    out = []
    for dual, tls in ((0, (896, 897)), (1, (736, 737))):
        for ti, tl in enumerate(tls):
            for wi, w in enumerate((20, -1)):
                for mi, flag in enumerate(SSEC_MODES):
                    tag = mi + 3 * wi
                    out.append(_ssec_case(dual, tl + (13 if (mi + wi) % 2 else -11), tl, w, flag, (-1, 200)[(mi + wi + dual) % 2], E_BLK0, ("lds", "hbm")[ti],
                                          ("ssec-lds", dual, tl), tag, gold=(mi + wi) % 3 == 0))
    return out


def ssec_blk_cases():
    """Unforced: the register form's 960 positions (K2A_SSECB_SPAN) reached through w, through qlen and through tlen, and one past;
    the same shapes with KSW_EZ_GENERIC_SC and with a 6-code matrix, which the register form does not take."""
    out = []
    for dual in (0, 1):
        for span, want in ((960, "blk"), (961, "!blk")):
            for wi, way in enumerate(("w", "q", "t")):
                ql, tl, w = {"w": (1100, 1150, span - 1), "q": (span, 1150, -1), "t": (1150, span, -1)}[way]
                flag = SSEC_MODES[(wi + dual) % 3]
                zd = (-1, 300)[(wi + dual) % 2]
                out.append(_ssec_case(dual, ql, tl, w, flag, zd, E_NONE, want, ("ssec-blk", dual, span), wi, gold=True))
                out.append(_ssec_case(dual, ql, tl, w, flag | po.GENERIC_SC, zd, E_NONE, "!blk", ("ssec-generic", dual, span), wi, gold=span == 960 and wi == dual))
                out.append(_ssec_case(dual, ql, tl, w, flag, zd, E_NONE, "!blk", ("ssec-m6", dual, span), wi, m=6, gold=span == 960 and wi != dual))
    return out


# ---------------------------------------------------------------- running a list of cases

def _mat(c):
    a, b, scn = c["sc"][:3]
    return po.simple_mat(c["m"], a, b, scn)


def reference(c, which="oracle"):
    """one case through the oracle (or, in the generator, the compiled reference)"""
    a, b, scn, gq, ge, gq2, ge2 = c["sc"]
    if c["fam"] == "exts":
        return po.exts2(which, c["q"], c["t"], _mat(c), gq, ge, gq2, ge2, zdrop=c["zdrop"], junc_bonus=c["jb"], flag=c["flag"], junc=c["junc"])
    if c["fam"] == "extf":
        return po.extf2(which, c["q"], c["t"], a, -b, ge, c["w"], c["zdrop"])
    return po.align(which, "extd2_sse" if c["dual"] else "extz2_sse", c["q"], c["t"], _mat(c), gq, ge, gq2, ge2, w=c["w"], zdrop=c["zdrop"], flag=c["flag"], m=c["m"])


def expected(c):
    if "expect" in c:
        return c["expect"]
    if c["key"] not in _ORACLE:
        _ORACLE[c["key"]] = reference(c)
    return _ORACLE[c["key"]]


def _plan(lib, cs):
    c0 = cs[0]
    a, b, scn, gq, ge, gq2, ge2 = c0["sc"]
    qs, ts = [c["q"] for c in cs], [c["t"] for c in cs]
    zd, fl = np.array([c["zdrop"] for c in cs]), np.array([c["flag"] for c in cs])
    if c0["fam"] == "exts":
        return lib.make_splice_batch(qs, ts, _mat(c0), gq, ge, gq2, ge2, zdrop=zd, junc_bonus=c0["jb"], flag=fl, juncs=[c["junc"] for c in cs]).plan()
    if c0["fam"] == "extf":
        return lib.make_linear_batch(qs, ts, a, -b, ge, w=[c["w"] for c in cs], xdrop=zd).plan()
    return lib.make_batch(qs, ts, _mat(c0), gq, ge, gq2, ge2, w=np.array([c["w"] for c in cs]), zdrop=zd, flag=fl | COMPAT, m=c0["m"]).sse_plan(bool(c0["dual"]))


def _assert_form(fam, want, d, cs, tag):
    """the plan's description against the form the group expects; returns {count key: #pairs}"""
    n = len(cs)
    assert d and sum(c["tasks"] for c in d) == n, (tag, d, n)
    seen = {}
    if fam == "exts":
        assert {c["kernel"] for c in d} == {want}, (tag, want, d)
        assert sum(c["tasks"] for c in d if c["generic"]) == sum(1 for c in cs if c["flag"] & po.GENERIC_SC), (tag, d)
        assert sum(c["tasks"] for c in d if c["mode"] == "score") == sum(1 for c in cs if c["flag"] & po.SCORE_ONLY), (tag, d)
        assert sum(c["tasks"] for c in d if c["mode"] == "right") == sum(1 for c in cs if c["flag"] & po.RIGHT and not c["flag"] & po.SCORE_ONLY), (tag, d)
        for c in d:
            seen["%s/%s" % (c["kernel"], c["mode"])] = seen.get("%s/%s" % (c["kernel"], c["mode"]), 0) + c["tasks"]
    elif fam == "extf":
        kernel, form, ring = (want.split("/") + ["-", "0"])[:3]
        assert all(c["kernel"] == kernel and c["form"] == form and c["ring"] == int(ring) for c in d), (tag, want, d)
        seen[kernel] = n
        if form != "-":
            seen[want] = n
    else:
        gaps = 2 if cs[0]["dual"] else 1
        assert all(c["kernel"] == "ssec" and c["gaps"] == gaps for c in d), (tag, d)
        assert all(c["form"] != "blk" for c in d) if want == "!blk" else {c["form"] for c in d} == {want}, (tag, want, d)
        for c in d:
            seen["%s/%d" % (c["form"], gaps)] = seen.get("%s/%d" % (c["form"], gaps), 0) + c["tasks"]
    return seen


def run_cases(lib, setenv, delenv, cases):
    """Every case, grouped by (family, switches, expected form, group, scoring): one plan per group, its form asserted from describe(),
    that plan run and fetched, every field (and the CIGAR) against expected().  Returns {form key: #pairs}."""
    groups = {}
    for c in cases:
        groups.setdefault((c["fam"], c["env"], c["want"], c["grp"], c["jb"], c["dual"], c["m"], c["sc"]), []).append(c)
    seen = {}
    for (fam, env, want, grp, *_), cs in groups.items():
        eu.set_env(setenv, delenv, ENVS[env])
        p = _plan(lib, cs)
        d = p.describe()
        try:
            got = _assert_form(fam, want, d, cs, (fam, ENVS[env], grp))
            p.run()
            res = p.fetch()
        finally:
            p.close()
        fields = FIELDS if fam == "extf" else FIELDS + ["cigar"]
        for c, r in zip(cs, res):
            exp = expected(c)
            bad = diff(exp, r, fields)
            assert not bad, (fam, ENVS[env], want, grp, len(c["q"]), len(c["t"]), c["w"], c["zdrop"], hex(c["flag"]),
                             {k: (exp[k], r[k]) for k in bad if k != "cigar"})
        for k, v in got.items():
            seen[k] = seen.get(k, 0) + v
    eu.set_env(setenv, delenv, {})
    return seen


def check_zstar(cases):
    """the Z* cases of a list come in pairs: no drop at Z*, a drop at Z* - 1 (by the oracle); returns #pairs"""
    zs = [c for c in cases if c["key"][1] == "drop"]
    for at, below in zip(zs[0::2], zs[1::2]):
        assert at["zdrop"] == below["zdrop"] + 1 and expected(at)["zdropped"] == 0 and expected(below)["zdropped"] == 1, at["key"]
    return len(zs) // 2


# ---------------------------------------------------------------- 4. the committed subset with the reference's answers

def golden_subset():
    """The cases the generator runs through the compiled reference: at least one per form and per side of each limit; for exts every
    mode at 448 / 449 and 960 / 961; two of the 21 504-long targets at w = 1000."""
    exts = [c for c in with_env(exts_cases(rots=range(6)), E_NONE) if c["gold"]]
    rest = [c for c in extf_tier_cases() + extf_window_cases() + extf_group_cases() + extf_lane_cases() + ssec_lds_cases() + ssec_blk_cases() if c["gold"]]
    return exts + rest


def golden_cases():
    """tests/golden/form_edge_cases.npz as a list of cases with the reference's record under "expect" """
    z = np.load(GOLDEN)
    out = []
    so, co = z["seq_off"], z["cigar_off"]
    for k in range(len(z["params"])):
        fam, dual, m, a, b, scn, gq, ge, gq2, ge2, w, zd, flag, jb, env, want, grp = (int(v) for v in z["params"][k])
        exp = dict(zip(FIELDS, (int(v) for v in z["expect"][k])))
        exp["cigar"] = [int(c) for c in z["cigar"][co[k]:co[k + 1]]]
        q, t, j = (z["seq"][so[3 * k + i]:so[3 * k + i + 1]] for i in range(3))
        out.append(dict(fam=FAMS[fam], q=q, t=t, junc=j if len(j) else None, jb=jb, flag=flag, zdrop=zd, w=w, dual=dual, m=m, sc=(a, b, scn, gq, ge, gq2, ge2),
                        env=env, want=WANTS[want], grp=grp, ncol=min(len(q), len(t)), expect=exp, key=("golden", k)))
    return out


def check_golden_oracle():
    """the oracle against the reference's answers at the form limits (every field and the CIGAR); returns #cases"""
    cs = golden_cases()
    for k, c in enumerate(cs):
        fields = FIELDS if c["fam"] == "extf" else FIELDS + ["cigar"]
        got = reference(c)
        assert not diff(c["expect"], got, fields), (k, c["fam"], c["want"], len(c["q"]), len(c["t"]), diff(c["expect"], got, fields))
    assert {c["fam"] for c in cs} == set(FAMS) and {c["want"] for c in cs} == set(WANTS), sorted(set(WANTS) - {c["want"] for c in cs})
    for ncol in (448, 449, 960, 961):                       # every exts mode at the limits and one past them
        modes = {c["flag"] & 0xff for c in cs if c["fam"] == "exts" and c["ncol"] == ncol}
        assert set(EXTS_MODES) <= modes, (ncol, modes)
    return len(cs)


def check_golden(lib, setenv, delenv):
    """the library on the committed cases, each under the switches it was recorded for; the exts cases again under
    KSW2AMD_EXTS_BIG=1 and (where they fit eight slots) KSW2AMD_EXTS_REG=1: the reference's answer does not depend on the form"""
    cs = golden_cases()
    exts = [c for c in cs if c["fam"] == "exts"]
    seen = run_cases(lib, setenv, delenv, cs + with_env(exts, E_BIG) + with_env([c for c in exts if c["ncol"] <= 448], E_REG))
    return len(cs), seen
