"""Shared by the simulator tier and the GPU tier: a deterministic path-shape grid for the traceback walks (k2a_trace_walk through
k2a_trace_kernel / k2a_trace_pk_kernel and their generation-serial forms, k2a_trace_solo) and for the CIGAR round (k2a_compact_kernel).

Pairs are built from a random 4-letter base with gaps of chosen kind, length and target row ("planted paths"): one gap at every
multiple of 64 rows (a strip boundary of every geometry, and every 2nd / 8th / 16th / 32nd of them a lane wrap), shifted by a swept
offset, so that every gap meets a strip boundary, a window refetch and the four-cell probe at every phase.  Expected records and CIGARs
come from the oracle only, every field of parity_util.CMP_FIELDS, every generated pair.  Which kernel ran is read from the plan's
description, never assumed.

walk_events() decodes the ORACLE's CIGAR into the cell path and replays the walk's control flow over it (windows of K2A_WALK_NW
lane-steps, strip crossings, the four-cell probe's guards) for a given (G, C, generation-serial or not), only to count which of the
edge events of required_events() the case went through.  It never produces an expected value: if it is wrong it misreports coverage, it cannot
make a wrong CIGAR pass.  Every check returns {event: count}; the tiers assert count >= NEED for every event required of the form."""
import os

import numpy as np

from ksw2_amd import synth
from oracle import pyoracle as po
from tests.edge_util import set_env
from tests.parity_util import diff

NW = 16                         # K2A_WALK_NW
AHEAD = 8                       # the solo walk's look-ahead
SOLO_C = 8                      # K2A_SOLO_C: rows per half of a double strip with traceback on (asserted from describe())
NEED = 4
MAT = synth.simple_mat(5, 2, 4, 0)
GAPS = (4, 2, 24, 1)            # q + l e = q2 + l e2 at l = 20: the two-piece crossover


def _rand(rng, n):
    return rng.integers(0, 4, int(n), dtype=np.uint8)


# ---------------------------------------------------------------- planted paths

def planted_pair(rng, tlen, gaps, lead=None):
    """A pair whose target has `tlen` rows: a shared random base, and for every (row, kind, length) of `gaps` (rows ascending) either
    `length` extra target bases from target row `row` on (kind 'D', a deletion) or `length` extra query bases in front of that row
    (kind 'I', an insertion).  lead = (kind, length): the gap sits in front of row 0 / column 0."""
    nd = sum(ln for _, k, ln in gaps if k == "D") + (lead[1] if lead and lead[0] == "D" else 0)
    base = _rand(rng, tlen - nd)
    q, t, b, row = [], [], 0, 0
    if lead:
        (t if lead[0] == "D" else q).append(_rand(rng, lead[1]))
        row += lead[1] if lead[0] == "D" else 0
    for r, kind, ln in gaps:
        take = r - row
        assert take > 0 and b + take <= len(base), (r, row, b, len(base))
        q.append(base[b:b + take]); t.append(base[b:b + take])
        b += take; row += take
        # extra bases that differ from the base's next one on both sides: the gap cannot slide
        ins = _rand(rng, ln)
        if b < len(base):
            ins[0] = (base[b] + 1 + ins[0] % 3) % 4
            ins[-1] = (base[b - 1] + 1 + ins[-1] % 3) % 4 if ln > 1 else ins[0]
        if kind == "D":
            t.append(ins); row += ln
        else:
            q.append(ins)
    q.append(base[b:]); t.append(base[b:])
    q, t = np.concatenate(q), np.concatenate(t)
    assert len(t) == tlen
    return q, t


# gap programs: (kind, length) per site, rotated per group.  Lengths: 1, the window's 15 / 16 / 17 and 31 / 32 / 33, the two-piece
# crossover's 19 / 20 / 21 and 60 in both directions, whole strips of 8 / 16 / 32 rows (C + 2 = 10 / 18 / 34), 39.
PROGRAM = [("D", 1), ("I", 15), ("D", 10), ("I", 16), ("D", 19), ("I", 17), ("D", 18), ("I", 31), ("D", 21), ("I", 32), ("D", 34),
           ("I", 33), ("D", 20), ("I", 19), ("D", 60), ("I", 21), ("D", 3), ("I", 60), ("D", 39), ("I", 1), ("D", 7), ("I", 20)]


def grid_groups(tlen, nsites, offs, rots, step=64, first=64, wrap=0):
    """Gap lists: one group per rotation of PROGRAM over the sites first, first + step, ..; inside a group one list per offset --
    the same kinds and lengths (one shape), every gap shifted by the offset.  The site after a deletion of 25 rows or more stays
    empty (the run would reach it); the site at row `wrap` takes a deletion in every second group."""
    out = []
    for gi, rot in enumerate(rots):
        grp = []
        for off in offs:
            gaps, skip, pc = [], False, rot
            for s in range(nsites):
                if skip:
                    skip = False
                    continue
                kind, ln = PROGRAM[pc % len(PROGRAM)]
                pc += 1
                if first + s * step == wrap and gi % 2 == 0:
                    kind = "D"
                skip = kind == "D" and ln >= 25
                gaps.append((first + s * step + off, kind, ln))
            assert gaps[-1][0] + gaps[-1][2] + 8 <= tlen, (tlen, gaps[-1])
            grp.append(gaps)
        out.append(grp)
    return out


def dense_pair(n):
    """Match / 1-base-gap alternation: n blocks of (one shared base, one base only in the target | only in the query); the shared
    bases alternate 0 / 1, the target's extra bases are 2 and the query's 3, so that nothing else matches.  Under
    cheap gaps (D M I M = 0 against two mismatches and a match = -6) the optimal CIGAR has one op per base:
    n_cigar = 2 n >= (qlen + tlen) / 2."""
    q, t = [], []
    for k in range(n):
        q.append(k % 2); t.append(k % 2)
        if k % 2 == 0:
            t.append(2)
        else:
            q.append(3)
    return np.array(q, dtype=np.uint8), np.array(t, dtype=np.uint8)


DENSE_MAT = synth.simple_mat(5, 2, 4, 0)         # mismatch -4 = 2 (q + e), the harshest the entry points take; a gap of one base -(1 + 1)
DENSE_GAPS = (1, 1, 3, 1)


# ---------------------------------------------------------------- coverage accounting (never an expected value)

def cigar_path(cigar):
    """CIGAR words (start -> end) -> (ti, tj, ops in walk order: end -> start)."""
    ops, ti, tj = [], -1, -1
    for c in cigar:
        op, ln = c & 0xf, c >> 4
        ops += [op] * ln
        ti += ln if op in (0, 2) else 0
        tj += ln if op in (0, 1) else 0
    return ti, tj, ops[::-1]


def _bump(ev, k, n=1):
    ev[k] = ev.get(k, 0) + n


def cigar_events(cigar, G, C, dual, mp, ev, xo=20):
    """Events that are properties of the runs: deletion runs against strip boundaries / lane wraps, insertion run lengths."""
    i = j = 0
    R = G * C
    for x, c in enumerate(cigar):
        op, ln = c & 0xf, c >> 4
        if op == 2 and i > 0 and x + 1 < len(cigar):                 # rows i .. i + ln - 1 (not the leading / trailing run)
            a, b = i, i + ln - 1
            if a // C != b // C:
                if not dual or ln < xo:
                    _bump(ev, "del_cross_state1")
                if dual and ln > xo:
                    _bump(ev, "del_cross_state3")
                if a // R != b // R:
                    _bump(ev, "gen_del" if mp else "wrap_del")
            if a % C == 0:
                _bump(ev, "del_from_row0")
            if b % C == C - 1:
                _bump(ev, "del_to_rowC1")
            if ln >= C + 2:
                _bump(ev, "del_whole_strip")
        if op == 1 and ln in (15, 16, 17, 31, 32, 33) and j > 0:
            _bump(ev, "ins_len_%d" % ln)
        if dual and xo == 20 and op in (1, 2) and ln in (19, 20, 21, 60) and i > 0 and j > 0:
            _bump(ev, "piece_%s_%d" % ("E" if op == 2 else "F", ln))
        i += ln if op in (0, 2) else 0
        j += ln if op in (0, 1) else 0


def walk_events(cigar, G, C, dual, mp, w, ev, xo=20):
    """Replays k2a_trace_walk's control flow over the oracle's path."""
    cigar_events(cigar, G, C, dual, mp, ev, xo)
    ti, tj, ops = cigar_path(cigar)
    quad = C >= 16
    R = G * C
    i, j, pos = ti, tj, 0
    prev = prev2 = None
    mrun, first, ngen = 0, True, 0
    if ti % C == 0:
        _bump(ev, "start_row0")
    if ti % C == C - 1:
        _bump(ev, "start_rowC1")
    if ti == 0:
        _bump(ev, "start_i0")
    if tj == 0:
        _bump(ev, "start_j0")
    if mp and ti // R >= 2:
        _bump(ev, "gen_start_ge2")
    c = i % C
    while i >= 0 and j >= 0:
        S = i // C
        if mp:
            g = S // G
            step = j - max(0, g * R - w) + (S - g * G)
            blk = step if (S % G == 0 and g == 0) else 1 << 30
        else:
            blk = S + j if S % G == 0 else 1 << 30
        back = min(j, blk, NW - 1)
        nw, k = back + 1, 0
        if first and tj < NW - 1:
            _bump(ev, "win_clip_j")
            if S == 0:
                _bump(ev, "win_clip_block")
        first = False
        while k < nw and c >= 0 and j >= 0:
            op = ops[pos]
            state0 = prev in (None, 0)
            if quad and state0:
                guards = (k + 3 < nw, c >= 3, j >= 3)
                if all(guards):
                    nxt = ops[pos:pos + 4]
                    if c == 3:
                        _bump(ev, "quad_ck3")
                    if j == 3:
                        _bump(ev, "quad_j3")
                    if k == nw - 4:
                        _bump(ev, "quad_k_nw4")
                    if prev == 0 and prev2 in (1, 2):
                        _bump(ev, "quad_after_gap")
                    if nxt == [0, 0, 0, 0]:
                        i -= 4; j -= 4; c -= 4; k += 4; pos += 4
                        mrun += 4
                        prev = prev2 = 0
                        continue
                    at = next(x for x in range(4) if nxt[x] != 0)
                    if mrun >= 8:
                        _bump(ev, "quad_gap_at_%d" % at)
                elif guards == (True, False, True) and c == 2:
                    _bump(ev, "quad_ck2")
                elif guards == (True, True, False) and j == 2:
                    _bump(ev, "quad_j2")
                elif guards == (False, True, True) and k == nw - 3:
                    _bump(ev, "quad_k_nw3")
            pos += 1
            if op == 0:
                cross = c == 0 and i > 0 and j > 0
                i -= 1; j -= 1; c -= 1; k += 1
                mrun += 1
                if cross:
                    _bump(ev, "cross_diag")
                    if (i + 1) % R == 0:
                        _bump(ev, "gen_diag" if mp else "wrap_diag")
                        ngen += 1
            elif op == 2:
                cross = c == 0 and i > 0
                i -= 1; c -= 1
                mrun = 0
                if cross:
                    if k == 0:
                        _bump(ev, "locate_k0")
                    if (i + 1) % R == 0:
                        ngen += 1
            else:
                j -= 1; k += 1
                mrun = 0
                more = pos < len(ops) and ops[pos] == 1 and j >= 0
                if k == nw and more:
                    _bump(ev, "ins_open_refetch")
                if k == nw and not more and j >= 0 and nw == NW:
                    _bump(ev, "ins_ends_window")
            prev2, prev = prev, op
        if c < 0 and i >= 0:
            c = i % C
    if mp and ngen >= 2:
        _bump(ev, "gen_two_crossed")
    if i < 0 and j < 0:
        _bump(ev, "end_corner")
    if i >= 0:
        _bump(ev, "lead_del_merged" if prev == 2 else "lead_del_after_M")
    if j >= 0:
        _bump(ev, "lead_ins_merged" if prev == 1 else "lead_ins_after_M")
    return ev


def solo_events(cigar, C, ev):
    """Replays k2a_trace_solo's control flow (look-ahead of AHEAD cells on the diagonal inside one half of a double strip)."""
    ti, tj, ops = cigar_path(cigar)
    i, j, pos = ti, tj, 0
    while i >= 0 and j >= 0:
        r = i % (2 * C)
        c = r % C
        nq = min(AHEAD, c + 1, min(i, j) + 1)
        if c + 1 <= AHEAD and nq == c + 1:
            _bump(ev, "solo_clip_c%d" % c)
        for k in range(nq):
            op = ops[pos]; pos += 1
            if op == 0:
                if i % C == 0 and i > 0 and j > 0:
                    _bump(ev, "solo_cross_half" if i % (2 * C) == C else "solo_cross_strip")
                    if i % (128 * C) == 0:
                        _bump(ev, "solo_wrap")
                i -= 1; j -= 1
            else:
                _bump(ev, "solo_gap_at_%d" % k)
                if op == 2:
                    if i % C == 0 and i > 0:
                        _bump(ev, "solo_cross_del")
                    i -= 1
                else:
                    j -= 1
                break
    if i < 0 and j < 0:
        _bump(ev, "end_corner")
    if i >= 0:
        _bump(ev, "lead_del")
    if j >= 0:
        _bump(ev, "lead_ins")
    return ev


def start_events(exp, flag, ev):
    if exp["zdropped"]:
        _bump(ev, "start_zdrop")
    elif not flag & po.EXTZ_ONLY:
        _bump(ev, "start_corner")
    elif exp["reach_end"]:
        _bump(ev, "start_mqe")
    else:
        _bump(ev, "start_max")


BASE_EVENTS = ["cross_diag", "del_cross_state1", "del_from_row0", "del_to_rowC1", "del_whole_strip", "wrap_diag", "wrap_del",
               "ins_len_15", "ins_len_16", "ins_len_17", "ins_len_31", "ins_len_32", "ins_len_33", "ins_open_refetch", "ins_ends_window",
               "locate_k0", "end_corner", "lead_ins_after_M", "lead_del_after_M",
               "start_corner", "start_max", "start_mqe", "start_zdrop", "start_row0", "start_rowC1"]
DUAL_EVENTS = ["del_cross_state3"] + ["piece_%s_%d" % (p, n) for p in "EF" for n in (19, 20, 21, 60)]
QUAD_EVENTS = ["quad_gap_at_%d" % x for x in range(4)] + ["quad_ck3", "quad_ck2", "quad_j3", "quad_k_nw4", "quad_k_nw3", "quad_after_gap"]
MP_EVENTS = ["gen_diag", "gen_del", "gen_start_ge2", "gen_two_crossed"]
CLIP_EVENTS = ["start_i0", "start_j0", "win_clip_j", "win_clip_block"]
SOLO_EVENTS = ["solo_gap_at_%d" % x for x in range(AHEAD)] + ["solo_clip_c%d" % x for x in range(AHEAD)] + \
              ["solo_cross_half", "solo_cross_strip", "solo_cross_del", "solo_wrap", "end_corner", "lead_del", "lead_ins",
               "start_corner", "start_max", "start_mqe", "start_zdrop"]


def required_events(form):
    if form["kernel"] == "solo":
        return list(SOLO_EVENTS)
    ev = list(BASE_EVENTS)
    if form["mp"]:
        ev = [e for e in ev if not e.startswith("wrap_")] + MP_EVENTS
    if form["dual"]:
        ev += DUAL_EVENTS if not form["rebased"] else DUAL_EVENTS[:1]        # (the re-based forms' scoring has its crossover at 14)
    if form["C"] >= 16:
        ev += QUAD_EVENTS
    if form["clipw"] is not None:
        ev += CLIP_EVENTS
    return ev


# ---------------------------------------------------------------- forms

BIG_MAT = synth.simple_mat(5, 10, 12, 0)       # with (12, 4, 40, 2): scores leave 16 bits from about 900 rows on -- the re-based kernels
BIG_GAPS = (12, 4, 40, 2)                      # (crossover at 14 bases)


def _form(name, kernel, G, C, dual, env, w, tlen, minlen=64, mp=False, rebased=0, clipw=None, big=False, short=0):
    return dict(name=name, kernel=kernel, G=G, C=C, dual=dual, env=env, w=w, tlen=tlen, minlen=minlen, mp=mp, rebased=rebased, clipw=clipw, short=short,
                big=big, mat=BIG_MAT if rebased else MAT, gaps=BIG_GAPS if rebased else GAPS, xo=14 if rebased else 20)


def _forms():
    out = []
    for dual in (False, True):
        s = "-2p" if dual else ""
        i32 = {"KSW2AMD_NO_PK": 1}
        # int32: the first geometry that holds the band wins -- (16,8) w <= 68; (64,8) more than 128 rows and w <= 284;
        # (64,16) more than 512 rows and w <= 536; (64,32) more than 1 024 rows and w <= 1 040; then generation-serial
        out.append(_form("int32-16x8" + s, "int32", 16, 8, dual, i32, 68, 360, clipw=68))
        out.append(_form("int32-64x8" + s, "int32", 64, 8, dual, i32, 100, 616, minlen=136, clipw=284))
        out.append(_form("int32-64x16" + s, "int32", 64, 16, dual, i32, 300, 1128, minlen=520, clipw=536, short=240))
        out.append(_form("int32-64x32" + s, "int32", 64, 32, dual, i32, 600, 2152, minlen=1032, clipw=1040, big=True, short=450))
        out.append(_form("mp-64x16" + s, "mp", 64, 16, dual, {"KSW2AMD_NO_PKMP": 1, "KSW2AMD_NO_PK": 1}, -1, 2152, minlen=2152, mp=True, clipw=-1, big=True, short=200))
        # packed: KSW2AMD_PK_FIRST names the first geometry tried; (8,18) is score only (no traceback is ever planned for it)
        out.append(_form("pk-16x8" + s, "pk", 16, 8, dual, {"KSW2AMD_PK_FIRST": 1}, 68, 360, clipw=68))
        out.append(_form("pk-64x8" + s, "pk", 64, 8, dual, {"KSW2AMD_PK_FIRST": 2}, 100, 616, clipw=100))
        out.append(_form("pk-64x16" + s, "pk", 64, 16, dual, {"KSW2AMD_PK_FIRST": 3}, 100, 1128, clipw=100))
        out.append(_form("pk-64x8-rb" + s, "pk", 64, 8, dual, {"KSW2AMD_PK_FIRST": 2}, 100, 1128, minlen=1032, rebased=1, big=True))
        out.append(_form("pk-64x16-rb" + s, "pk", 64, 16, dual, {"KSW2AMD_PK_FIRST": 3}, 100, 1128, minlen=1032, rebased=1, big=True))
        out.append(_form("pkmp-64x16" + s, "pkmp", 64, 16, dual, {}, -1, 2152, minlen=2152, mp=True, clipw=-1, big=True, short=200))
        out.append(_form("solo" + s, "solo", 64, SOLO_C, dual, {"KSW2AMD_SOLO": "all"}, 64, 1080, clipw=64))
    for k, f in enumerate(out):
        f["seed"] = 7 + k
    # the plan's own form for long pairs in a narrow band with a CIGAR: (16,8) re-based
    for k, dual in ((8, False), (21, True)):
        f = _form("pk-16x8-rb" + ("-2p" if dual else ""), "pk", 16, 8, dual, {"KSW2AMD_PK_FIRST": 1}, 68, 1128, minlen=1032, rebased=1, big=True)
        f["seed"] = 100 + int(dual)
        out.insert(k, f)
    return out


FORMS = _forms()
FORM_IDS = [f["name"] for f in FORMS]


def form_ok(form, d, qs, ts, flag):
    """The plan's description against the form: every class is the form's kernel, geometry and gap model -- except as many tasks as
    there are (shape, alignment side) keys with an odd number of pairs, which a packed plan may hand to another kernel."""
    fl = np.broadcast_to(np.asarray(flag), (len(qs),))
    keys = {}
    for i in range(len(qs)):
        k = (len(qs[i]), len(ts[i]), int(fl[i]))
        keys[k] = keys.get(k, 0) + 1
    nodd = sum(v & 1 for v in keys.values()) if form["kernel"] in ("pk", "pkmp") else 0
    main = [c for c in d if c["kernel"] == form["kernel"]]
    rest = [c for c in d if c["kernel"] != form["kernel"]]
    ok = bool(main) and all(c["gaps"] == (2 if form["dual"] else 1) and c["mode"] != "score" for c in main)
    # (a solo class reports the rows of its double strip)
    ok = ok and all(c["G"] == form["G"] and c["C"] == form["C"] * (2 if form["kernel"] == "solo" else 1) for c in main)
    if form["kernel"] == "pk":
        ok = ok and all(c["rebased"] == form["rebased"] for c in main)
    return ok and sum(c["tasks"] for c in rest) <= nodd


# ---------------------------------------------------------------- the checks

def run_batch(lib, form, qs, ts, w, flag, zdrop=-1, end_bonus=0, flat=False, mat=None, gaps=None, exp=None):
    """One plan over the pointer (or flat) batch against the oracle, the form asserted from its describe(); returns the oracle's
    records."""
    mat = form["mat"] if mat is None else mat
    gaps = form["gaps"] if gaps is None else gaps
    q, e, q2, e2 = gaps if form["dual"] else (gaps[0], gaps[1], 0, 0)
    func = "extd2" if form["dual"] else "extz2"
    n = len(qs)
    bc = lambda v: np.array(np.broadcast_to(np.asarray(v), (n,)))           # noqa: E731
    zd, eb, fl = bc(zdrop), bc(end_bonus), bc(flag)
    mk = lib.make_flat_batch if flat else lib.make_batch
    b = mk(qs, ts, mat, q, e, q2, e2, w=w, zdrop=zd, end_bonus=eb, flag=fl)
    p = b.plan(form["dual"])                                   # the plan that is described is the plan that runs
    d = p.describe()
    assert form_ok(form, d, qs, ts, fl), (form["name"], d)
    p.run()
    res = p.fetch()
    p.close()
    if exp is None:
        exp = [po.align("oracle", func, qs[i], ts[i], mat, q, e, q2, e2, w=w, zdrop=int(zd[i]), end_bonus=int(eb[i]), flag=int(fl[i])) for i in range(n)]
    bad = [(i, diff(exp[i], res[i])) for i in range(n) if diff(exp[i], res[i])]
    assert not bad, (form["name"], "flat" if flat else "batch", len(bad), bad[:4], [(exp[i]["cigar"], res[i]["cigar"]) for i, _ in bad[:1]])
    return exp


def account(form, exp, qs, ts, w, flag, ev):
    fl = np.broadcast_to(np.asarray(flag), (len(exp),))
    for i, x in enumerate(exp):
        cig = x["cigar"][::-1] if int(fl[i]) & po.REV_CIGAR else x["cigar"]
        if not cig:
            continue
        ww = max(len(qs[i]), len(ts[i])) if w < 0 else w
        if form["kernel"] == "solo":
            solo_events(cig, form["C"], ev)
        else:
            walk_events(cig, form["G"], form["C"], form["dual"], form["mp"], ww, ev, form["xo"])
        start_events(x, int(fl[i]), ev)


def _fit_band(gaps, w):
    """keep the path inside the band: flip the kinds that would carry it past +- (w - 4)"""
    drift, out = 0, []
    for r, kind, ln in gaps:
        s = ln if kind == "D" else -ln
        if w >= 0 and abs(drift + s) > w - 4:
            kind, s = ("I" if kind == "D" else "D"), -s
        drift += s
        out.append((r, kind, ln))
    return out


def grid_cases(form, thin=1):
    """The pairs of one form: [(tag, qs, ts, flag, zdrop, end_bonus)].  thin > 1 (the simulator tier) keeps a part of every sweep:
    the offsets -2 .. 3 of -5 .. 6, every third rotation of the gap program, four of the twelve leading-gap lengths, every fourth head
    length.  The forms marked `big` (every pair of more than 1 000 or 2 000 rows) sweep the offsets -2 .. 3 and every fourth rotation,
    six leading-gap lengths and every second head length, thinned to -1 .. 2, every sixth rotation, two lengths and every eighth head."""
    rng = np.random.Generator(np.random.PCG64(form["seed"]))
    C, T, w, Lm, big = form["C"], form["tlen"], form["w"], form["minlen"], form["big"]
    nsites = (T - 64 - 60 - 16) // 64 + 1
    if T <= 400:
        thin = 1                                               # (a few strips: cheap everywhere)
    offs = [-1, 0, 1, 2] if big and thin > 1 else [-2, -1, 0, 1, 2, 3] if big or thin > 1 else list(range(-5, 7))
    rots = list(range(0, len(PROGRAM), (4 if big else 1) if thin == 1 else (6 if big else 3)))
    # forms that need many rows (not many columns): the short sweeps run on a query of `short` bases, the target stretched by
    # unrelated rows to the form's minimum (a deletion run from the corner, or rows past the start cell)
    short = form["short"]
    Ls = short if short else Lm

    def stretch(t):
        return np.concatenate([t, _rand(rng, Lm + 8 - len(t))]) if short else t

    out = []
    for right in (0, po.RIGHT):
        qs, ts = [], []
        for gi, grp in enumerate(grid_groups(T - 8, nsites, offs, rots, wrap=form["G"] * C)):
            for gaps in grp:
                # start rows C - 2, C - 1 and 0 of a strip (T is a multiple of 32 plus 8)
                q, t = planted_pair(rng, T - 8 + (gi % 3) - 1, _fit_band(gaps, w))
                qs.append(q); ts.append(t)
        if form["kernel"] in ("pk", "pkmp"):                   # an odd alignment in its class
            q, t = planted_pair(rng, T - 8, _fit_band(grid_groups(T - 8, nsites, [0], [1])[0][0], w))
            qs.append(q); ts.append(t)
        out.append(("grid", qs, ts, right, -1, 0))
    # the two alignments of a task on different paths: a long insertion and a long deletion against a pure diagonal, both orders
    qs, ts = [], []
    for k in range(6 if thin == 1 else 2):
        q, t = planted_pair(rng, Ls + 100, [(30 + k, "D", 30), (Ls + 50 + k, "I", 30)])
        d = _rand(rng, Ls + 100)
        t, d2 = stretch(t), stretch(d)
        d1 = d2[:len(q)] if short else d
        qs += [q, d1, d1.copy(), q.copy()][::1 if k % 2 else -1]; ts += [t, d2, d2.copy(), t.copy()][::1 if k % 2 else -1]
    out.append(("halves", qs, ts, 0, -1, 0))
    # leading gaps of 1 .. 12 bases in front of row 0 / column 0 (the four-cell probe at j = 3, the leading run after an M run),
    # alone and with a gap a few cells after them (shapes come in pairs)
    lens = (range(1, 13, 2) if big else range(1, 13)) if thin == 1 else (1, 2, 3, 6) if not big else (2, 5)
    for right in (0, po.RIGHT):
        qs, ts = [], []
        for ln in lens:
            for kind in "DI":
                for near in ([], [], [(ln + 5, "D", 2), (ln + 24, "I", 2)], [(ln + 9, "I", 2), (ln + 30, "D", 2)]):
                    q, t = planted_pair(rng, Ls + ln + (2 if near else 0), near, lead=(kind, ln))
                    qs.append(q); ts.append(stretch(t))
        out.append(("lead", qs, ts, right, -1, 0))
    # start cells: the corner, the maximum under EXTZ_ONLY, the mqe cell with an end bonus, the maximum of a Z-dropped pair -- a
    # matching head of a swept length, then tails that do not match (each pair twice: a partner of its shape)
    qs, ts, fl, zd, eb = [], [], [], [], []
    L = Ls + 40
    hstep = (2 if big else 1) if thin == 1 else 8 if big else 4
    for head in range(L - 40, L - 8, hstep):
        for mode in range(4):
            for rep in range(2):
                base = _rand(rng, head)
                if mode == 2:                                # the query ends inside the target: mqe + bonus beats the maximum
                    q = np.concatenate([base, (base[-1:] + 1) % 4])
                    t = np.concatenate([base, (base[-1:] + 2) % 4, np.full(L - head - 1, (int(base[-1]) + 3) % 4, np.uint8)])
                else:
                    q = np.concatenate([base, np.full(L - head, 0, np.uint8)])
                    t = np.concatenate([base, np.full(L - head, 1, np.uint8)])
                qs.append(q); ts.append(stretch(t))
                fl.append((0, po.EXTZ_ONLY, po.EXTZ_ONLY, 0)[mode] | (po.RIGHT if ((head - L) // hstep) % 2 else 0))
                zd.append(2 if mode == 3 else -1)         # (2 < q: drops with the row maximum at either end of its ties, so under RIGHT too)
                eb.append(20 if mode == 2 else 0)
    out.append(("start", qs, ts, np.array(fl), np.array(zd), np.array(eb)))
    if form["clipw"] is not None:
        # a start cell in columns 0 .. 14 (a first window clipped by j): the query is the target's first 1 .. 15 bases -- under
        # EXTZ_ONLY the walk starts at (k - 1, k - 1), strip 0 of lane 0, where the block's start clips the window too, and with k = 1
        # at i = j = 0; without it at (tlen - 1, k - 1), a deletion run down from the last strip
        qs, ts, fl = [], [], []
        for k in (range(1, 16) if thin == 1 else (1, 2, 5, 15)):
            for rep in range(4 if k == 1 else 2):
                b = _rand(rng, Lm + 8)
                qs += [b[:k], b[:k].copy()]; ts += [b, b.copy()]; fl += [po.EXTZ_ONLY | (rep % 2) * po.RIGHT, (rep % 2) * po.RIGHT]
        out.append(("clip", qs, ts, np.array(fl), -1, 0))
    return out


def check_form(lib, setenv, delenv, form, thin=1, flat=True):
    """Every pair of grid_cases(form) through the pointer batch entry, the lead and start sweeps through the flat entry as well;
    returns the events the oracle's paths went through."""
    set_env(setenv, delenv, form["env"])
    ev = {}
    for tag, qs, ts, flag, zd, eb in grid_cases(form, thin):
        w = form["clipw"] if tag == "clip" else form["w"]
        exp = run_batch(lib, form, qs, ts, w, flag, zd, eb)
        account(form, exp, qs, ts, w, flag, ev)
        if flat and tag in ("lead", "start"):
            run_batch(lib, form, qs, ts, w, flag, zd, eb, flat=True, exp=exp)
    set_env(setenv, delenv, {})
    return ev


def oracle_events(form, thin=1):
    """The same accounting on the oracle alone."""
    ev = {}
    q, e, q2, e2 = form["gaps"] if form["dual"] else (form["gaps"][0], form["gaps"][1], 0, 0)
    for tag, qs, ts, flag, zd, eb in grid_cases(form, thin):
        n, w = len(qs), form["clipw"] if tag == "clip" else form["w"]
        fl, zd, eb = (np.broadcast_to(np.asarray(v), (n,)) for v in (flag, zd, eb))
        exp = [po.align("oracle", "extd2" if form["dual"] else "extz2", qs[i], ts[i], form["mat"], q, e, q2, e2, w=w, zdrop=int(zd[i]),
                        end_bonus=int(eb[i]), flag=int(fl[i])) for i in range(n)]
        account(form, exp, qs, ts, w, flag, ev)
    return ev


def assert_coverage(form, ev):
    missing = {e: ev.get(e, 0) for e in required_events(form) if ev.get(e, 0) < NEED}
    assert not missing, (form["name"], missing)


# ---------------------------------------------------------------- the CIGAR round (k2a_compact_kernel) and walks per wavefront

def dense_case(nops):
    """A pair whose optimal CIGAR under DENSE_MAT / DENSE_GAPS has `nops` operations: nops // 2 blocks of dense_pair(), and a
    shared run of three bases at the end when nops is odd."""
    q, t = dense_pair(nops // 2)
    if nops & 1:
        tail = np.array([(nops // 2) % 2, 1 - (nops // 2) % 2, (nops // 2) % 2], dtype=np.uint8)
        q, t = np.concatenate([q, tail]), np.concatenate([t, tail])
    return q.astype(np.uint8), t.astype(np.uint8)


COMPACT_NOPS = (1, 2, 63, 64, 65, 128, 129)


def check_compaction(lib, setenv, delenv, env, dual, kernels):
    """n_cigar in COMPACT_NOPS with and without KSW_EZ_REV_CIGAR, and the dense-indel pair (n_cigar >= (qlen + tlen) / 2: the
    per-pair CIGAR scratch of qlen + tlen + 2 words), in ONE plan ordered so that a pair's neighbours have CIGARs of other lengths,
    longer on one side and (where there is a shorter one) shorter on the other: a wrong pos[i] overlaps them.  The lengths are
    asserted on the oracle's records, the kernels (`kernels`: the set the env allows) on the plan that runs.  Returns
    {(n_cigar, reversed): count}."""
    set_env(setenv, delenv, env)
    want = [300, 1, 129, 2, 128, 63, 65, 64, 300, 64, 2, 129, 1, 65, 63, 128]
    qs, ts, fl = [], [], []
    for rep in range(2):
        for k, nops in enumerate(want):
            q, t = dense_case(nops)
            qs.append(q); ts.append(t); fl.append(po.REV_CIGAR if (k + rep) % 2 else 0)
    want = want * 2
    q, e, q2, e2 = DENSE_GAPS if dual else (DENSE_GAPS[0], DENSE_GAPS[1], 0, 0)
    func = "extd2" if dual else "extz2"
    exp = [po.align("oracle", func, qs[i], ts[i], DENSE_MAT, q, e, q2, e2, w=40, flag=fl[i]) for i in range(len(qs))]
    got = [x["n_cigar"] for x in exp]
    assert got == want, (got, want)
    assert all(2 * x["n_cigar"] >= len(qs[i]) + len(ts[i]) for i, x in enumerate(exp) if want[i] == 300)
    for flat in (False, True):
        mk = lib.make_flat_batch if flat else lib.make_batch
        b = mk(qs, ts, DENSE_MAT, q, e, q2, e2, w=40, zdrop=-1, end_bonus=0, flag=np.array(fl))
        p = b.plan(dual)
        d = p.describe()
        assert d and all(c["kernel"] in kernels and c["mode"] != "score" and c["gaps"] == (2 if dual else 1) for c in d), (env, d)
        assert sum(c["tasks"] * (2 if c["kernel"] in ("pk", "pkmp") else 1) for c in d) >= len(qs), (env, d)
        p.run()
        res = p.fetch()
        p.close()
        bad = [(i, diff(exp[i], res[i])) for i in range(len(qs)) if diff(exp[i], res[i])]
        assert not bad, (env, dual, flat, bad[:4])
    set_env(setenv, delenv, {})
    seen = {}
    for i, n in enumerate(want):
        seen[(n, fl[i] != 0)] = seen.get((n, fl[i] != 0), 0) + 1
    return seen


def trace_ppw(nwalks):
    """k2a_trace_ppw (ksw2_shim_hip.hip): walks per wavefront of one trace launch"""
    return min(8, max(1, -(-nwalks // 4096)))


def check_ppw(lib, setenv, delenv, env, dual, nwalks, kernel):
    """`nwalks` walks of 24 x 24 .. 40 x 40 in ONE class of one plan (asserted: the class's task count is what k2a_trace_ppw
    sees) -- tiled from 64 distinct planted pairs (32 shapes, two pairs each) in a shuffled order, so that the threads of a
    wavefront walk different paths; the oracle runs on the 64 only.  Returns the walks per wavefront that the class's walk count gives."""
    set_env(setenv, delenv, env)
    rng = np.random.Generator(np.random.PCG64(43))
    base_q, base_t = [], []
    for k in range(32):
        L = 24 + k % 13
        for rep in range(2):
            kind = "DI"[(k + rep) % 2]
            other = "ID"[(k + rep) % 2]
            q, t = planted_pair(rng, L + 4, [(6 + (k + 5 * rep) % 9, kind, 4), (18 + (k + 3 * rep) % 5, other, 4)])
            base_q.append(q); base_t.append(t)
    assert all(24 <= len(x) <= 40 for x in base_q + base_t)
    q, e, q2, e2 = GAPS if dual else (GAPS[0], GAPS[1], 0, 0)
    exp = [po.align("oracle", "extd2" if dual else "extz2", base_q[i], base_t[i], MAT, q, e, q2, e2, w=20, flag=0) for i in range(64)]
    assert len({tuple(x["cigar"]) for x in exp}) >= 32
    # tasks of the packed kernels hold two pairs of one shape: shuffle the 32 shapes, keep a shape's two pairs together
    order = np.concatenate([2 * rng.permutation(32)[:, None] + np.arange(2)[None, :] for _ in range(-(-nwalks // 64))]).reshape(-1)[:nwalks]
    qs, ts = [base_q[i] for i in order], [base_t[i] for i in order]
    b = lib.make_batch(qs, ts, MAT, q, e, q2, e2, w=20, zdrop=-1, end_bonus=0, flag=0)
    p = b.plan(dual)
    d = p.describe()
    # one class holds every walk: the int32 trace launch counts tasks, the packed one two walks per task
    assert len(d) == 1 and d[0]["kernel"] == kernel and d[0]["mode"] != "score" and d[0]["gaps"] == (2 if dual else 1), d
    assert d[0]["tasks"] * (2 if kernel == "pk" else 1) == nwalks, (d, nwalks)
    p.run()
    res = p.fetch()
    p.close()
    bad = [(i, diff(exp[order[i]], res[i])) for i in range(nwalks) if diff(exp[order[i]], res[i])]
    assert not bad, (env, nwalks, len(bad), bad[:4])
    set_env(setenv, delenv, {})
    return trace_ppw(nwalks)


# ---------------------------------------------------------------- the reference's own answers on planted cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trace_cases.npz")
GOLDEN_FIELDS = ["score", "max", "max_t", "max_q", "mqe", "mqe_t", "mte", "mte_q", "zdropped", "reach_end", "n_cigar"]
GOLDEN_FORMS = ["int32-16x8", "int32-64x16", "mp-64x16", "solo"]       # and their two-piece rows


def golden_events(form):
    """The events of the form's table that the compiled reference's scalar ksw_extz / ksw_extd can express on the grid's pairs.  It
    cannot: `start_mqe` (the scalar entry points have no end bonus); and for the (16,8) row `start_i0` / `start_j0`, which need the
    query of ONE base against 72 rows with w = 68 -- rows outside the band (tlen > qlen + w), on which the reference's scalar code
    writes past its row buffer, so pairs with such rows are left out."""
    ev = [e for e in required_events(form) if e != "start_mqe"]
    if (form["G"], form["C"], form["kernel"]) == (16, 8, "int32"):
        ev = [e for e in ev if e not in ("start_i0", "start_j0")]
    return ev


def _golden_form(name, dual):
    return FORMS[FORM_IDS.index(name + ("-2p" if dual else ""))]


def golden_coverage(cases, exp):
    """{(form name, KSW_EZ_RIGHT or 0): {event: count}} over records `exp` of cases (form index, dual, q, t, w, zdrop, flag), and the
    assertion that every event of golden_events() is there at least once per form row (so per gap model) and per value of RIGHT."""
    cov = {}
    for c, x in zip(cases, exp):
        form = _golden_form(GOLDEN_FORMS[c[0]], c[1])
        account(form, [x], [c[2]], [c[3]], c[4], c[6], cov.setdefault((form["name"], c[6] & po.RIGHT), {}))
    for fi, name in enumerate(GOLDEN_FORMS):
        for dual in (False, True):
            form = _golden_form(name, dual)
            for right in (0, po.RIGHT):
                ev = cov.get((form["name"], right), {})
                missing = [e for e in golden_events(form) if ev.get(e, 0) < 1]
                assert not missing, (form["name"], right, missing)
    return cov


def golden_inputs():
    """The subset of the grid for tests/gen_trace_golden.py: [(form index in GOLDEN_FORMS, dual, q, t, w, zdrop, flag)].  For every
    row of GOLDEN_FORMS, both gap models and both values of KSW_EZ_RIGHT, pairs of the row's thinned sweeps are taken greedily (the
    pair that adds the most events of golden_events() not yet seen, by the oracle's path) until every such event is there, then every
    sixth of the remaining pairs of the rows under 2 000 rows.  Pairs with an end bonus or with rows outside the band are left out."""
    out = []
    for fi, name in enumerate(GOLDEN_FORMS):
        for dual in (False, True):
            form = _golden_form(name, dual)
            q, e, q2, e2 = GAPS if dual else (GAPS[0], GAPS[1], 0, 0)
            cand = []
            for tag, qs, ts, flag, zd, eb in grid_cases(form, thin=3):
                n, w = len(qs), form["clipw"] if tag == "clip" else form["w"]
                fl, zd, eb = (np.broadcast_to(np.asarray(v), (n,)) for v in (flag, zd, eb))
                for i in range(n):
                    if int(eb[i]) == 0 and (w < 0 or len(ts[i]) <= len(qs[i]) + w):
                        cand.append((fi, dual, qs[i], ts[i], w, int(zd[i]), int(fl[i])))
            evs = []
            for c in cand:
                x = po.align("oracle", "extd" if dual else "extz", c[2], c[3], MAT, q, e, q2, e2, w=c[4], zdrop=c[5], flag=c[6])
                ev = {}
                account(form, [x], [c[2]], [c[3]], c[4], c[6], ev)
                evs.append(set(ev) & set(golden_events(form)))
            taken = set()
            for right in (0, po.RIGHT):
                need = set(golden_events(form))
                idx = [i for i, c in enumerate(cand) if (c[6] & po.RIGHT) == right]
                while need:
                    best = max(idx, key=lambda i: (len(evs[i] & need), -i))
                    assert evs[best] & need, (form["name"], right, sorted(need))
                    taken.add(best)
                    need -= evs[best]
            rest = [i for i in range(len(cand)) if i not in taken]
            if form["tlen"] < 2000:
                taken |= set(rest[::6])
            out += [cand[i] for i in sorted(taken)]
    return out


def save_golden(path, cases, exp):
    """Data only; written member by member with a fixed time stamp, so that the same cases give the same bytes."""
    import io
    import zipfile
    arrs = dict(par=np.array([[c[0], int(c[1]), len(c[2]), len(c[3]), c[4], c[5], c[6]] for c in cases], np.int32),
                seq=np.concatenate([np.asarray(x, np.uint8) for c in cases for x in (c[2], c[3])]),
                exp=np.array([[e[f] for f in GOLDEN_FIELDS] for e in exp], np.int32),
                cigar=np.array([c for e in exp for c in e["cigar"]], np.uint32))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrs[k], version=(1, 0))
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def load_golden(path=GOLDEN):
    """-> ([(form index, dual, q, t, w, zdrop, flag)], [expected record with its CIGAR])"""
    z = np.load(path)
    cases, exp, so, co = [], [], 0, 0
    for k, (fi, dual, ql, tl, w, zd, fl) in enumerate(z["par"].tolist()):
        q, t = z["seq"][so:so + ql], z["seq"][so + ql:so + ql + tl]
        so += ql + tl
        e = dict(zip(GOLDEN_FIELDS, (int(v) for v in z["exp"][k])))
        e["cigar"] = [int(c) for c in z["cigar"][co:co + e["n_cigar"]]]
        co += e["n_cigar"]
        cases.append((fi, bool(dual), q, t, w, zd, fl))
        exp.append(e)
    return cases, exp


def check_golden_oracle():
    """The oracle (the scalar contract and the ..2 entry points without an end bonus) against the reference's answers, and the
    file's own coverage: every event the reference can express, per form row and value of RIGHT."""
    cases, exp = load_golden()
    golden_coverage(cases, exp)
    for k, ((fi, dual, q, t, w, zd, fl), e) in enumerate(zip(cases, exp)):
        for func in (("extd", "extd2") if dual else ("extz", "extz2")):
            got = po.align("oracle", func, q, t, MAT, *GAPS, w=w, zdrop=zd, flag=fl) if dual else po.align("oracle", func, q, t, MAT, GAPS[0], GAPS[1], w=w, zdrop=zd, flag=fl)
            assert not diff(e, got), (k, func, diff(e, got))
    return len(cases)


def check_golden(lib, setenv, delenv):
    """A library on the same cases, one plan per form row: under the row's own env (the form asserted from describe(), as in
    run_batch) and, each pair twice so that it has a partner of its shape, under the plan's own choice -- asserted to be the packed
    family for every pair."""
    cases, exp = load_golden()
    n = 0
    for fi, name in enumerate(GOLDEN_FORMS):
        for dual in (False, True):
            form = _golden_form(name, dual)
            sub = [k for k, c in enumerate(cases) if c[0] == fi and c[1] == dual]
            assert sub, form["name"]
            q, e, q2, e2 = GAPS if dual else (GAPS[0], GAPS[1], 0, 0)
            for env, rep in ((form["env"], 1), ({}, 2)):
                set_env(setenv, delenv, env)
                idx = [k for k in sub for _ in range(rep)]
                qs, ts = [cases[k][2] for k in idx], [cases[k][3] for k in idx]
                w, zd, fl = (np.array([cases[k][x] for k in idx]) for x in (4, 5, 6))
                p = lib.make_batch(qs, ts, MAT, q, e, q2, e2, w=w, zdrop=zd, end_bonus=0, flag=fl).plan(dual)
                d = p.describe()
                if rep == 1:
                    assert form_ok(form, d, qs, ts, fl), (form["name"], d)
                else:
                    assert d and all(c["kernel"] in ("pk", "pkmp", "solo") and c["mode"] != "score" for c in d), (form["name"], d)
                p.run()
                res = p.fetch()
                p.close()
                bad = [(k, diff(exp[k], r)) for k, r in zip(idx, res) if diff(exp[k], r)]
                assert not bad, (form["name"], env, bad[:4])
                n += len(sub)
    set_env(setenv, delenv, {})
    return n
