"""Helpers of the tests of the two-piece suboptimal score and the two-piece single-pair entries (ksw2amd_lld_sub_batch / _flat,
ksw2amd_lld, ksw2amd_lld_align, ksw2amd_lld_sub): the scalar oracle tests/llds_oracle.c compiled with gcc into a
temporary directory, a brute-force Python statement of the definition, the simulator build with the launch's twin
(tests/llsim/llds_shim_sim.cpp), and the inputs and checks that the CPU tier (simulator) and the GPU tier share.
costs = (gapo, gape, gapo2, gape2) throughout."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u
from tests import lld_util as d
from tests import llf_util as lf
from tests import lls_util as s

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "llds_cases.npz")
CROSS = d.CROSS                  # (4, 2, 24, 1): the pieces cross at l = 20
CHEAP2 = (6, 3, 2, 1)            # the second piece is cheaper everywhere
COSTS = (CROSS, CHEAP2)
M5 = s.M5
NONE = [0, -1, -1]
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "libllds_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "llds_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.llds_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_batch(queries, targets, mat, costs, excl=-1, m=None):
    """(n, 6) int32 array of score, qe, te, score2, qe2, te2 from the scalar two-piece oracle."""
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    m = int(round(len(mat) ** 0.5)) if m is None else m
    n = len(queries)
    seqs = [np.ascontiguousarray(x, dtype=np.uint8) for x in list(queries) + list(targets)]
    lens = np.array([len(x) for x in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    base = np.concatenate(seqs + [np.zeros(1, np.uint8)]).astype(np.uint8)
    qoff, toff = np.ascontiguousarray(offs[:n]), np.ascontiguousarray(offs[n:2 * n])
    qlen, tlen = lens[:n].astype(np.int32), lens[n:].astype(np.int32)
    out = np.zeros((max(n, 1), 6), dtype=np.int32)
    oracle().llds_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                               m, mat.ctypes.data, *[int(c) for c in costs], int(excl), out.ctypes.data)
    return out[:n]


def brute(query, target, mat, costs, m, excl):
    """The definition in plain Python on the full matrix with unclamped E, F, E2, F2: (score, qe, te, score2, qe2, te2)."""
    go, ge, go2, ge2 = costs
    q, t = list(map(int, query)), list(map(int, target))
    NEG = -(1 << 40)
    nq, nt = len(q), len(t)
    smax = max(int(x) for x in mat)
    if smax <= 0 or not q or not t:
        return 0, -1, -1, 0, -1, -1
    H = [[0] * (nq + 1) for _ in range(nt + 1)]
    E = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    F = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    E2 = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    F2 = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    for i in range(1, nt + 1):
        for j in range(1, nq + 1):
            E[i][j] = max(E[i - 1][j] - ge, H[i - 1][j] - go - ge)
            F[i][j] = max(F[i][j - 1] - ge, H[i][j - 1] - go - ge)
            E2[i][j] = max(E2[i - 1][j] - ge2, H[i - 1][j] - go2 - ge2)
            F2[i][j] = max(F2[i][j - 1] - ge2, H[i][j - 1] - go2 - ge2)
            H[i][j] = max(0, H[i - 1][j - 1] + int(mat[t[i - 1] * m + q[j - 1]]), E[i][j], F[i][j], E2[i][j], F2[i][j])
    R = [max(H[i + 1][1:]) for i in range(nt)]
    score = max(R)
    if score <= 0:
        return 0, -1, -1, 0, -1, -1
    te = min(i for i in range(nt) if R[i] == score)
    qe = min(j for j in range(nq) if H[te + 1][j + 1] == score)
    dd = excl if excl >= 0 else -(-score // smax)
    rows = [i for i in range(nt) if abs(i - te) > dd]
    s2 = max([R[i] for i in rows], default=0)
    if s2 <= 0:
        return score, qe, te, 0, -1, -1
    te2 = min(i for i in rows if R[i] == s2)
    qe2 = min(j for j in range(nq) if H[te2 + 1][j + 1] == s2)
    return score, qe, te, s2, qe2, te2


def sim_library(path_out=None):
    """tests/lld_util.py's simulator build plus ksw2_host_lls.c (tests/llsim/lls_shim_sim.cpp compiles llf_shim_sim.cpp in and takes its
    place), ksw2_host_llds.c and tests/llsim/llds_shim_sim.cpp: every local-alignment entry of the library.  Returns the path of the .so."""
    dd = tempfile.mkdtemp(prefix="lldssim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "lls", "lld", "llds"):
        o = os.path.join(dd, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "lls_shim_sim.cpp"), "llssim.o"),
                   (os.path.join(HERE, "llsim", "lld_shim_sim.cpp"), "lldsim.o"), (os.path.join(HERE, "llsim", "llds_shim_sim.cpp"), "lldssim.o")):
        o = os.path.join(dd, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(dd, "libksw2_amd_lldssim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """(launches of k2a_shim_launch_lld_sub's twin with tasks, every other alignment launch, check launches) since the last reset"""
    L = lib.lib
    for f in (L.llds_sim_launches, L.lld_sim_launches, L.lls_sim_sub_launches, L.llf_sim_align_launches, L.llf_sim_check_launches):
        f.restype = ctypes.c_long
    if reset:
        L.llds_sim_reset_launches()
        L.lld_sim_reset_launches()
        L.lls_sim_reset_counters()
    return int(L.llds_sim_launches()), int(L.lld_sim_launches()) + int(L.lls_sim_sub_launches()) + int(L.llf_sim_align_launches()), int(L.llf_sim_check_launches())


# ---------------------------------------------------------------- inputs

def base_query(seed=77):
    """200 letters from {0, 1, 2}: letter 3 (the pad and the residues under a planted gap) matches nothing of it"""
    return np.random.default_rng(seed).integers(0, 3, 200, dtype=np.uint8)


def _pad(n):
    return np.full(n, 3, np.uint8)


def boundary_case(q, ln):
    """item 1: q[10:100] + ln pad rows + q[100:190] from row 930 on -- the gap's rows start at 1 020 and cross 1 023 -> 1 024 -- and q
    itself at rows 1 500..1 699 of an 1 800-row target of pad -> target"""
    t = _pad(1800)
    hit = np.concatenate([q[10:100], _pad(ln), q[100:190]])
    t[930:930 + len(hit)] = hit
    t[1500:1700] = q
    return t


BOUNDARY_SCORE2 = {19: (17958, 17958), 20: (17956, 17956), 21: (17955, 17954), 60: (17916, 17876)}      # ln -> (under CROSS, under (4, 2))


def window_case(q):
    """item 2: 300 rows of pad, then q[:100] + 60 pad rows + q[100:] -- under CROSS the gap costs 84 instead of 124, score 19 916 instead
    of 19 876, so d = 200 instead of 199 and the best row outside the window is 358 instead of 359"""
    return np.concatenate([_pad(300), q[:100], _pad(60), q[100:]]).astype(np.uint8)


def shoulder_case(q):
    """item 3: 900 rows of pad, q[:100] + 60 pad rows + q[100:] at rows 300..559, a copy of q[:80] ending at row 759"""
    t = _pad(900)
    t[300:560] = np.concatenate([q[:100], _pad(60), q[100:]])
    t[680:760] = q[:80]
    return t


def planted(q=None):
    """the twelve pairs of items 1 - 3, each also with query and target exchanged (qlen > tlen) -> (queries, targets)"""
    q = base_query() if q is None else q
    ts = [boundary_case(q, ln) for ln in (19, 20, 21, 60)] + [window_case(q), shoulder_case(q)]
    return [q] * len(ts) + ts, ts + [q] * len(ts)


def wide_query(rng):
    """qlen = 65 536 and 65 535 against a target of 70: the first does not fit the 16-bit column index (tests/lls_util.check_wide_query)"""
    t = rng.integers(0, 4, 70, dtype=np.uint8)
    q = rng.integers(0, 4, 65536, dtype=np.uint8)
    q[65536 - 30:] = t[40:]
    q[100:130] = t[:30]
    return [q, q[:65535]], [t, t]


def grid4():
    """item 4: the edge grid of tests/lls_util.py -> list of (name, queries, targets, mat, m, excl, every pair has score2 > 0)"""
    out = []
    q, t = s.generation_edges(np.random.default_rng(301))
    out.append(("generation_edges", q, t, M5, 5, -1, True))
    for k, (q, t, excl) in enumerate(s.window_edges(np.random.default_rng(303))):
        out.append(("window_edges_%d" % k, q, t, M5, 5, excl, False))
    rng = np.random.default_rng(304)
    q, t = s.differing_halves(rng)
    out.append(("differing_halves_5", q, t, M5, 5, -1, False))
    m20 = u.random_mat(rng, 20)
    q, t = s.differing_halves(rng, 20)
    out.append(("differing_halves_20", q, t, m20, 20, -1, False))
    q, t = s.tandem_repeats(np.random.default_rng(305))
    out.append(("tandem_repeats", q, t, M5, 5, -1, False))
    q, t = s.forced_orientation(np.random.default_rng(302))
    out.append(("forced_orientation", q, t, M5, 5, -1, True))
    q, t, mat, excl = s.wide_score(np.random.default_rng(312))
    out.append(("wide_score", q, t, mat, 5, excl, False))
    q, t = wide_query(np.random.default_rng(306))
    out.append(("wide_query", q, t, M5, 5, 3, True))
    return out


def ragged_set(costs, small=False):
    """300 pairs of lengths 1 - 600 plus 6 of up to 3 000, half of them with m = 5 and half with m = 20 -> [(queries, targets, mat, m)]"""
    rng = np.random.default_rng(900 + sum(costs))
    out = []
    for m in (5, 20):
        q, t = u.ragged(rng, 150, m, 1, 600)
        q2, t2 = u.ragged(rng, 3, m, 600, 3000)
        if small:                                      # what a lock-step simulator runs in seconds
            q, t, q2, t2 = q[::10], t[::10], [x[:700] for x in q2[:1]], [x[:900] for x in t2[:1]]
        out.append((q + q2, t + t2, M5 if m == 5 else u.random_mat(rng, 20), m))
    return out


def pin_sets(rng):
    """pairs whose target holds a second, weaker hit, so that score2 > 0 -> [(queries, targets, mat, m, costs)]"""
    m20 = u.random_mat(rng, 20)
    out = []
    for n, m, lo, hi, mat, costs in ((500, 5, 8, 160, M5, CROSS), (400, 20, 8, 120, m20, (6, 2, 10, 1)), (400, 4, 20, 200, M5, (4, 2, 8, 1)),
                                     (400, 5, 8, 120, M5, CHEAP2), (300, 5, 8, 120, M5, (0, 2, 3, 1))):
        q = [rng.integers(0, m, int(rng.integers(lo, hi + 1)), dtype=np.uint8) for _ in range(n)]
        t = [np.concatenate([u.mutate(rng, x, m, 0.03, 0.04), rng.integers(0, m, int(rng.integers(1, 40)), dtype=np.uint8),
                             u.mutate(rng, x, m, 0.08, 0.04), rng.integers(0, m, int(rng.integers(0, 20)), dtype=np.uint8)]) for x in q]
        out.append((q, t, mat, 5 if m == 4 else m, costs))
    return out


# ---------------------------------------------------------------- the checks of the grid: lib is the simulator build or the GPU library

def forms(monkeypatch, m=5):
    """every (form, lookup) combination of the switches (m > 5 takes the LDS lookup whatever the switch says: one value)"""
    for form in ("0", "1", "2"):
        for lds in ("0", "1") if m <= 5 else ("0",):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
            yield form, lds


def check(lib, q, t, mat, costs, excl=-1, m=None, positive=False, exp=None):
    """lld_sub_batch against the scalar oracle; res bit-identical to lld_batch -> the expected (n, 6) array"""
    exp = oracle_batch(q, t, mat, costs, excl, m) if exp is None else exp
    res, sub = lib.lld_sub_batch(q, t, mat, *costs, excl=excl, m=m)
    np.testing.assert_array_equal(res, exp[:, :3])
    np.testing.assert_array_equal(sub, exp[:, 3:])
    np.testing.assert_array_equal(res, lib.lld_batch(q, t, mat, *costs, m=m))
    if positive:
        assert (exp[:, 3] > 0).all(), exp
    return exp


def trace_line(err, m, lds):
    """the trace of a two-piece sub chunk: the lld: line, then the lld-sub: line, no single-piece line -> (pk_tasks, int32_tasks)"""
    lines = [l for l in err.splitlines() if "[ksw2_amd] ll" in l]
    assert len(lines) >= 2 and " lld: " in lines[0] and " lld-sub: " in lines[1], err
    assert " ll: " not in err and " ll-sub: " not in err and "-rev:" not in err, err
    g = re.search(r"lld-sub: pk_tasks=(\d+) int32_tasks=(\d+) profile=(\w+) excl=(-?\d+)( pk_profile=lds)?$", lines[1])
    assert g, lines[1]
    reg = lds == "0" and m <= 5
    assert g.group(3) == ("registers" if reg else "lds"), lines[1]
    assert (g.group(5) is not None) == (reg and not d_pk_reg()), lines[1]       # packed two-piece tasks take the LDS profile
    assert ("pk_profile=lds" in lines[0]) == (g.group(5) is not None), lines[0]
    return int(g.group(1)), int(g.group(2)), int(g.group(4))


def d_pk_reg():
    """K2A_LLD_PK_REG of ksw2_types.h"""
    src = open(os.path.join(ROOT, "ksw2_amd", "csrc", "ksw2_types.h")).read()
    return int(re.search(r"#define K2A_LLD_PK_REG (\d)", src).group(1))


def check_boundary(lib, monkeypatch, capfd):
    """item 1: the second piece changes score2 only, across the generation boundary"""
    q = base_query()
    mat = d.cross_mat(5)
    qs, ts = [], []
    for ln in (19, 20, 21, 60):
        qs += [q, q]                                   # twice: a packed partner
        ts += [boundary_case(q, ln)] * 2
    exp = oracle_batch(qs, ts, mat, CROSS)
    for k, ln in enumerate((19, 20, 21, 60)):
        assert exp[2 * k].tolist() == [20000, 199, 1699, BOUNDARY_SCORE2[ln][0], 189, 1109 + ln], (ln, exp[2 * k])
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form, lds in forms(monkeypatch):
        capfd.readouterr()
        res, sub = lib.lld_sub_batch(qs, ts, mat, *CROSS)
        pk, i32, _ = trace_line(capfd.readouterr().err, 5, lds)
        assert (pk, i32) == ((0, 8) if form == "0" else (4, 0)), (form, pk, i32)
        np.testing.assert_array_equal(np.hstack([res, sub]), exp)
        np.testing.assert_array_equal(res, lib.lld_batch(qs, ts, mat, *CROSS))
        check(lib, ts, qs, mat, CROSS)                 # qlen 1 800 > tlen 200: rows stay the target
    res1, sub1 = lib.ll_sub_batch(qs, ts, mat, 4, 2)
    for k, ln in enumerate((19, 20, 21, 60)):
        assert sub1[2 * k].tolist() == [BOUNDARY_SCORE2[ln][1], 189, 1109 + ln] and res1[2 * k].tolist() == [20000, 199, 1699]
        assert (sub1[2 * k].tolist() != exp[2 * k, 3:].tolist()) == (ln > 20), ln


def check_window(lib, monkeypatch):
    """item 2: the second piece changes score, hence d"""
    q = base_query()
    mat = d.cross_mat(5)
    t = window_case(q)
    assert len(t) == 560
    for form, lds in forms(monkeypatch):
        exp = check(lib, [q, q], [t, t], mat, CROSS)
        assert exp[0].tolist() == [19916, 199, 559, 5900, 58, 358], exp
        check(lib, [t, t], [q, q], mat, CROSS)
    res1, sub1 = lib.ll_sub_batch([q], [t], mat, 4, 2)
    assert res1[0].tolist() == [19876, 199, 559] and sub1[0].tolist() == [6000, 59, 359]


def check_shoulder(lib, monkeypatch):
    """item 3: gape2 = 1 < smax = 100 -- the default window ceil(19 916 / 100) = 200 ends at row 759, the shoulder of the best hit
    H(559 + k, 199) = 19 916 - (24 + k) does not: score2 is its row 760, a pad row, and not the hit of 8 000 that ends at row 759.
    An excl of (score - gapo2) / gape2 outlives it"""
    q = base_query()
    mat = d.cross_mat(5)
    t = shoulder_case(q)
    for form, lds in forms(monkeypatch):
        exp = check(lib, [q, q], [t, t], mat, CROSS)
        assert exp[0].tolist() == [19916, 199, 559, 19691, 199, 760], exp
        assert t[760] == 3
    exp = check(lib, [q], [t], mat, CROSS, excl=(19916 - 24) // 1)
    assert exp[0].tolist() == [19916, 199, 559, 0, -1, -1]
    exp = check(lib, [q], [t], mat, CROSS, excl=240)                        # a wider excl only moves score2 down the shoulder
    assert exp[0, 3:].tolist() == [19916 - (24 + 241), 199, 800]


def check_grid4(lib, monkeypatch, name):
    """item 4 (one entry of grid4() by the start of its name) under CROSS and CHEAP2, and item 6: equal pieces equal ll_sub_batch"""
    for nm, q, t, mat, m, excl, positive in grid4():
        if not nm.startswith(name):
            continue
        wide = nm == "wide_query"                     # 65 536 columns: the form that packs the admissible pair only (as lls_util.check_wide_query)
        for costs in COSTS:
            exp = oracle_batch(q, t, mat, costs, excl, m)
            for form, _ in forms(monkeypatch, m):
                if not wide or form == "2":
                    check(lib, q, t, mat, costs, excl, m, positive, exp)
        go, ge = (30, 10) if nm == "wide_score" else (4, 2)
        for form in ("2",) if wide else ("1", "0"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            res1, sub1 = lib.ll_sub_batch(q, t, mat, go, ge, excl=excl, m=m)
            for go2, ge2 in ((go, ge), (go + 5, ge), (127, 127)):
                res, sub = lib.lld_sub_batch(q, t, mat, go, ge, go2, ge2, excl=excl, m=m)
                np.testing.assert_array_equal(res, res1, nm)
                np.testing.assert_array_equal(sub, sub1, nm)


def check_shape_grid(lib, monkeypatch):
    """item 5: rows 15 / 16 / 17 / 33 / 1 025 against columns 1 / 2 / 63 / 65, in both orientations"""
    q, t = d.shape_grid(np.random.default_rng(41), 5, (15, 16, 17, 33, 1025), (1, 2, 63, 65))
    for costs in ((5, 3, 9, 1), CHEAP2):
        exp = oracle_batch(q, t, M5, costs, 2)
        for _ in forms(monkeypatch):
            check(lib, q, t, M5, costs, 2, exp=exp)
            check(lib, q, t, M5, costs)


def check_single(lib):
    """item 7: lld, lld_align and lld_sub equal row i of the batch entries on the twelve pairs of items 1 - 3"""
    qs, ts = planted()
    mat = d.cross_mat(5)
    res, sub = lib.lld_sub_batch(qs, ts, mat, *CROSS)
    np.testing.assert_array_equal(np.hstack([res, sub]), oracle_batch(qs, ts, mat, CROSS))
    alns = {flag: lib.lld_align_batch(qs, ts, mat, *CROSS, flag=flag) for flag in (0, d.SCORE_ONLY, d.RIGHT | d.REV_CIGAR)}
    assert len(qs) == 12
    for i in range(12):
        assert lib.lld(qs[i], ts[i], mat, *CROSS) == tuple(res[i].tolist())
        assert lib.lld_sub(qs[i], ts[i], mat, *CROSS) == (tuple(res[i].tolist()), tuple(sub[i].tolist()))
        assert lib.lld_sub(qs[i], ts[i], mat, *CROSS, excl=7)[1] == tuple(lib.lld_sub_batch(qs[i:i + 1], ts[i:i + 1], mat, *CROSS, excl=7)[1][0].tolist())
        for flag, al in alns.items():
            got = lib.lld_align(qs[i], ts[i], mat, *CROSS, flag=flag)
            assert got == al[i], (i, flag)
            assert (got["score"], got["qe"], got["te"]) == tuple(res[i].tolist()) and (got["n_cigar"] > 0) == (not flag & d.SCORE_ONLY)
    e = np.zeros(0, np.uint8)
    assert lib.lld(e, ts[0], mat, *CROSS) == (0, -1, -1) and lib.lld_sub(qs[0], e, mat, *CROSS) == ((0, -1, -1), (0, -1, -1))
    one, z = np.array([3], np.int8), np.zeros(9, np.uint8)                   # m = 1 is accepted by lld and the sub entries
    assert lib.lld(z, z, one, 1, 1, 2, 0, m=1) == (27, 8, 8)
    assert lib.lld_sub(z, z, one, 1, 1, 2, 0, excl=2, m=1) == ((27, 8, 8), (18, 5, 5))
    r, sb = lib.lld_sub_batch([z], [z], one, 1, 1, 2, 0, excl=2, m=1)
    assert r.tolist() == [[27, 8, 8]] and sb.tolist() == [[18, 5, 5]]


def check_ragged(lib, costs, small=False, monkeypatch=None):
    for q, t, mat, m in ragged_set(costs, small):
        if not small:
            assert len(q) == 153
        exp = oracle_batch(q, t, mat, costs, -1, m)
        if monkeypatch is None:
            check(lib, q, t, mat, costs, m=m, exp=exp)
        else:
            for _ in forms(monkeypatch, m):
                check(lib, q, t, mat, costs, m=m, exp=exp)
        assert (exp[:, 3] > 0).sum() > len(q) // 4


def check_flat(lib, placed, kinds, monkeypatch, launches_fn=None):
    """the flat entry against the pointer entry: every arena kind, one query shared by all pairs, a multi-chunk call, a bad code"""
    rng = np.random.default_rng(307)
    q, t = s.differing_halves(rng)
    q2, t2 = u.ragged(rng, 60, 5, 1, 400)
    q, t = q + q2, t + t2
    a = lf.arena(q, t, rng, lead=3, gap=5)
    res0, sub0 = lib.lld_sub_batch(q, t, M5, *CROSS)
    np.testing.assert_array_equal(np.hstack([res0, sub0]), oracle_batch(q, t, M5, CROSS))
    for kind in kinds:
        with placed(lib, a[0], kind) as kw:
            res, sub = lib.lld_sub_batch_flat(*a, M5, *CROSS, **kw)
            np.testing.assert_array_equal(res, res0)
            np.testing.assert_array_equal(sub, sub0)
    monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "20000")                    # several chunks
    res, sub = lib.lld_sub_batch_flat(*a, M5, *CROSS)
    np.testing.assert_array_equal(np.hstack([res, sub]), np.hstack([res0, sub0]))
    # a bad code in the last third: the chunks before it are done, res[] and sub[] hold the reset values from the failing chunk on
    base = a[0].copy()
    bad = len(q) - 10
    base[int(a[3][bad])] = 9
    out, so = np.full((len(q), 3), 7, np.int32), np.full((len(q), 3), 7, np.int32)
    try:
        lib.lld_sub_batch_flat(base, *a[1:], M5, *CROSS, out=out, sub=so)
        raise AssertionError("a residue code >= m was accepted")
    except Exception as e:
        assert "error -2" in str(e) and "pair %d" % bad in lib.last_error(), (e, lib.last_error())
    first = next(i for i in range(len(q)) if (out[i] == NONE).all() and (out[i:, 0] == 0).all())
    assert 0 < first <= bad
    np.testing.assert_array_equal(out[:first], res0[:first])
    np.testing.assert_array_equal(so[:first], sub0[:first])
    assert (out[first:] == NONE).all() and (so[first:] == NONE).all()
    monkeypatch.delenv("KSW2AMD_LL_CHUNK_BYTES")
    # the same in ONE chunk: the check comes before every alignment launch, so none happens
    if launches_fn is not None:
        before = launches_fn()
    out[:], so[:] = 7, 7
    try:
        lib.lld_sub_batch_flat(base, *a[1:], M5, *CROSS, out=out, sub=so)
        raise AssertionError("a residue code >= m was accepted")
    except Exception as e:
        assert "error -2" in str(e), e
    assert (out == NONE).all() and (so == NONE).all()
    if launches_fn is not None:
        assert launches_fn() == before
    # one query shared by all pairs
    qq = rng.integers(0, 4, 120, dtype=np.uint8)
    ts = [np.concatenate([u.mutate(rng, qq, 4), rng.integers(0, 4, 50, dtype=np.uint8), u.mutate(rng, qq, 4, 0.1)]) for _ in range(20)]
    b = lf.arena([qq], ts)
    qoff, qlen = np.repeat(b[1], 20), np.repeat(b[2], 20)
    res, sub = lib.lld_sub_batch_flat(b[0], qoff, qlen, b[3], b[4], M5, *CROSS)
    np.testing.assert_array_equal(np.hstack([res, sub]), oracle_batch([qq] * 20, ts, M5, CROSS))
    assert (sub[:, 0] > 0).all()


def check_bad_arguments(lib, Ksw2Error, launches_fn=None):
    """launches_fn: () -> the launches a simulator build has counted; every rejected or empty call must leave the count where it was"""
    import ksw2_amd
    _i8p = ctypes.POINTER(ctypes.c_int8)
    x = np.array([0, 1, 2, 3, 0, 1], np.uint8)
    one = [x]
    a_ok = lf.arena(one, one)
    before = launches_fn() if launches_fn else None
    bad_costs = [tuple(v if j == k else 2 for j in range(4)) for k in range(4) for v in (-1, 128)]
    cases = [(c, {}) for c in bad_costs] + [(CROSS, dict(excl=0x40000000)), (CROSS, dict(m=0)), (CROSS, dict(m=128))]
    for costs, kw in cases:
        for call in (lambda: lib.lld_sub_batch(one, one, M5, *costs, **kw), lambda: lib.lld_sub_batch_flat(*a_ok, M5, *costs, **kw)):
            try:
                call()
                raise AssertionError("accepted: %r %r" % (costs, kw))
            except Ksw2Error as e:
                assert "error -2" in str(e), e
        if "m" not in kw:                              # the single-pair entries report and return the reset values
            n0 = lib.error_count()
            assert lib.lld_sub(x, x, M5, *costs, **kw) == ((0, -1, -1), (0, -1, -1))
            assert lib.error_count() == n0 + 1
            if "excl" in kw:
                assert "excl" in lib.last_error()
            else:
                assert lib.lld(x, x, M5, *costs) == (0, -1, -1)
                g = lib.lld_align(x, x, M5, *costs)
                assert (g["score"], g["qb"], g["qe"], g["tb"], g["te"], g["n_cigar"]) == (0, -1, -1, -1, -1, 0)
                assert lib.error_count() == n0 + 3
    for call in (lambda: lib.lld_sub_batch(one, [np.array([0, 5], np.uint8)], M5, *CROSS),):        # a code >= m, found on the host
        try:
            call()
            raise AssertionError("a residue code >= m was accepted")
        except Ksw2Error as e:
            assert "error -2" in str(e) and "pair 0" in lib.last_error()
    # NULL arrays, a NULL profile
    L = lib.lib
    pairs, keep = lib.local_pairs(one, one)
    res, sub = (ksw2_amd.LocalResult * 1)(), (ksw2_amd.LocalSub * 1)()
    mp = np.ascontiguousarray(M5, np.int8).ctypes.data_as(_i8p)
    assert L.ksw2amd_lld_sub_batch(5, mp, 4, 2, 24, 1, -1, 1, None, res, sub) == -2
    assert L.ksw2amd_lld_sub_batch(5, mp, 4, 2, 24, 1, -1, 1, pairs, None, sub) == -2
    assert L.ksw2amd_lld_sub_batch(5, mp, 4, 2, 24, 1, -1, 1, pairs, res, None) == -2
    assert L.ksw2amd_lld_sub_batch(5, None, 4, 2, 24, 1, -1, 1, pairs, res, sub) == -2
    assert L.ksw2amd_lld_sub_batch_flat(5, mp, 4, 2, 24, 1, -1, 1, None, res, sub) == -2
    qe, te, sb, aln = ctypes.c_int(5), ctypes.c_int(5), ksw2_amd.LocalSub(7, 7, 7), ksw2_amd.LocalAln()
    tp = x.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    n0 = lib.error_count()
    assert L.ksw2amd_lld(None, 6, tp, 4, 2, 24, 1, ctypes.byref(qe), ctypes.byref(te)) == 0 and (qe.value, te.value) == (-1, -1)
    qe.value = te.value = 5
    assert L.ksw2amd_lld_sub(None, 6, tp, 4, 2, 24, 1, -1, ctypes.byref(qe), ctypes.byref(te), ctypes.byref(sb)) == 0
    assert (qe.value, te.value, sb.score2, sb.qe2, sb.te2) == (-1, -1, 0, -1, -1)
    aln.score, aln.qb, aln.n_cigar = 9, 9, 9
    assert L.ksw2amd_lld_align(None, None, 6, tp, 4, 2, 24, 1, 0, ctypes.byref(aln)) == 0
    assert (aln.score, aln.qb, aln.qe, aln.tb, aln.te, aln.n_cigar) == (0, -1, -1, -1, -1, 0)
    assert lib.error_count() == n0 + 3 and "NULL profile" in lib.last_error()
    # ksw2amd_lld_align on a profile with m = 1: ksw2amd_lld_align_batch rejects it
    z = np.zeros(9, np.uint8)
    n0 = lib.error_count()
    g = lib.lld_align(z, z, np.array([3], np.int8), 1, 1, 2, 0, m=1)
    assert (g["score"], g["qb"], g["qe"], g["tb"], g["te"], g["n_cigar"]) == (0, -1, -1, -1, -1, 0)
    assert lib.error_count() == n0 + 1 and "m >= 2" in lib.last_error()
    # nothing to do: n = 0, a matrix without a positive entry, empty sequences
    res, sub = lib.lld_sub_batch([], [], M5, *CROSS)
    assert res.shape == (0, 3) and sub.shape == (0, 3)
    res, sub = lib.lld_sub_batch(one, one, -np.abs(M5), *CROSS)
    assert res.tolist() == [NONE] and sub.tolist() == [NONE]
    e = np.zeros(0, np.uint8)
    res, sub = lib.lld_sub_batch(one + [e], [e] + one, M5, *CROSS)
    assert res.tolist() == [NONE] * 2 and sub.tolist() == [NONE] * 2
    if launches_fn:
        assert launches_fn() == before, (launches_fn(), before)             # nothing above reached a launch


def check_c_caller(so_dir, libname, tmp_path):
    """tests/dropin/llds_caller.c built against include/ksw2_amd.h: the batch call and the three single-pair calls print the oracle's numbers"""
    exe = str(tmp_path / "llds_caller")
    subprocess.run(["gcc", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(HERE, "dropin", "llds_caller.c"),
                    "-L" + so_dir, "-l" + libname, "-Wl,-rpath," + so_dir], check=True)
    rng = np.random.default_rng(309)
    q, t = u.ragged(rng, 10, 5, 1, 400)
    q2, t2 = s.generation_edges(rng)
    q, t = q + q2[:2], t + t2[:2]
    inp = str(tmp_path / "pairs.txt")
    with open(inp, "w") as f:
        f.write("5 %d %d %d %d -1\n%s\n%d\n" % (CROSS + (" ".join(str(int(x)) for x in M5), len(q))))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
    got = np.array([list(map(int, l.split())) for l in out.strip().splitlines()], dtype=np.int32)
    exp = oracle_batch(q, t, M5, CROSS)
    cells = d.start_cells(q, t, M5, CROSS, 5)                               # score, qb, qe, tb, te, s'
    third = np.column_stack([exp[:, 0], exp[:, 1], exp[:, 2], cells[:, 0], cells[:, 1], cells[:, 3]])
    np.testing.assert_array_equal(got, np.vstack([exp, exp, third]))


# ---------------------------------------------------------------- golden file (tests/golden/llds_cases.npz, written by tests/gen_llds_golden.py)

def golden_inputs():
    """-> list of (queries, targets, mat, m, costs, excl)"""
    rng = np.random.default_rng(20261)
    qs, ts = planted()
    out = [(qs[:6], ts[:6], d.cross_mat(5), 5, CROSS, -1)]
    q, t = d.shape_grid(rng, 5, (15, 16, 17, 33, 1025), (1, 2, 63, 65))
    out.append((q, t, M5, 5, (5, 3, 9, 1), 2))
    q, t = s.generation_edges(rng)
    out.append((q[::2], t[::2], M5, 5, CHEAP2, -1))
    q, t = s.differing_halves(rng, 20)
    out.append((q, t, u.random_mat(rng, 20), 20, CROSS, -1))
    q, t = u.ragged(rng, 16, 5, 1, 200)
    out.append((q, t, M5, 5, (0, 0, 0, 0), 0))
    return out


def save_golden(path, sets):
    """sets: (queries, targets, mat, m, costs, excl, expected (n, 6))"""
    z = {"nsets": np.int32(len(sets))}
    for k, (q, t, mat, m, costs, excl, exp) in enumerate(sets):
        z["s%d_par" % k] = np.array([m] + list(costs) + [excl], np.int32)
        z["s%d_mat" % k] = np.asarray(mat, np.int8)
        z["s%d_qlen" % k] = np.array([len(x) for x in q], np.int32)
        z["s%d_tlen" % k] = np.array([len(x) for x in t], np.int32)
        z["s%d_q" % k] = np.concatenate([np.asarray(x, np.uint8) for x in q])
        z["s%d_t" % k] = np.concatenate([np.asarray(x, np.uint8) for x in t])
        z["s%d_res" % k] = np.asarray(exp, np.int32)
    np.savez_compressed(path, **z)


def load_golden(path=GOLDEN):
    """-> list of (queries, targets, mat, m, costs, excl, expected (n, 6))"""
    z = np.load(path)
    out = []
    for k in range(int(z["nsets"])):
        par = [int(x) for x in z["s%d_par" % k]]
        ql, tl = z["s%d_qlen" % k], z["s%d_tlen" % k]
        qo, to = np.concatenate([[0], np.cumsum(ql)]), np.concatenate([[0], np.cumsum(tl)])
        q = [z["s%d_q" % k][qo[i]:qo[i + 1]] for i in range(len(ql))]
        t = [z["s%d_t" % k][to[i]:to[i + 1]] for i in range(len(tl))]
        out.append((q, t, z["s%d_mat" % k], par[0], tuple(par[1:5]), par[5], z["s%d_res" % k]))
    return out
