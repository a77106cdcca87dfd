"""Helpers of the overlap alignment tests (ksw2amd_ov_batch / ksw2amd_ovd_batch, their flat forms and the single-pair entries;
include/ksw2_amd.h): the scalar oracle tests/ov_oracle.c compiled with gcc into a temporary directory, a brute-force
Python statement of the contract and its tie rule, the simulator build with the two launches' twin (tests/llsim/ov_shim_sim.cpp), the golden
file that the compiled reference produced (tests/gen_ov_golden.py), and the inputs that put the best cell where the last-row maximum and the
free first row change hands.  costs = (gapo, gape) or (gapo, gape, gapo2, gape2) throughout; ends = KSW2AMD_OV_QBEG | KSW2AMD_OV_QEND."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import ksw2_amd
from tests import ll_util as u
from tests import sg_util as s
from tests import sgd_util as d

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "ov_cases.npz")
QBEG, QEND = ksw2_amd.KSW2AMD_OV_QBEG, ksw2_amd.KSW2AMD_OV_QEND      # the bits of `ends` as the binding names them
assert (QBEG, QEND) == (1, 2)                                           # ... and as tests/ov_oracle.c reads them
ENDS = (1, 2, 3)
_oracle = None


def four(costs):
    """(gapo, gape, gapo2, gape2): a single piece stands twice"""
    costs = tuple(int(c) for c in costs)
    return costs if len(costs) == 4 else costs + costs


def gap_cost(costs, l):
    go, ge, go2, ge2 = four(costs)
    return min(go + l * ge, go2 + l * ge2)


def oracle():
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "libov_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "ov_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.ov_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_batch(queries, targets, mat, costs, ends, m=None):
    """(n, 3) int32 array of score, qe, te from the scalar oracle."""
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    m = int(round(len(mat) ** 0.5)) if m is None else m
    n = len(queries)
    seqs = [np.ascontiguousarray(x, dtype=np.uint8) for x in list(queries) + list(targets)]
    lens = np.array([len(x) for x in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    base = np.concatenate(seqs + [np.zeros(1, np.uint8)]).astype(np.uint8)
    qoff, toff = np.ascontiguousarray(offs[:n]), np.ascontiguousarray(offs[n:2 * n])
    qlen, tlen = lens[:n].astype(np.int32), lens[n:].astype(np.int32)
    out = np.zeros((max(n, 1), 3), dtype=np.int32)
    oracle().ov_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                             m, mat.ctypes.data, *four(costs), int(ends), out.ctypes.data)
    return out[:n]


def pick(cands):
    """the tie rule on a list of (H, te, qe): the largest H, then the smallest te, then the smallest qe"""
    sc, te, qe = min(cands, key=lambda c: (-c[0], c[1], c[2]))
    return sc, qe, te


def brute(query, target, mat, costs, ends, m):
    """(score, qe, te) in plain Python: full matrices with unclamped gap states, the candidate cells listed one by one, the tie rule."""
    q, t = list(map(int, query)), list(map(int, target))
    nq, nt = len(q), len(t)
    c4 = four(costs)
    if nq == 0:
        return 0, -1, -1
    if nt == 0:
        return (0 if ends & QBEG else -gap_cost(c4, nq)), nq - 1, -1
    H = d._matrix(q, t, mat, c4, m, (lambda j: 0) if ends & QBEG else (lambda j: -gap_cost(c4, j)), lambda i: 0)
    cands = [(H[i][nq], i - 1, nq - 1) for i in range(1, nt + 1)]
    if ends & QEND:
        cands += [(H[nt][j], nt - 1, j - 1) for j in range(1, nq + 1)]
    return pick(cands)


def call(lib, q, t, mat, costs, ends, m):
    """ov_batch or ovd_batch by the length of costs"""
    costs = tuple(int(c) for c in costs)
    return lib.ov_batch(list(q), list(t), mat, costs[0], costs[1], ends, m=m, costs2=costs[2:] if len(costs) == 4 else None)


def call_flat(lib, arena, mat, costs, ends, m, **kw):
    costs = tuple(int(c) for c in costs)
    return lib.ov_batch_flat(*arena, mat, costs[0], costs[1], ends, m=m, costs2=costs[2:] if len(costs) == 4 else None, **kw)


def sim_library(path_out=None):
    """tests/sgd_util.py's simulator build plus ksw2_host_ov.c and tests/llsim/ov_shim_sim.cpp.  Returns the path of the .so."""
    dd = tempfile.mkdtemp(prefix="ovsim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "sg", "sga", "sgd", "ov"):
        o = os.path.join(dd, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o"),
                   (os.path.join(HERE, "llsim", "sg_shim_sim.cpp"), "sgsim.o"), (os.path.join(HERE, "llsim", "sga_shim_sim.cpp"), "sgasim.o"),
                   (os.path.join(HERE, "llsim", "sgd_shim_sim.cpp"), "sgdsim.o"), (os.path.join(HERE, "llsim", "ov_shim_sim.cpp"), "ovsim.o")):
        o = os.path.join(dd, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(dd, "libksw2_amd_ovsim.so")
    subprocess.run(["g++", "-shared", "-Wl,-z,now", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """(single-piece overlap launches, two-piece overlap launches, launches of every other alignment twin, check launches) that had tasks
    since the last reset"""
    L = lib.lib
    for f in (L.ov_sim_launches, L.ovd_sim_launches, L.sgd_sim_launches, L.sgd_sim_rev_launches, L.sg_sim_launches, L.sga_sim_launches,
              L.llf_sim_align_launches, L.llf_sim_check_launches):
        f.restype = ctypes.c_long
    if reset:
        L.ov_sim_reset_launches()
        L.sgd_sim_reset_launches()
        L.sg_sim_reset_launches()
        L.sga_sim_reset_launches()
        L.llf_sim_reset_counters()
    other = int(L.sgd_sim_launches()) + int(L.sgd_sim_rev_launches()) + int(L.sg_sim_launches()) + int(L.sga_sim_launches()) + int(L.llf_sim_align_launches())
    return int(L.ov_sim_launches()), int(L.ovd_sim_launches()), other, int(L.llf_sim_check_launches())


def pk_tasks(err, name="ov"):
    """(pk_tasks, int32_tasks) of every trace line of the entry in a captured stderr"""
    import re
    return [(int(a), int(b)) for a, b in re.findall(r"\] %s: pairs=\d+ pk_tasks=(\d+) int32_tasks=(\d+)" % name, err)]


# ---- inputs: targets over the codes {0, 1}, queries over {2, 3}, so that only a planted copy matches
TLENS = (1, 2, 8, 15, 16, 17, 31, 32, 1023, 1024, 1025, 1040, 2047, 2049)
QLENS = (1, 2, 5, 63, 64, 65, 130)


def prefix_lengths(qlen):
    """p: the query's first p residues are the target's last p; p - 1 around the 4-step prefetch and the 63-step skew, and at the corner"""
    return sorted({p for p in (1, 2, 3, 4, 5, 63, 64, 65, qlen - 1, qlen) if 1 <= p <= qlen})


def qend_pair(rng, tlen, qlen, p):
    """the target ends with the query's first p residues (as many of them as the target holds): with the query's end free the best cell
    is (tlen - 1, min(p, tlen) - 1) under a match / mismatch matrix"""
    t = rng.integers(0, 2, tlen, dtype=np.uint8)
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    k = min(p, tlen)
    t[tlen - k:] = q[p - k:p]
    return q, t


def qend_grid(rng, tlens=TLENS, qlens=QLENS):
    """-> queries, targets, [(tlen, qlen, p)]"""
    qs, ts, what = [], [], []
    for tl in tlens:
        for ql in qlens:
            for p in prefix_lengths(ql):
                q, t = qend_pair(rng, tl, ql, p)
                qs.append(q); ts.append(t); what.append((tl, ql, p))
    return qs, ts, what


def qbeg_pair(rng, tlen, qlen, s_):
    """the target starts with the query's last s_ residues: with the query's start free the best cell is (s_ - 1, qlen - 1)"""
    t = rng.integers(0, 2, tlen, dtype=np.uint8)
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    t[:s_] = q[qlen - s_:]
    return q, t


def qbeg_grid(rng):
    """s_ - 1 on both sides of rows 15 / 16 and 1 023 / 1 024 (queries long enough to hang over), and a whole copy in the middle of the
    target, whose score a free start must not change -> queries, targets, [(tlen, qlen, s_ or -row)]"""
    qs, ts, what = [], [], []
    for tl, ql, s_ in ((40, 30, 15), (40, 30, 16), (40, 30, 17), (40, 17, 16), (1100, 1100, 1023), (1100, 1100, 1024), (1100, 1100, 1025),
                       (2100, 1030, 1024), (1, 5, 1), (16, 64, 16), (1024, 1030, 1024)):
        q, t = qbeg_pair(rng, tl, ql, s_)
        qs.append(q); ts.append(t); what.append((tl, ql, s_))
    for tl, ql, end in ((200, 20, 100), (1100, 64, 1023), (1100, 64, 1024), (2100, 33, 1500)):
        q, t = s.planted(rng, 5, tl, ql, end)
        qs.append(q); ts.append(t); what.append((tl, ql, -end))
    return qs, ts, what


def both_pairs(rng, n=60, ov=25):
    """a suffix-prefix overlap in both orientations, a contained query, a contained target -> queries, targets, kinds"""
    a = rng.integers(2, 4, n, dtype=np.uint8)
    x = lambda k: rng.integers(0, 2, k, dtype=np.uint8)
    qs = [np.concatenate([x(n - ov), a[:ov]]), np.concatenate([a[n - ov:], x(n - ov)]), a[10:40].copy(), np.concatenate([x(20), a, x(30)])]
    ts = [np.concatenate([a[:ov], x(n - ov)]), np.concatenate([x(n - ov), a[n - ov:]]), np.concatenate([x(700), a, x(500)]), a[5:50].copy()]
    return qs, ts, ["query suffix = target prefix", "query prefix = target suffix", "query contained", "target contained"]


def tie_cases():
    """-> queries, targets, ends, expected (score, qe, te) under unit_mat(5) = +2 / -4 and costs (4, 2).  Code 4 scores -4 against everything
    but itself and does not occur in the queries."""
    W = lambda *a: np.array(a, np.uint8)
    out = []
    # the last column at row 8 < tlen - 1 (the whole query with one mismatch: 6 * 2 - 4) against the last row (the query's first four
    # residues: 4 * 2), equal scores: the last column's cell, its te is smaller
    out.append((W(0, 1, 2, 3, 1, 0, 2), W(4, 4, 0, 1, 2, 3, 1, 4, 2, 4, 4, 4, 0, 1, 2, 3), 2, (8, 6, 8)))
    # two equal maxima in the last row, H(4, 1) = H(4, 4) = 4: the smaller column
    out.append((W(0, 1, 3, 0, 1, 3, 3), W(4, 4, 4, 0, 1), 3, (4, 1, 4)))
    out.append((W(0, 1, 3, 0, 1, 3, 3), W(4, 4, 4, 0, 1), 2, (4, 1, 4)))
    # the corner (tlen - 1, qlen - 1) against a smaller column of the last row, H(4, 1) = H(4, 4) = 4: the smaller column
    out.append((W(0, 1, 3, 0, 1), W(4, 4, 4, 0, 1), 3, (4, 1, 4)))
    out.append((W(0, 1, 3, 0, 1), W(4, 4, 4, 0, 1), 2, (4, 1, 4)))
    qs, ts, es, exp = [c[0] for c in out], [c[1] for c in out], [c[2] for c in out], [c[3] for c in out]
    return qs, ts, es, exp


def ragged_batch(rng, n=4000, m=5, qmax=200, tmax=1500, long_targets=40):
    """n pairs, queries 1..qmax x targets 1..tmax plus long_targets targets of 4 000 - 5 000; a third of the pairs with a mutated query prefix
    at the target's tail or a mutated query suffix at its head"""
    qs, ts = [], []
    for k in range(n):
        q = rng.integers(0, m, int(rng.integers(1, qmax + 1 if k % 7 else 9)), dtype=np.uint8)
        tl = int(rng.integers(4000, 5001)) if k < long_targets else int(rng.integers(1, tmax + 1 if k % 5 else 40))
        t = rng.integers(0, m, tl, dtype=np.uint8)
        if k % 3 == 0:
            p = int(rng.integers(1, len(q) + 1))
            if k % 2:
                c = u.mutate(rng, q[:p], m, 0.06, 0.05)[:tl]
                if len(c):
                    t[tl - len(c):] = c
            else:
                c = u.mutate(rng, q[len(q) - p:], m, 0.06, 0.05)[:tl]
                if len(c):
                    t[:len(c)] = c
        qs.append(q); ts.append(t.astype(np.uint8))
    return qs, ts


def write_input(path, q, t, mat, m, costs):
    """the input file of tests/dropin/ov_caller.c"""
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n%s\n%d\n" % ((m,) + four(costs) + (" ".join(str(int(x)) for x in mat), len(q))))
        for x, y in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(x), " ".join(map(str, x.tolist())), len(y), " ".join(map(str, y.tolist()))))


# ---- the golden file (tests/gen_ov_golden.py writes it from the compiled reference; data only: the expected (score, qe, te) arrays)
def save_golden(path, single, dual):
    """single / dual: per group of tests/sg_util.golden_inputs() a dict ends -> (n, 3) array"""
    out = dict(ngroups=np.int32(len(single)))
    for k, (a, b) in enumerate(zip(single, dual)):
        for e in ENDS:
            out["g%d_ov%d" % (k, e)] = np.asarray(a[e], dtype=np.int32)
            out["g%d_ovd%d" % (k, e)] = np.asarray(b[e], dtype=np.int32)
    np.savez_compressed(path, **out)


_golden = None


def load_golden():
    """[(name, m, mat, (gapo, gape), (gapo, gape, gapo2, gape2), queries, targets, {ends: exp}, {ends: exp two-piece})]: the inputs of
    tests/golden/sg_cases.npz, the second pieces of tests/golden/sgd_cases.npz, the expected arrays of tests/golden/ov_cases.npz.  Loaded
    once; treat it as read-only."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        out = []
        for k, (g, gd) in enumerate(zip(s.load_golden(), d.load_golden())):
            name, m, mat, gapo, gape, qs, ts, _ = g
            out.append((name, m, mat, (gapo, gape), gd[3], qs, ts, {e: z["g%d_ov%d" % (k, e)].astype(np.int32) for e in ENDS},
                        {e: z["g%d_ovd%d" % (k, e)].astype(np.int32) for e in ENDS}))
        assert len(out) == int(z["ngroups"])
        _golden = out
    return _golden
