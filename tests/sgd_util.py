"""Helpers of the tests of the two-piece semi-global entries (ksw2amd_sgd_batch / ksw2amd_sgd_align_batch, their flat forms and the
single-pair entries; include/ksw2_amd.h): the scalar oracle tests/sgd_oracle.c compiled with gcc into a temporary
directory, a brute-force Python statement of the contract, the simulator build with the two launches' twin (tests/llsim/sgd_shim_sim.cpp),
the golden file that the compiled reference produced (tests/gen_sgd_golden.py), and the inputs that hit what the second piece adds to the
semi-global boundary.  costs = (gapo, gape, gapo2, gape2) throughout."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u
from tests import lla_util as la
from tests import lld_util as ld
from tests import sg_util as s
from tests import sga_util as a

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sgd_cases.npz")
SCORE_ONLY, RIGHT, GENERIC_SC, REV_CIGAR = la.SCORE_ONLY, la.RIGHT, la.GENERIC_SC, la.REV_CIGAR
FLAGS = a.FLAGS
FIELDS = a.FIELDS
CELLS = ("score", "qb", "qe", "tb", "te")
CROSS = ld.CROSS                  # (4, 2, 24, 1): the pieces cross at l = 20
# the second pieces of the golden file, one per group of tests/sg_util.golden_inputs(): both orders of the pieces, zeros, an equal pair
GOLDEN_COSTS = ((4, 2, 24, 1), (24, 1, 4, 2), (0, 1, 5, 0), (6, 3, 0, 0), (7, 3, 7, 3), (4, 2, 24, 1), (24, 1, 4, 2), (0, 1, 5, 0), (5, 0, 2, 1))
_oracle = None
gap_cost = ld.gap_cost
assert_same = a.assert_same


def oracle():
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "libsgd_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "sgd_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.sgd_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_cells(queries, targets, mat, costs, m=None):
    """(n, 5) int32 array of score, qb, qe, tb, te from the scalar oracle (it asserts that some x reaches the score on every pair)."""
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
    oracle().sgd_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                              m, mat.ctypes.data, *[int(c) for c in costs], out.ctypes.data)
    assert (out[:n, 5] == 1).all(), "no interval reaches the score on pairs %s" % np.nonzero(out[:n, 5] != 1)[0][:8]
    return out[:n, :5]


def oracle_batch(queries, targets, mat, costs, m=None):
    """(n, 3) int32 array of score, qe, te: what the score entries return"""
    return np.ascontiguousarray(oracle_cells(queries, targets, mat, costs, m)[:, [0, 2, 4]])


def _matrix(q, t, mat, costs, m, top, left):
    """H over full matrices in plain Python: top(j) = H(-1, j - 1), left(i) = H(i - 1, -1) for j, i >= 1; H[0][0] = 0"""
    go, ge, go2, ge2 = costs
    nq, nt = len(q), len(t)
    NEG = -(1 << 50)
    H = [[0 if (i == 0 and j == 0) else top(j) if i == 0 else left(i) if j == 0 else NEG for j in range(nq + 1)] for i in range(nt + 1)]
    E, F, E2, F2 = ([[NEG] * (nq + 1) for _ in range(nt + 1)] for _ in range(4))
    for i in range(1, nt + 1):
        for j in range(1, nq + 1):
            E[i][j] = max(E[i - 1][j] - ge, H[i - 1][j] - go - ge)
            F[i][j] = max(F[i][j - 1] - ge, H[i][j - 1] - go - ge)
            E2[i][j] = max(E2[i - 1][j] - ge2, H[i - 1][j] - go2 - ge2)
            F2[i][j] = max(F2[i][j - 1] - ge2, H[i][j - 1] - go2 - ge2)
            H[i][j] = max(H[i - 1][j - 1] + int(mat[t[i - 1] * m + q[j - 1]]), E[i][j], F[i][j], E2[i][j], F2[i][j])
    return H


def brute_global(q, t, mat, m, costs):
    q, t = list(map(int, q)), list(map(int, t))
    return _matrix(q, t, mat, costs, m, lambda j: -gap_cost(costs, j), lambda i: -gap_cost(costs, i))[len(t)][len(q)]


def brute(query, target, mat, costs, m):
    """(score, qb, qe, tb, te) in plain Python: the forward formula over full matrices and its tie rule, then G(x) for EVERY x in
    [0, te + 1] by a global matrix of its own, and the largest x whose G equals the score."""
    q, t = list(map(int, query)), list(map(int, target))
    nq, nt = len(q), len(t)
    if nq == 0:
        return 0, -1, -1, -1, -1
    if nt == 0:
        return -gap_cost(costs, nq), 0, nq - 1, 0, -1
    H = _matrix(q, t, mat, costs, m, lambda j: -gap_cost(costs, j), lambda i: 0)
    last = [H[i][nq] for i in range(1, nt + 1)]
    sc = max(last)
    te = min(i for i, v in enumerate(last) if v == sc)
    G = [brute_global(q, t[x:te + 1], mat, m, costs) for x in range(te + 1)] + [-gap_cost(costs, nq)]
    assert max(G) == sc, (G, sc)                 # no interval that ends in te beats the semi-global score
    return sc, 0, nq - 1, max(x for x, g in enumerate(G) if g == sc), te


def global_extd(query, target, mat, m, costs, flag, which=None):
    """The scalar ksw_extd, unbanded, no Z-drop, KSW_EZ_GENERIC_SC | flag -> (score, CIGAR list); which: 'ref' / 'oracle' (default: the
    compiled reference where it is built)."""
    from oracle import pyoracle as po
    go, ge, go2, ge2 = costs
    which = which or ("ref" if la.have_ref() else "oracle")
    r = po.align(which, "extd", query, target, mat, go, ge, go2, ge2, w=-1, zdrop=-1, flag=GENERIC_SC | flag, m=m)
    return int(r["score"]), list(r["cigar"])


def expected(queries, targets, mat, costs, m, flag=0, which=None, cells=None):
    """The contract for every pair: list of dicts score, qb, qe, tb, te, n_cigar, cigar (+ gscore: the interval's global score by the
    scalar ksw_extd)."""
    cells = oracle_cells(queries, targets, mat, costs, m) if cells is None else cells
    out = []
    for i in range(len(queries)):
        sc, qb, qe, tb, te = map(int, cells[i])
        d = dict(score=sc, qb=qb, qe=qe, tb=tb, te=te, n_cigar=0, cigar=[], gscore=sc)
        if qe >= 0 and not (flag & SCORE_ONLY):
            if tb <= te:
                d["gscore"], d["cigar"] = global_extd(np.asarray(queries[i]), np.asarray(targets[i])[tb:te + 1], mat, m, costs,
                                                      flag & (RIGHT | REV_CIGAR), which)
            else:
                d["cigar"] = [(qe + 1) << 4 | 1]
            d["n_cigar"] = len(d["cigar"])
        out.append(d)
    return out


def cells_of(got):
    return [[g[f] for f in CELLS] for g in got]


def sim_library(path_out=None):
    """tests/sga_util.py's simulator build plus ksw2_host_sgd.c and tests/llsim/sgd_shim_sim.cpp.  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="sgdsim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "sg", "sga", "sgd"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o"),
                   (os.path.join(HERE, "llsim", "sg_shim_sim.cpp"), "sgsim.o"), (os.path.join(HERE, "llsim", "sga_shim_sim.cpp"), "sgasim.o"),
                   (os.path.join(HERE, "llsim", "sgd_shim_sim.cpp"), "sgdsim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_sgdsim.so")
    subprocess.run(["g++", "-shared", "-Wl,-z,now", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """(two-piece forward launches, two-piece start-pass launches, launches of the single-piece semi-global and local twins, check
    launches) that had tasks since the last reset"""
    L = lib.lib
    for f in (L.sgd_sim_launches, L.sgd_sim_rev_launches, L.sg_sim_launches, L.sga_sim_launches, L.llf_sim_align_launches, L.llf_sim_check_launches):
        f.restype = ctypes.c_long
    if reset:
        L.sgd_sim_reset_launches()
        L.sg_sim_reset_launches()
        L.sga_sim_reset_launches()
        L.llf_sim_reset_counters()
    return (int(L.sgd_sim_launches()), int(L.sgd_sim_rev_launches()), int(L.sg_sim_launches()) + int(L.sga_sim_launches()) + int(L.llf_sim_align_launches()),
            int(L.llf_sim_check_launches()))


# ---- inputs
def other_letters(rng, n):
    """n residues over the codes {0, 1}: the queries of the planted inputs are over {2, 3}"""
    return rng.integers(0, 2, n, dtype=np.uint8)


def gapped_copy(rng, tlen, qlen, at, gap_at, gap_len, deletion, short_at=None):
    """A query of qlen over {2, 3} and a target of tlen over {0, 1} in which a copy of the query starts at row `at`.  deletion: gap_len
    residues of {0, 1} are put into the copy after its first gap_at residues (the path runs gap_len rows down one column: E / E2);
    else gap_len residues of the query, from gap_at on, are left out of the copy (the path runs along gap_len columns of one row: F / F2).
    short_at: query residue short_at is left out of the copy as well -- a gap of one, which the piece with the smaller open takes.
    -> query, target, (tb, te) of the copy"""
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    tail = q[gap_at:] if deletion else q[gap_at + gap_len:]
    if short_at is not None:
        k = short_at - (qlen - len(tail))
        assert 8 <= k < len(tail) - 8
        tail = np.concatenate([tail[:k], tail[k + 1:]])
    c = np.concatenate([q[:gap_at], other_letters(rng, gap_len) if deletion else q[:0], tail])
    t = other_letters(rng, tlen)
    assert at + len(c) <= tlen
    t[at:at + len(c)] = c
    return q, t, (at, at + len(c) - 1)


def suffix_copy(rng, qlen, skip, tail, mirror=False):
    """target = query[skip:] followed by `tail` residues of other codes: the optimum inserts the first `skip` query residues before
    target[0] (row -1 of the forward pass, at cost(skip)).  mirror: target = `tail` other residues, then query[:qlen - skip] -- the last
    `skip` query residues are inserted behind the copy, which the reverse pass meets first, along its row -1, and whose column -1 runs on
    for the whole copy."""
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    t = np.concatenate([other_letters(rng, tail), q[:qlen - skip]]) if mirror else np.concatenate([q[skip:], other_letters(rng, tail)])
    return q, t.astype(np.uint8)


def ragged_batch(rng, n=300, m=5, qmax=150, tmax=1300):
    """about n pairs, q 1..qmax x t 1..tmax, a third with a mutated copy of the query in the target, a few of one shape"""
    qs, ts = [], []
    for k in range(n):
        q = rng.integers(0, m, int(rng.integers(1, qmax + 1 if k % 7 else 9)), dtype=np.uint8)
        t = rng.integers(0, m, int(rng.integers(1, tmax + 1 if k % 5 else 40)), dtype=np.uint8)
        if k % 3 == 0:
            c = u.mutate(rng, q, m, 0.06, 0.05)
            at = int(rng.integers(0, len(t)))
            t = np.concatenate([t[:at], c, t[at:]])[:tmax].astype(np.uint8)
        qs.append(q); ts.append(t)
    qs += [qs[0], qs[1]]
    ts += [ts[0][::-1].copy(), ts[1][::-1].copy()]
    return qs, ts


def write_input(path, q, t, mat, m, costs, flag):
    """the input file of tests/dropin/sgd_caller.c"""
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n%s\n%d\n" % ((m,) + tuple(costs) + (flag, " ".join(str(int(x)) for x in mat), len(q))))
        for x, y in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(x), " ".join(map(str, x.tolist())), len(y), " ".join(map(str, y.tolist()))))


# ---- the golden file (tests/gen_sgd_golden.py writes it from the compiled reference; data only)
def save_golden(path, cases):
    """cases: [(name, costs, cells (n, 5), {flag: [cigar lists]})] in the order of tests/sg_util.golden_inputs(); the inputs stay in sg_cases.npz"""
    d = dict(ngroups=np.int32(len(cases)))
    for k, (name, costs, cells, cig) in enumerate(cases):
        p = "g%d_" % k
        d[p + "name"] = np.array(name)
        d[p + "costs"] = np.asarray(costs, dtype=np.int32)
        d[p + "cells"] = np.asarray(cells, dtype=np.int32)
        for fl in FLAGS:
            d[p + "ncig%d" % fl] = np.array([len(c) for c in cig[fl]], dtype=np.int32)
            d[p + "cig%d" % fl] = np.array([x for c in cig[fl] for x in c], dtype=np.uint32)
    np.savez_compressed(path, **d)


_golden = None


def load_golden():
    """[(name, m, mat, costs, queries, targets, cells (n, 5) score qb qe tb te, {flag: [cigar lists]})]: the inputs of
    tests/golden/sg_cases.npz, everything else of tests/golden/sgd_cases.npz.  Loaded once; treat it as read-only."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        out = []
        for k, (name, m, mat, gapo, gape, qs, ts, exp) in enumerate(s.load_golden()):
            p = "g%d_" % k
            assert str(z[p + "name"]) == name
            n = len(qs)
            cig = {}
            for fl in FLAGS:
                offs = np.concatenate([[0], np.cumsum(z[p + "ncig%d" % fl])])
                flat = z[p + "cig%d" % fl]
                cig[fl] = [[int(x) for x in flat[offs[i]:offs[i + 1]]] for i in range(n)]
            out.append((name, m, mat, tuple(int(x) for x in z[p + "costs"]), qs, ts, z[p + "cells"].astype(np.int32), cig))
        _golden = out
    return _golden
