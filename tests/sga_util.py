"""Helpers of the tests of ksw2amd_sg_align_batch / ksw2amd_sg_align_batch_flat / ksw2amd_sg_align (semi-global alignment with the start of
the interval and a CIGAR): the scalar oracle tests/sga_oracle.c compiled with gcc into a temporary directory, a brute-force Python statement
of "the largest x with G(x) == score", the simulator build with the start pass's twin (tests/llsim/sga_shim_sim.cpp), the golden file that
the compiled reference produced (tests/gen_sga_golden.py), and the inputs that put the interval where the reversed schedule changes hands."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u
from tests import lla_util as la
from tests import sg_util as s

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sga_cases.npz")
SCORE_ONLY, RIGHT, REV_CIGAR = la.SCORE_ONLY, la.RIGHT, la.REV_CIGAR
FLAGS = (0, RIGHT, REV_CIGAR)
FIELDS = ("score", "qb", "qe", "tb", "te", "n_cigar", "cigar")
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "libsga_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "sga_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.sga_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_cells(queries, targets, mat, gapo, gape, m=None):
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
    oracle().sga_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                              m, mat.ctypes.data, gapo, gape, out.ctypes.data)
    assert (out[:n, 5] == 1).all(), "no interval reaches the score on pairs %s" % np.nonzero(out[:n, 5] != 1)[0][:8]
    return out[:n, :5]


def brute(query, target, mat, gapo, gape, m):
    """(score, qb, qe, tb, te) in plain Python: tests/sg_util.brute for score and te, then G(x) for EVERY x in [0, te + 1] by a global
    matrix of its own, and the largest x whose G equals the score."""
    sc, qe, te = s.brute(query, target, mat, gapo, gape, m)
    nq = len(query)
    if nq == 0:
        return 0, -1, -1, -1, -1
    if len(target) == 0:
        return sc, 0, qe, 0, -1
    G = [la.brute_global(query, target[x:te + 1], mat, m, gapo, gape) for x in range(te + 1)] + [-(gapo + nq * gape)]
    assert max(G) == sc, (G, sc)                 # no interval that ends in te beats the semi-global score
    return sc, 0, qe, max(x for x, g in enumerate(G) if g == sc), te


def expected(queries, targets, mat, gapo, gape, m, flag=0, which=None, cells=None):
    """The contract for every pair: list of dicts score, qb, qe, tb, te, n_cigar, cigar (+ gscore: the interval's global score by the
    scalar ksw_extz -- the compiled reference where it is built, the project's restatement otherwise)."""
    cells = oracle_cells(queries, targets, mat, gapo, gape, m) if cells is None else cells
    out = []
    for i in range(len(queries)):
        sc, qb, qe, tb, te = map(int, cells[i])
        d = dict(score=sc, qb=qb, qe=qe, tb=tb, te=te, n_cigar=0, cigar=[], gscore=sc)
        if qe >= 0 and not (flag & SCORE_ONLY):
            if tb <= te:
                d["gscore"], d["cigar"] = la.global_extz(np.asarray(queries[i]), np.asarray(targets[i])[tb:te + 1], mat, m, gapo, gape,
                                                         flag & (RIGHT | REV_CIGAR), which)
            else:
                d["cigar"] = [(qe + 1) << 4 | 1]
            d["n_cigar"] = len(d["cigar"])
        out.append(d)
    return out


def assert_same(got, exp, msg=""):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert e["gscore"] == e["score"], (msg, i, e)            # the contract's own consistency
        assert all(g[f] == e[f] for f in FIELDS), (msg, i, {f: g[f] for f in FIELDS}, {f: e[f] for f in FIELDS})


def sim_library(path_out=None):
    """tests/sg_util.py's simulator build plus ksw2_host_sga.c and tests/llsim/sga_shim_sim.cpp.  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="sgasim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "sg", "sga"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o"),
                   (os.path.join(HERE, "llsim", "sg_shim_sim.cpp"), "sgsim.o"), (os.path.join(HERE, "llsim", "sga_shim_sim.cpp"), "sgasim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_sgasim.so")
    subprocess.run(["g++", "-shared", "-Wl,-z,now", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """(forward launches, start-pass launches, launches of the local twins, check launches) that had tasks since the last reset"""
    L = lib.lib
    for f in (L.sg_sim_launches, L.sga_sim_launches, L.llf_sim_align_launches, L.llf_sim_check_launches):
        f.restype = ctypes.c_long
    if reset:
        L.sg_sim_reset_launches()
        L.sga_sim_reset_launches()
        L.llf_sim_reset_counters()
    return int(L.sg_sim_launches()), int(L.sga_sim_launches()), int(L.llf_sim_align_launches()), int(L.llf_sim_check_launches())


# ---- inputs
def planted_copy(rng, m, tlen, qlen, te, sub=0.03, ind=0.0):
    """A random target of tlen over the codes {0, 1} and a query over {2, 3}; a lightly mutated copy of the query (of its tail where it
    does not fit) ends at target index te: the interval is about qlen long and ends at te."""
    t = rng.integers(0, 2, tlen, dtype=np.uint8)
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    c = q.copy()
    for k in range(len(c)):
        if 8 <= k < len(c) - 8 and rng.random() < sub:
            c[k] = 5 - c[k]                       # 2 <-> 3: a mismatch inside the copy, eight residues clear of its ends
    if rng.random() < ind and len(c) >= 60:       # (a shorter copy would rather shift and mismatch than open a gap)
        k = int(rng.integers(len(c) // 3, 2 * len(c) // 3))
        c = np.concatenate([c[:k], c[k + 1:]])    # one residue less in the middle: the interval is qlen - 1 long
    lo = max(0, te + 1 - len(c))
    t[lo:te + 1] = c[len(c) - (te + 1 - lo):]
    return q, t


def edge_cases(tlens=(17, 1025, 2049), qlens=(1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)):
    """[(tlen, qlen, te)]: the copy ends at te in {qlen - 1, 15, 16, 1 023, 1 024, tlen - 1} where that fits, so that rl = te + 1 lands
    on 16 / 17 / 1 024 / 1 025 and interval lengths on either side of a lane (16 rows) and of a generation (1 024 rows)"""
    out = []
    for tl in tlens:
        for ql in qlens:
            for te in sorted({ql - 1, 15, 16, 1023, 1024, tl - 1}):
                if 0 <= te < tl and ql <= te + 1:
                    out.append((tl, ql, te))
    return out


def edge_grid(rng, m, cases=None):
    qs, ts = [], []
    for k, (tl, ql, te) in enumerate(cases or edge_cases()):
        q, t = planted_copy(rng, m, tl, ql, te, ind=1.0 if k % 3 == 0 else 0.0)
        qs.append(q); ts.append(t)
    return qs, ts


def uneven_halves(rng, m, tlen=2100, qlen=40, ends=(45, 2090), tail=None):
    """Two pairs of ONE shape (a packed task under KSW2AMD_LL_FORM = 1) whose copies end at very different te"""
    qs, ts = [], []
    for te in ends:
        q, t = planted_copy(rng, m, tlen, qlen, te)
        qs.append(q); ts.append(t)
    return qs, ts


# ---- the golden file (tests/gen_sga_golden.py writes it from the compiled reference; data only)
def save_golden(path, cases):
    """cases: [(name, tb (n,) int32, {flag: [cigar lists]})] in the order of tests/sg_util.golden_inputs(); the inputs stay in sg_cases.npz"""
    d = dict(ngroups=np.int32(len(cases)))
    for k, (name, tb, cig) in enumerate(cases):
        p = "g%d_" % k
        d[p + "name"] = np.array(name)
        d[p + "tb"] = np.asarray(tb, dtype=np.int32)
        for fl in FLAGS:
            d[p + "ncig%d" % fl] = np.array([len(c) for c in cig[fl]], dtype=np.int32)
            d[p + "cig%d" % fl] = np.array([x for c in cig[fl] for x in c], dtype=np.uint32)
    np.savez_compressed(path, **d)


def load_golden():
    """[(name, m, mat, gapo, gape, queries, targets, cells (n, 5) score qb qe tb te, {flag: [cigar lists]})]: the inputs and score / te of
    tests/golden/sg_cases.npz, tb and the CIGARs of tests/golden/sga_cases.npz"""
    z = np.load(GOLDEN)
    out = []
    for k, (name, m, mat, gapo, gape, qs, ts, exp) in enumerate(s.load_golden()):
        p = "g%d_" % k
        assert str(z[p + "name"]) == name
        n = len(qs)
        cells = np.zeros((n, 5), np.int32)
        cells[:, 0], cells[:, 2], cells[:, 4], cells[:, 3] = exp[:, 0], exp[:, 1], exp[:, 2], z[p + "tb"]
        cig = {}
        for fl in FLAGS:
            offs = np.concatenate([[0], np.cumsum(z[p + "ncig%d" % fl])])
            flat = z[p + "cig%d" % fl]
            cig[fl] = [[int(x) for x in flat[offs[i]:offs[i + 1]]] for i in range(n)]
        out.append((name, m, mat, gapo, gape, qs, ts, cells, cig))
    return out
