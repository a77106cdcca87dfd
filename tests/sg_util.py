"""Helpers of the semi-global alignment tests (ksw2amd_sg_batch / ksw2amd_sg_batch_flat / ksw2amd_sg): the scalar oracle
tests/sg_oracle.c compiled with gcc into a temporary directory, a brute-force Python statement of the formula and its tie rule, the
simulator build with the semi-global kernels' twin (tests/llsim/sg_shim_sim.cpp), the golden file that the compiled reference produced
(tests/gen_sg_golden.py), and the inputs that put the best row where the schedule changes hands."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "sg_cases.npz")
_oracle = None


def oracle():
    """ctypes handle of tests/sg_oracle.c (built once per process into a temp dir)."""
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "libsg_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "sg_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.sg_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_batch(queries, targets, mat, gapo, gape, m=None):
    """(n, 3) int32 array of score, qe, te from the scalar oracle."""
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    m = int(round(len(mat) ** 0.5)) if m is None else m
    n = len(queries)
    seqs = [np.ascontiguousarray(x, dtype=np.uint8) for x in list(queries) + list(targets)]
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    base = np.concatenate(seqs + [np.zeros(1, np.uint8)]).astype(np.uint8)
    qoff, toff = np.ascontiguousarray(offs[:n]), np.ascontiguousarray(offs[n:2 * n])
    qlen, tlen = lens[:n].astype(np.int32), lens[n:].astype(np.int32)
    out = np.zeros((max(n, 1), 3), dtype=np.int32)
    oracle().sg_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                             m, mat.ctypes.data, gapo, gape, out.ctypes.data)
    return out[:n]


def brute(query, target, mat, gapo, gape, m):
    """The formula in plain Python over full matrices, then the tie rule applied to the set of maxima of the last column."""
    q, t = list(map(int, query)), list(map(int, target))
    nq, nt = len(q), len(t)
    if nq == 0:
        return 0, -1, -1
    if nt == 0:
        return -(gapo + nq * gape), nq - 1, -1
    NEG = -(1 << 50)
    H = [[0] + [-(gapo + j * gape) if i == 0 else NEG for j in range(1, nq + 1)] for i in range(nt + 1)]
    E = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    F = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    for i in range(1, nt + 1):
        for j in range(1, nq + 1):
            E[i][j] = max(E[i - 1][j] - gape, H[i - 1][j] - gapo - gape)
            F[i][j] = max(F[i][j - 1] - gape, H[i][j - 1] - gapo - gape)
            H[i][j] = max(H[i - 1][j - 1] + int(mat[t[i - 1] * m + q[j - 1]]), E[i][j], F[i][j])
    last = [H[i][nq] for i in range(1, nt + 1)]
    best = max(last)
    return best, nq - 1, min(i for i, v in enumerate(last) if v == best)


def sim_library(path_out=None):
    """tests/llf_util.py's simulator build plus ksw2_host_sg.c and tests/llsim/sg_shim_sim.cpp.  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="sgsim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "sg"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o"),
                   (os.path.join(HERE, "llsim", "sg_shim_sim.cpp"), "sgsim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_sgsim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """(launches of the semi-global twin that had tasks, launches of the local twins, check launches) since the last reset"""
    L = lib.lib
    L.sg_sim_launches.restype = ctypes.c_long
    L.llf_sim_align_launches.restype = ctypes.c_long
    L.llf_sim_check_launches.restype = ctypes.c_long
    if reset:
        L.sg_sim_reset_launches()
        L.llf_sim_reset_counters()
    return int(L.sg_sim_launches()), int(L.llf_sim_align_launches()), int(L.llf_sim_check_launches())


def load_golden():
    """[(name, m, mat, gapo, gape, queries, targets, expected (n, 3) array)] from tests/golden/sg_cases.npz"""
    z = np.load(GOLDEN)
    out = []
    for k in range(int(z["ngroups"])):
        p = "g%d_" % k
        ql, tl, seq = z[p + "qlen"], z[p + "tlen"], z[p + "seq"]
        offs = np.concatenate([[0], np.cumsum(np.concatenate([ql, tl]))]).astype(np.int64)
        n = len(ql)
        qs = [seq[offs[i]:offs[i + 1]].copy() for i in range(n)]
        ts = [seq[offs[n + i]:offs[n + i + 1]].copy() for i in range(n)]
        m, gapo, gape = (int(x) for x in z[p + "par"])
        out.append((str(z[p + "name"]), m, z[p + "mat"].astype(np.int8), gapo, gape, qs, ts, z[p + "exp"].astype(np.int32)))
    return out


# ---- inputs
def unit_mat(m, match=2, mismatch=4):
    return u.simple_mat(m, match, mismatch)


def planted(rng, m, tlen, qlen, end):
    """A random target of tlen over the codes {0, 1} and a query over the codes {2, 3} whose copy (where qlen > end + 1: its last end + 1
    residues) replaces target[.. end]: under a match / mismatch matrix no other row can score as much, the best row is `end`."""
    t = rng.integers(0, 2, tlen, dtype=np.uint8)
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    lo = max(0, end - qlen + 1)
    t[lo:end + 1] = q[qlen - (end + 1 - lo):]
    return q, t


def edge_rows(tlen):
    """the rows where the schedule changes hands, inside a target of tlen: last row of a lane, first of the next, last of generation 0,
    first of generation 1, last row of the target"""
    return sorted({r for r in (15, 16, 1023, 1024, tlen - 1) if 0 <= r < tlen})


def edge_grid(rng, m, tlens=(1, 15, 16, 17, 1023, 1024, 1025, 2049), qlens=(1, 2, 3, 4, 5, 63, 64, 65)):
    qs, ts = [], []
    for tl in tlens:
        for ql in qlens:
            for r in edge_rows(tl):
                q, t = planted(rng, m, tl, ql, r)
                qs.append(q); ts.append(t)
    return qs, ts


def tie_pairs(m=5):
    """The query twice in a target of a letter it does not hold, the copies ending at rows (a, b) on either side of a lane boundary
    (15, 16), of a generation boundary (1 023, 1 024), and far apart: two rows tie for the best score, the smaller is the answer.
    -> queries, targets, the expected te"""
    qs, ts, tes = [], [], []
    q = np.array([0, 1, 2, 1, 0, 2], dtype=np.uint8)
    for a, b, tl in ((15, 16 + 6, 40), (9, 16, 40), (1023, 1024 + 6, 1100), (1017, 1024, 1100), (15, 2047, 2100)):
        t = np.full(tl, 3, dtype=np.uint8)
        t[a - 5:a + 1] = q
        t[b - 5:b + 1] = q
        qs.append(q); ts.append(t); tes.append(a)
    return qs, ts, tes


# ---- the golden file (tests/gen_sg_golden.py writes it from the compiled reference; data only)
def golden_inputs():
    """[(name, m, mat, gapo, gape, queries, targets)]: a few hundred pairs of at most 120 x 400 -- m 2..6 and 20, gapo = 0 and gape = 0
    among the costs, matrices without a positive entry, a third of the pairs with a (mutated) copy of the query planted in the target"""
    rng = np.random.default_rng(20)
    out = []
    sets = [("m5", 5, u.simple_mat(5, 2, 4, -1), 4, 2), ("m2_gapo0", 2, u.random_mat(rng, 2), 0, 1), ("m3_gape0", 3, u.random_mat(rng, 3), 3, 0),
            ("m4_free_gaps", 4, u.simple_mat(4, 3, 2), 0, 0), ("m6", 6, u.random_mat(rng, 6), 7, 3), ("m20", 20, u.random_mat(rng, 20), 6, 1),
            ("m4_nonpositive", 4, u.random_mat(rng, 4, -6, 1), 2, 1), ("m5_negative", 5, u.random_mat(rng, 5, -9, 0), 0, 2),
            ("m20_nonpositive", 20, u.random_mat(rng, 20, -4, 1), 5, 0)]
    for name, m, mat, gapo, gape in sets:
        qs, ts = [], []
        for k in range(36):
            q = rng.integers(0, m, int(rng.integers(1, 121 if k % 6 else 13)), dtype=np.uint8)
            t = rng.integers(0, m, int(rng.integers(1, 401 if k % 4 else 30)), dtype=np.uint8)
            if k % 3 == 0:                          # a copy of the query, mutated, somewhere in the target (cut at its end)
                c = u.mutate(rng, q, m, 0.08, 0.06)
                at = int(rng.integers(0, len(t)))
                t = np.concatenate([t[:at], c, t[at:]])[:400].astype(np.uint8)
            qs.append(q); ts.append(t)
        out.append((name, m, mat, gapo, gape, qs, ts))
    return out


def save_golden(path, cases):
    d = dict(ngroups=np.int32(len(cases)))
    for k, (name, m, mat, gapo, gape, qs, ts, exp) in enumerate(cases):
        p = "g%d_" % k
        d[p + "name"] = np.array(name)
        d[p + "par"] = np.array([m, gapo, gape], dtype=np.int32)
        d[p + "mat"] = np.asarray(mat, dtype=np.int8)
        d[p + "qlen"] = np.array([len(x) for x in qs], dtype=np.int32)
        d[p + "tlen"] = np.array([len(x) for x in ts], dtype=np.int32)
        d[p + "seq"] = np.concatenate(list(qs) + list(ts)).astype(np.uint8)
        d[p + "exp"] = np.asarray(exp, dtype=np.int32)
    np.savez_compressed(path, **d)
