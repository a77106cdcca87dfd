"""Helpers of the local-alignment tests (ksw_ll_qinit / ksw_ll_i16 / ksw2amd_ll_batch): the scalar oracle tests/ll_oracle.c compiled
with gcc into a temporary directory, a brute-force Python check of the tie rule, and random pair generators."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_oracle = None


def build_dir():
    d = os.path.join(tempfile.gettempdir(), "ksw2amd_ll_tests_%d" % os.getuid())
    os.makedirs(d, exist_ok=True)
    return d


def _compile(src, out, extra=()):
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, src] + list(extra), check=True)


def oracle():
    """ctypes handle of tests/ll_oracle.c (built once per process into a temp dir)."""
    global _oracle
    if _oracle is None:
        out = os.path.join(build_dir(), "libll_oracle_%d.so" % os.getpid())
        _compile(os.path.join(HERE, "ll_oracle.c"), out)
        lib = ctypes.CDLL(out)
        lib.ll_oracle_batch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
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
    oracle().ll_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                             m, mat.ctypes.data, gapo, gape, out.ctypes.data)
    return out[:n]


def brute(query, target, mat, gapo, gape, m):
    """Full-matrix local alignment in plain Python: every cell's H, then the tie rule applied to the set of maxima."""
    q, t = list(map(int, query)), list(map(int, target))
    NEG = -(1 << 40)
    H = [[0] * (len(q) + 1) for _ in range(len(t) + 1)]
    E = [[NEG] * (len(q) + 1) for _ in range(len(t) + 1)]
    F = [[NEG] * (len(q) + 1) for _ in range(len(t) + 1)]
    for i in range(1, len(t) + 1):
        for j in range(1, len(q) + 1):
            E[i][j] = max(E[i - 1][j] - gape, H[i - 1][j] - gapo - gape)
            F[i][j] = max(F[i][j - 1] - gape, H[i][j - 1] - gapo - gape)
            H[i][j] = max(0, H[i - 1][j - 1] + int(mat[t[i - 1] * m + q[j - 1]]), E[i][j], F[i][j])
    best = max(max(r) for r in H)
    if best <= 0:
        return 0, -1, -1
    cells = [(i - 1, j - 1) for i in range(1, len(t) + 1) for j in range(1, len(q) + 1) if H[i][j] == best]
    te, qe = min(cells)
    return best, qe, te


def simple_mat(m, match, mismatch, wild=None):
    """m x m match / mismatch matrix; the last code a wildcard scoring `wild` against everything when given."""
    a = np.full((m, m), -abs(mismatch), dtype=np.int8)
    np.fill_diagonal(a, match)
    if wild is not None:
        a[m - 1, :] = wild
        a[:, m - 1] = wild
    return a.reshape(-1)


def random_mat(rng, m, lo=-6, hi=7):
    a = rng.integers(lo, hi, size=(m, m)).astype(np.int8)
    return a.reshape(-1)


def mutate(rng, s, m, sub=0.05, ind=0.02):
    out = []
    for c in s:
        r = rng.random()
        if r < ind / 2:
            continue
        if r < ind:
            out.append(int(rng.integers(0, m)))
        out.append(int(rng.integers(0, m)) if rng.random() < sub else int(c))
    return np.array(out if out else [0], dtype=np.uint8)


def ragged(rng, n, m, lo, hi, related=0.5):
    """n pairs of random lengths in [lo, hi]; a fraction are mutated copies of each other (high local scores)."""
    qs, ts = [], []
    for _ in range(n):
        a = rng.integers(0, m, int(rng.integers(lo, hi + 1)), dtype=np.uint8)
        if rng.random() < related:
            b = mutate(rng, a, m)
            cut = int(rng.integers(0, max(1, len(b) // 4)))
            b = b[cut:]
            extra = rng.integers(0, m, int(rng.integers(0, max(1, hi - len(b) + 1) if hi > len(b) else 1)), dtype=np.uint8)
            b = np.concatenate([extra[: max(0, hi - len(b))], b])[:hi]
            if len(b) < lo:
                b = np.concatenate([b, rng.integers(0, m, lo - len(b), dtype=np.uint8)])
        else:
            b = rng.integers(0, m, int(rng.integers(lo, hi + 1)), dtype=np.uint8)
        qs.append(a)
        ts.append(b)
    return qs, ts


def sim_library(path_out=None):
    """A test-local simulator build of the product: tests/sim/ksw2_shim_sim.cpp and the host objects as they are, plus ksw2_host_ll.c and
    tests/llsim/ll_shim_sim.cpp (ksw2_lane_ll.h for 64 lanes in lock step).  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="llsim_", dir=build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "ll_shim_sim.cpp"), "llsim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_llsim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out
