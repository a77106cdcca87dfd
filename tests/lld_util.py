"""Helpers of the tests of the two-piece local-alignment entries (ksw2amd_lld_batch / ksw2amd_lld_align_batch and their flat forms): the
scalar oracle tests/lld_oracle.c compiled with gcc into a temporary directory, a brute-force Python statement of the definition, the
simulator build with the two-piece kernels' twin (tests/llsim/lld_shim_sim.cpp), the contract's formula (oracle forward and on the
reversed prefixes, then a global scalar ksw_extd on the interval), a CIGAR re-scorer under the two-piece cost, and the inputs that hit
what the second piece adds.  costs = (gapo, gape, gapo2, gape2) throughout."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u
from tests import lla_util as la

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "lld_cases.npz")
SCORE_ONLY, RIGHT, GENERIC_SC, REV_CIGAR = la.SCORE_ONLY, la.RIGHT, la.GENERIC_SC, la.REV_CIGAR
FIELDS = la.FIELDS
CROSS = (4, 2, 24, 1)            # the pieces cross at l = 20: 4 + 2 l = 24 + l
_oracle = None


def oracle():
    """ctypes handle of tests/lld_oracle.c (built once per process into a temp dir)."""
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "liblld_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "lld_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.lld_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_batch(queries, targets, mat, costs, m=None):
    """(n, 3) int32 array of score, qe, te from the scalar two-piece oracle."""
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
    oracle().lld_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                              m, mat.ctypes.data, *[int(c) for c in costs], out.ctypes.data)
    return out[:n]


def gap_cost(costs, ln):
    go, ge, go2, ge2 = costs
    return min(go + ge * ln, go2 + ge2 * ln)


def brute(query, target, mat, costs, m):
    """The definition in plain Python: every cell's H with unclamped E, F, E2, F2, then the tie rule applied to the set of maxima."""
    go, ge, go2, ge2 = costs
    q, t = list(map(int, query)), list(map(int, target))
    NEG = -(1 << 40)
    nq, nt = len(q), len(t)
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
    best = max(max(r) for r in H)
    if best <= 0:
        return 0, -1, -1
    te, qe = min((i - 1, j - 1) for i in range(1, nt + 1) for j in range(1, nq + 1) if H[i][j] == best)
    return best, qe, te


def sim_library(path_out=None):
    """tests/llf_util.py's simulator build plus ksw2_host_lld.c and tests/llsim/lld_shim_sim.cpp.  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="lldsim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "lld"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o"),
                   (os.path.join(HERE, "llsim", "lld_shim_sim.cpp"), "lldsim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_lldsim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """launches of the two-piece twins (with tasks) plus those of the single-piece twins since the last reset"""
    L = lib.lib
    L.lld_sim_launches.restype = ctypes.c_long
    L.llf_sim_align_launches.restype = ctypes.c_long
    L.llf_sim_check_launches.restype = ctypes.c_long
    if reset:
        L.lld_sim_reset_launches()
        L.llf_sim_reset_counters()
    return int(L.lld_sim_launches()), int(L.llf_sim_align_launches()), int(L.llf_sim_check_launches())


def global_extd(query, target, mat, m, costs, flag, which=None):
    """The scalar ksw_extd, unbanded, no Z-drop -> (score, CIGAR list); which: 'ref' / 'oracle' (default: the project's restatement)."""
    from oracle import pyoracle as po
    go, ge, go2, ge2 = costs
    r = po.align(which or "oracle", "extd", query, target, mat, go, ge, go2, ge2, w=-1, zdrop=-1, flag=flag, m=m)
    return int(r["score"]), list(r["cigar"])


def start_cells(queries, targets, mat, costs, m, fwd=None):
    """(n, 6) int32 array score, qb, qe, tb, te, s' by the contract's formula: the oracle forward, then on the reversed prefixes."""
    fwd = oracle_batch(queries, targets, mat, costs, m) if fwd is None else fwd
    n = len(queries)
    out = np.full((n, 6), -1, dtype=np.int32)
    out[:, 0] = 0
    out[:, 5] = 0
    pos = [i for i in range(n) if fwd[i][0] > 0]
    if pos:
        rq = [np.ascontiguousarray(np.asarray(queries[i], dtype=np.uint8)[:fwd[i][1] + 1][::-1]) for i in pos]
        rt = [np.ascontiguousarray(np.asarray(targets[i], dtype=np.uint8)[:fwd[i][2] + 1][::-1]) for i in pos]
        rev = oracle_batch(rq, rt, mat, costs, m)
        for k, i in enumerate(pos):
            s, qe, te = map(int, fwd[i])
            out[i] = (s, qe - int(rev[k][1]), qe, te - int(rev[k][2]), te, int(rev[k][0]))
    return out


def expected(queries, targets, mat, costs, m, flag=0, which=None):
    """The contract for every pair: list of dicts score, qb, qe, tb, te, n_cigar, cigar (+ gscore, rscore: the formula's own checks)."""
    cells = start_cells(queries, targets, mat, costs, m)
    out = []
    for i in range(len(queries)):
        s, qb, qe, tb, te, s2 = map(int, cells[i])
        d = dict(score=s, qb=qb, qe=qe, tb=tb, te=te, n_cigar=0, cigar=[], gscore=s, rscore=s2)
        if s > 0 and not (flag & SCORE_ONLY):
            d["gscore"], d["cigar"] = global_extd(np.asarray(queries[i])[qb:qe + 1], np.asarray(targets[i])[tb:te + 1], mat, m, costs,
                                                  flag & (RIGHT | REV_CIGAR), which)
            d["n_cigar"] = len(d["cigar"])
        out.append(d)
    return out


assert_same = la.assert_same


def rescore(cigar, query, target, mat, m, costs, rev=False):
    """(score, query residues consumed, target residues consumed) of a CIGAR under the two-piece cost."""
    ops = list(cigar)[::-1] if rev else list(cigar)
    s = i = j = 0
    for c in ops:
        ln, op = c >> 4, c & 0xf
        if op == 0:
            for k in range(ln):
                s += int(mat[int(target[i + k]) * m + int(query[j + k])])
            i += ln
            j += ln
        elif op == 1:
            s -= gap_cost(costs, ln)
            j += ln
        elif op == 2:
            s -= gap_cost(costs, ln)
            i += ln
        else:
            raise AssertionError("unexpected CIGAR operation %d" % op)
    return s, j, i


def check_cigars(got, queries, targets, mat, m, costs, flag=0):
    """every returned CIGAR covers its interval and re-scores to `score` under the two-piece cost; M at both ends when a gap costs"""
    go, ge, go2, ge2 = costs
    for i, g in enumerate(got):
        if g["score"] <= 0 or flag & SCORE_ONLY:
            assert g["n_cigar"] == 0
            continue
        qi, ti = np.asarray(queries[i])[g["qb"]:g["qe"] + 1], np.asarray(targets[i])[g["tb"]:g["te"] + 1]
        assert rescore(g["cigar"], qi, ti, mat, m, costs, rev=bool(flag & REV_CIGAR)) == (g["score"], len(qi), len(ti)), (i, g)
        if min(go + ge, go2 + ge2) > 0:
            assert g["cigar"][0] & 0xf == 0 and g["cigar"][-1] & 0xf == 0, (i, g)


# ---------------------------------------------------------------- inputs

def with_indel(rng, a, m, at, ln, insert):
    """a copy of `a` with `ln` residues inserted at `at` (insert) or removed from there (else).  The inserted residues are drawn from
    the letters so that they do not extend the flanking matches by accident more than chance allows."""
    a = np.asarray(a, dtype=np.uint8)
    if insert:
        return np.concatenate([a[:at], rng.integers(0, m, ln, dtype=np.uint8), a[at:]]).astype(np.uint8)
    return np.concatenate([a[:at], a[at + ln:]]).astype(np.uint8)


def cross_mat(m):
    """+100 / -100: one matched residue pays for any planted gap (at most 24 + 60), and unrelated sequence drifts down"""
    a = np.full((m, m), -100, dtype=np.int8)
    np.fill_diagonal(a, 100)
    return a.reshape(-1)


def crossover_pairs(rng, m, big=True):
    """Pairs under cross_mat(m) and costs CROSS (the second piece takes over above l = 20) whose best alignment holds ONE planted gap of
    length 19, 20, 21 or 60.  Rows are the longer sequence, the columns a window of it around the gap, in both orientations:
      * a vertical gap (E / E2: residues missing from the columns' sequence) over rows 12.., crossing the lane hand-over 15 -> 16, and
        (big) over rows 1 020.., crossing the generation boundary 1 023 -> 1 024;
      * a horizontal gap (F / F2: residues added to the columns' sequence) between rows 15 and 16, and (big) 1 023 and 1 024;
      * a gap that starts in column 0: one matched residue in column 0, then a vertical gap in that column; and the same with a
        horizontal gap from column 1 on.
    -> (queries, targets, gap length of every pair)"""
    qs, ts, lns = [], [], []
    assert m >= 4

    def add(cols, rows, ln):
        assert len(cols) <= len(rows)
        qs.append(np.ascontiguousarray(cols, np.uint8)); ts.append(np.ascontiguousarray(rows, np.uint8)); lns.append(ln)      # rows = target
        qs.append(np.ascontiguousarray(rows, np.uint8)); ts.append(np.ascontiguousarray(cols, np.uint8)); lns.append(ln)      # rows = query

    # the flanks use letters 0..2, the residues under the gap are all 3: nothing but the planted gap joins the flanks
    gap = lambda ln: np.full(ln, 3, np.uint8)
    for ln in (19, 20, 21, 60):
        for rows, at in ((260, 12), (1300, 1020)) if big else ((260, 12),):
            base = rng.integers(0, 3, rows, dtype=np.uint8)
            w0 = max(0, at - 100)
            add(np.concatenate([base[w0:at], base[at + ln:at + ln + 100]]), np.concatenate([base[:at], gap(ln), base[at + ln:]]), ln)
            at = (at + 15) // 16 * 16
            w0 = max(0, at - 100)
            add(np.concatenate([base[w0:at], gap(ln), base[at:at + 100]]), base, ln)
        base = rng.integers(0, 3, 260, dtype=np.uint8)
        add(np.concatenate([base[5:6], base[6 + ln:150]]), np.concatenate([base[:6], gap(ln), base[6 + ln:]]), ln)
        add(np.concatenate([base[5:6], gap(ln), base[6:100]]), base, ln)
    return qs, ts, lns


def shape_grid(rng, m, rows_list, cols_list, related=True):
    """one pair per (rows, cols) and orientation: the columns' sequence is a mutated piece of the rows' (so gaps of both kinds occur)"""
    qs, ts = [], []
    for r in rows_list:
        for c in cols_list:
            a = rng.integers(0, m, r, dtype=np.uint8)
            lo = int(rng.integers(0, max(1, r - c)))
            b = u.mutate(rng, a[lo:lo + c], m, 0.05, 0.06)[:c] if related else rng.integers(0, m, c, dtype=np.uint8)
            if len(b) < c:
                b = np.concatenate([b, rng.integers(0, m, c - len(b), dtype=np.uint8)])
            qs.append(b); ts.append(a)                               # rows = target
            qs.append(a); ts.append(b)                               # qlen > tlen: rows = query
    return qs, ts


def decoy(rng, m, n=6):
    return u.ragged(rng, n, m, 20, 120)


# ---------------------------------------------------------------- golden file (tests/golden/lld_cases.npz, written by tests/gen_lld_golden.py)

def golden_inputs():
    """the cases of the golden file: (name, m, mat, costs, queries, targets)"""
    rng = np.random.default_rng(20260)
    m5 = u.simple_mat(5, 2, 4, -1)
    m20 = u.random_mat(np.random.default_rng(3), 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(m20, 3)
    m20 = m20.reshape(-1)
    out = []
    q, t, _ = crossover_pairs(rng, 5, big=True)
    out.append(("cross5", 5, cross_mat(5), CROSS, q, t))
    q, t, _ = crossover_pairs(rng, 20, big=False)
    out.append(("cross20", 20, cross_mat(20), CROSS, q, t))
    q, t = shape_grid(rng, 5, (15, 16, 17, 33, 1025), (1, 2, 63, 65))
    out.append(("grid5", 5, m5, (5, 3, 9, 1), q, t))
    q, t = u.ragged(rng, 24, 20, 1, 300)
    out.append(("cheap2", 20, m20, (6, 3, 2, 1), q, t))
    q, t = u.ragged(rng, 16, 5, 1, 200)
    out.append(("zero", 5, m5, (0, 0, 0, 0), q, t))
    return out


def save_golden(path, cases):
    """cases: (name, m, mat, costs, queries, targets, expected dicts)"""
    d = {"names": np.array([c[0] for c in cases])}
    for name, m, mat, costs, q, t, exp in cases:
        d[name + "_m"] = np.int32(m)
        d[name + "_mat"] = np.asarray(mat, np.int8)
        d[name + "_costs"] = np.asarray(costs, np.int32)
        d[name + "_seq"] = np.concatenate([np.asarray(x, np.uint8) for x in list(q) + list(t)] + [np.zeros(0, np.uint8)])
        d[name + "_len"] = np.array([len(x) for x in list(q) + list(t)], np.int32)
        d[name + "_cells"] = np.array([[e["score"], e["qb"], e["qe"], e["tb"], e["te"], e["n_cigar"]] for e in exp], np.int32).reshape(-1, 6)
        d[name + "_cigar"] = np.array([c for e in exp for c in e["cigar"]], np.uint32)
    np.savez_compressed(path, **d)


def load_golden(path=GOLDEN):
    z = np.load(path)
    out = []
    for name in [str(x) for x in z["names"]]:
        lens = z[name + "_len"]
        offs = np.concatenate([[0], np.cumsum(lens)])
        seqs = [z[name + "_seq"][offs[k]:offs[k + 1]] for k in range(len(lens))]
        n = len(lens) // 2
        cells, cig, exp, pos = z[name + "_cells"], z[name + "_cigar"], [], 0
        for i in range(n):
            s, qb, qe, tb, te, nc = map(int, cells[i])
            exp.append(dict(score=s, qb=qb, qe=qe, tb=tb, te=te, n_cigar=nc, cigar=[int(c) for c in cig[pos:pos + nc]], gscore=s, rscore=s))
            pos += nc
        out.append((name, int(z[name + "_m"]), z[name + "_mat"], tuple(int(c) for c in z[name + "_costs"]), seqs[:n], seqs[n:], exp))
    return out
