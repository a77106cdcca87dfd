"""Helpers of the tests of ksw2amd_ll_align_batch / ksw2amd_ll_align (local alignment with start cell and CIGAR): the simulator build with
the start-cell pass's twin (tests/llsim/lla_shim_sim.cpp), the contract's formula as an oracle (tests/ll_oracle.c forward and on the
reversed prefixes, then a global scalar ksw_extz on the interval -- the compiled reference where it is built, the project's own
restatement otherwise), a CIGAR re-scorer and the inputs that hit what the start-cell pass adds."""
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libksw2ref.so")
SCORE_ONLY, RIGHT, GENERIC_SC, REV_CIGAR = 0x01, 0x02, 0x04, 0x80


def sim_library(path_out=None):
    """tests/ll_util.py's simulator build plus ksw2_host_lla.c and tests/llsim/lla_shim_sim.cpp.  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="llasim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "ll_shim_sim.cpp"), "llsim.o"),
                   (os.path.join(HERE, "llsim", "lla_shim_sim.cpp"), "llasim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_llasim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def have_ref():
    return os.path.exists(REF_SO)


def global_extz(query, target, mat, m, gapo, gape, flag, which=None):
    """The scalar ksw_extz, unbanded, no Z-drop, KSW_EZ_GENERIC_SC | flag -> (score, CIGAR list); which: 'ref' / 'oracle' (default: the
    compiled reference where it is built)."""
    from oracle import pyoracle as po
    which = which or ("ref" if have_ref() else "oracle")
    r = po.align(which, "extz", query, target, mat, gapo, gape, w=-1, zdrop=-1, flag=GENERIC_SC | flag, m=m)
    return int(r["score"]), list(r["cigar"])


def start_cells(queries, targets, mat, gapo, gape, m, fwd=None):
    """(n, 6) int32 array score, qb, qe, tb, te, s' by the contract's formula: the scalar local oracle forward, then on the reversed
    prefixes that end in (qe, te)."""
    fwd = u.oracle_batch(queries, targets, mat, gapo, gape, m) if fwd is None else fwd
    n = len(queries)
    out = np.full((n, 6), -1, dtype=np.int32)
    out[:, 0] = 0
    out[:, 5] = 0
    pos = [i for i in range(n) if fwd[i][0] > 0]
    if pos:
        rq = [np.ascontiguousarray(np.asarray(queries[i], dtype=np.uint8)[:fwd[i][1] + 1][::-1]) for i in pos]
        rt = [np.ascontiguousarray(np.asarray(targets[i], dtype=np.uint8)[:fwd[i][2] + 1][::-1]) for i in pos]
        rev = u.oracle_batch(rq, rt, mat, gapo, gape, m)
        for k, i in enumerate(pos):
            s, qe, te = map(int, fwd[i])
            out[i] = (s, qe - int(rev[k][1]), qe, te - int(rev[k][2]), te, int(rev[k][0]))
    return out


def expected(queries, targets, mat, gapo, gape, m, flag=0, which=None):
    """The contract for every pair: list of dicts score, qb, qe, tb, te, n_cigar, cigar (+ gscore: the interval's global score)."""
    cells = start_cells(queries, targets, mat, gapo, gape, m)
    out = []
    for i in range(len(queries)):
        s, qb, qe, tb, te, s2 = map(int, cells[i])
        d = dict(score=s, qb=qb, qe=qe, tb=tb, te=te, n_cigar=0, cigar=[], gscore=s, rscore=s2)
        if s > 0 and not (flag & SCORE_ONLY):
            d["gscore"], d["cigar"] = global_extz(np.asarray(queries[i])[qb:qe + 1], np.asarray(targets[i])[tb:te + 1], mat, m, gapo, gape,
                                                  flag & (RIGHT | REV_CIGAR), which)
            d["n_cigar"] = len(d["cigar"])
        out.append(d)
    return out


FIELDS = ("score", "qb", "qe", "tb", "te", "n_cigar", "cigar")


def assert_same(got, exp, msg=""):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert e["rscore"] == e["score"] and e["gscore"] == e["score"], (msg, i, e)       # the formula's own consistency
        assert all(g[f] == e[f] for f in FIELDS), (msg, i, {f: g[f] for f in FIELDS}, {f: e[f] for f in FIELDS})


def rescore(cigar, query, target, mat, m, gapo, gape, rev=False):
    """(score, query residues consumed, target residues consumed) of a CIGAR over query / target (already cut to the interval)."""
    ops = list(cigar)[::-1] if rev else list(cigar)
    s = i = j = 0
    for c in ops:
        ln, op = c >> 4, c & 0xf
        if op == 0:
            for k in range(ln):
                s += int(mat[int(target[i + k]) * m + int(query[j + k])])
            i += ln
            j += ln
        elif op == 1:        # insertion: consumes the query
            s -= gapo + gape * ln
            j += ln
        elif op == 2:        # deletion: consumes the target
            s -= gapo + gape * ln
            i += ln
        else:
            raise AssertionError("unexpected CIGAR operation %d" % op)
    return s, j, i


def brute_global(q, t, mat, m, gapo, gape):
    """Global affine-gap score of q against t in plain Python (both non-empty)."""
    NEG = -(1 << 40)
    nq, nt = len(q), len(t)
    H = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    E = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    F = [[NEG] * (nq + 1) for _ in range(nt + 1)]
    H[0][0] = 0
    for j in range(1, nq + 1):
        H[0][j] = -(gapo + gape * j)
    for i in range(1, nt + 1):
        H[i][0] = -(gapo + gape * i)
        for j in range(1, nq + 1):
            E[i][j] = max(E[i - 1][j] - gape, H[i - 1][j] - gapo - gape)
            F[i][j] = max(F[i][j - 1] - gape, H[i][j - 1] - gapo - gape)
            H[i][j] = max(H[i - 1][j - 1] + int(mat[int(t[i - 1]) * m + int(q[j - 1])]), E[i][j], F[i][j])
    return H[nt][nq]


def brute_start(q, t, mat, m, gapo, gape):
    """(score, qb, qe, tb, te) by brute force: the forward tie rule of tests/ll_util.brute for the end cell, then among every (qb, tb)
    whose sub-rectangle's GLOBAL score equals the local score, the largest tb, then the largest qb."""
    s, qe, te = u.brute(q, t, mat, gapo, gape, m)
    if s <= 0:
        return 0, -1, -1, -1, -1
    cand = [(tb, qb) for tb in range(te + 1) for qb in range(qe + 1)
            if brute_global(q[qb:qe + 1], t[tb:te + 1], mat, m, gapo, gape) == s]
    tb, qb = max(cand)
    return s, qb, qe, tb, te


def _plant(rng, m, n, other, at, ln):
    """n random residues with other[0:ln] copied in at position `at`"""
    x = rng.integers(0, m, n, dtype=np.uint8)
    x[at:at + ln] = other[:ln]
    return x


def new_ground(rng, m, small=False):
    """Pairs that hit what the start-cell pass adds (queries, targets): same-shape packed partners whose end cells differ widely, in both
    orders of the halves and either orientation; rows above 1 024 with the halves' prefixes ending in different generations; a half
    with score 0 beside a positive partner; an alignment that ends in cell (0, 0); one spanning both full sequences; tandem repeats.
    Letters 0..min(m, 4)-1 carry the planted matches (m = 5: the last code is a wildcard)."""
    a = min(m, 4)
    qs, ts = [], []

    def add(q, t):
        qs.append(np.ascontiguousarray(q, dtype=np.uint8))
        ts.append(np.ascontiguousarray(t, dtype=np.uint8))

    for rows, cols in ((300, 200), (2600 if not small else 1300, 180)):
        for swap in (0, 1):
            for order in (0, 1):
                core = rng.integers(0, a, 40, dtype=np.uint8)
                near = (_plant(rng, a, cols, core, 2, 40), _plant(rng, a, rows, core, 3, 40))                       # ends near the origin
                far = (_plant(rng, a, cols, core, cols - 43, 40), _plant(rng, a, rows, core, rows - 45, 40))        # ... the far corner
                for c, r in ((near, far) if order == 0 else (far, near)):
                    add(r, c) if swap else add(c, r)          # swap: the query is the longer sequence (rows = the query)
    # a half with score 0 (no letter in common) beside a positive partner of the same shape
    z = np.zeros(150, np.uint8)
    add(z, np.ones(220, np.uint8))
    x = rng.integers(0, a, 150, dtype=np.uint8)
    add(x, _plant(rng, a, 220, x[50:], 100, 60))
    # ends in cell (0, 0): only the first residues match
    add(np.array([0] + [1] * 30, np.uint8), np.array([0] + [2] * 30, np.uint8))
    add(np.array([0] + [1] * 30, np.uint8), np.array([0] + [2] * 30, np.uint8))
    # spans both full sequences
    y = rng.integers(0, a, 180, dtype=np.uint8)
    add(y, y.copy())
    add(y[::-1], y[::-1].copy())
    # tie-heavy tandem repeats
    for k in range(6):
        unit = rng.integers(0, 2, int(rng.integers(1, 5)), dtype=np.uint8)
        add(np.tile(unit, 12), np.tile(unit, 40 + 300 * (k % 2)))
        add(np.tile(unit, 12), np.tile(unit, 40 + 300 * (k % 2)))
    q2, t2 = u.ragged(rng, 10, m, 1, 400)
    return qs + q2, ts + t2


def write_input(path, q, t, mat, m, go, ge, flag):
    with open(path, "w") as f:
        f.write("%d %d %d %d\n%s\n%d\n" % (m, go, ge, flag, " ".join(str(int(x)) for x in mat), len(q)))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))


def parse_caller(out):
    """lla_caller's output -> (batch dicts, single dicts, pool reallocs or None)"""
    parts, cur, pool = [[], []], 0, None
    for line in out.strip().splitlines():
        if line == "single":
            cur = 1
            continue
        if line.startswith("pool "):
            pool = int(line.split()[1])
            continue
        v = list(map(int, line.split()))
        parts[cur].append(dict(score=v[0], qb=v[1], qe=v[2], tb=v[3], te=v[4], n_cigar=v[5], cigar=v[6:]))
    return parts[0], parts[1], pool
