"""Helpers of the tests of ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch, their flat forms and the single-pair entries (overlap alignment
with the start cell and a CIGAR; include/ksw2_amd.h): the scalar oracle tests/ova_oracle.c compiled with gcc into a
temporary directory, a brute-force Python statement of the contract (full matrices, every candidate start cell, the tie rule), the simulator
build with the two start-pass launches' twin (tests/llsim/ova_shim_sim.cpp), the golden file that the compiled reference produced
(tests/gen_ova_golden.py), and the inputs that put the start cell where the reversed schedule changes hands.  costs = (gapo, gape) or
(gapo, gape, gapo2, gape2) throughout, as in tests/ov_util.py, which this module builds on."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u
from tests import lla_util as la
from tests import ov_util as ov
from tests import sgd_util as d

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "ova_cases.npz")
SCORE_ONLY, RIGHT, REV_CIGAR = la.SCORE_ONLY, la.RIGHT, la.REV_CIGAR
GOLDEN_FLAGS = (0, RIGHT)
FIELDS = ("score", "qb", "qe", "tb", "te", "n_cigar", "cigar")
CELLS = ("score", "qb", "qe", "tb", "te")
QBEG, QEND, ENDS = ov.QBEG, ov.QEND, ov.ENDS
four, gap_cost = ov.four, ov.gap_cost
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "libova_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "ova_oracle.c"), os.path.join(HERE, "ov_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.ova_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_cells(queries, targets, mat, costs, ends, m=None):
    """(n, 5) int32 array of score, qb, qe, tb, te from the scalar oracle (it asserts that some candidate reaches the score on every pair)."""
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
    oracle().ova_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                              m, mat.ctypes.data, *four(costs), int(ends), out.ctypes.data)
    assert (out[:n, 5] == 1).all(), "no start cell reaches the score on pairs %s" % np.nonzero(out[:n, 5] != 1)[0][:8]
    return out[:n, :5]


def candidates(qe, te, ends):
    """the candidate start cells (tb, qb) in the contract's order: the largest tb first, then the largest qb"""
    out = [(tb, 0) for tb in range(te + 1, 0, -1)]
    if ends & QBEG:
        out += [(0, qb) for qb in range(qe + 1, 0, -1)]
    return out + [(0, 0)]


def brute_G(q, t, mat, m, c4, tb, qb, qe, te):
    """the global score of query[qb..qe] against target[tb..te]; an empty interval costs the other one as a single gap"""
    if tb > te:
        return -gap_cost(c4, qe - qb + 1)
    if qb > qe:
        return -gap_cost(c4, te - tb + 1)
    return d.brute_global(q[qb:qe + 1], t[tb:te + 1], mat, m, c4)


def brute(query, target, mat, costs, ends, m):
    """(score, qb, qe, tb, te) in plain Python: tests/ov_util.brute for (score, qe, te), then G of EVERY candidate start cell by a global
    matrix of its own, the assertion that their maximum is the score, and the tie rule."""
    sc, qe, te = ov.brute(query, target, mat, costs, ends, m)
    q, t = list(map(int, query)), list(map(int, target))
    c4 = four(costs)
    if len(q) == 0:
        return 0, -1, -1, -1, -1
    if len(t) == 0:
        return sc, (len(q) if ends & QBEG else 0), qe, 0, -1
    cands = candidates(qe, te, ends)
    G = [brute_G(q, t, mat, m, c4, tb, qb, qe, te) for tb, qb in cands]
    assert max(G) == sc, (G, sc)                 # no candidate beats the forward score, and one reaches it
    tb, qb = cands[G.index(sc)]
    return sc, qb, qe, tb, te


def global_ext(query, target, mat, m, costs, flag, which=None):
    """the scalar ksw_extz (four costs: ksw_extd) on the whole of query x target -> (score, CIGAR list)"""
    costs = tuple(int(c) for c in costs)
    if len(costs) == 2:
        return la.global_extz(query, target, mat, m, costs[0], costs[1], flag, which)
    return d.global_extd(query, target, mat, m, costs, flag, which)


def expected(queries, targets, mat, costs, ends, m, flag=0, which=None, cells=None):
    """The contract for every pair: list of dicts score, qb, qe, tb, te, n_cigar, cigar (+ gscore: the intervals' global score by the scalar
    ksw_extz / ksw_extd -- the compiled reference where it is built, the project's restatement otherwise)."""
    cells = oracle_cells(queries, targets, mat, costs, ends, m) if cells is None else cells
    out = []
    for i in range(len(queries)):
        sc, qb, qe, tb, te = map(int, cells[i])
        e = dict(score=sc, qb=qb, qe=qe, tb=tb, te=te, n_cigar=0, cigar=[], gscore=sc)
        if qe >= 0 and not (flag & SCORE_ONLY):
            if tb <= te and qb <= qe:
                e["gscore"], e["cigar"] = global_ext(np.asarray(queries[i])[qb:qe + 1], np.asarray(targets[i])[tb:te + 1], mat, m, costs,
                                                     flag & (RIGHT | REV_CIGAR), which)
            elif qb > qe and te >= 0:
                e["cigar"] = [(te + 1) << 4 | 2]
            elif qb <= qe:
                e["cigar"] = [(qe + 1) << 4 | 1]
            e["n_cigar"] = len(e["cigar"])
        out.append(e)
    return out


def assert_same(got, exp, msg=""):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert e["gscore"] == e["score"], (msg, i, e)            # the contract's own consistency
        assert all(g[f] == e[f] for f in FIELDS), (msg, i, {f: g[f] for f in FIELDS}, {f: e[f] for f in FIELDS})


def cells_of(got):
    return [[g[f] for f in CELLS] for g in got]


def call(lib, q, t, mat, costs, ends, m, flag=0, **kw):
    """ov_align_batch, single- or two-piece by the length of costs"""
    costs = tuple(int(c) for c in costs)
    return lib.ov_align_batch(list(q), list(t), mat, costs[0], costs[1], ends, flag=flag, m=m, costs2=costs[2:] if len(costs) == 4 else None, **kw)


def call_flat(lib, arena, mat, costs, ends, m, flag=0, **kw):
    costs = tuple(int(c) for c in costs)
    return lib.ov_align_batch_flat(*arena, mat, costs[0], costs[1], ends, flag=flag, m=m, costs2=costs[2:] if len(costs) == 4 else None, **kw)


def sim_library(path_out=None):
    """tests/ov_util.py's simulator build plus ksw2_host_ova.c and tests/llsim/ova_shim_sim.cpp.  Returns the path of the .so."""
    dd = tempfile.mkdtemp(prefix="ovasim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "sg", "sga", "sgd", "ov", "ova"):
        o = os.path.join(dd, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o"),
                   (os.path.join(HERE, "llsim", "sg_shim_sim.cpp"), "sgsim.o"), (os.path.join(HERE, "llsim", "sga_shim_sim.cpp"), "sgasim.o"),
                   (os.path.join(HERE, "llsim", "sgd_shim_sim.cpp"), "sgdsim.o"), (os.path.join(HERE, "llsim", "ov_shim_sim.cpp"), "ovsim.o"),
                   (os.path.join(HERE, "llsim", "ova_shim_sim.cpp"), "ovasim.o")):
        o = os.path.join(dd, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(dd, "libksw2_amd_ovasim.so")
    subprocess.run(["g++", "-shared", "-Wl,-z,now", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def launches(lib, reset=False):
    """(forward overlap launches of both kinds, start-pass launches of both kinds, launches of every other alignment twin, check launches)
    that had tasks since the last reset"""
    L = lib.lib
    for f in (L.ova_sim_launches, L.ovda_sim_launches):
        f.restype = ctypes.c_long
    if reset:
        L.ova_sim_reset_launches()
    a, b, other, chk = ov.launches(lib, reset)
    return a + b, int(L.ova_sim_launches()) + int(L.ovda_sim_launches()), other, chk


def trace_tasks(err, name):
    """(pk_tasks, int32_tasks) of every `name-rev:` trace line in a captured stderr"""
    import re
    return [(int(a), int(b)) for a, b in re.findall(r"\] %s-rev: pk_tasks=(\d+) int32_tasks=(\d+)" % name, err)]


# ---- inputs: targets over the codes {0, 1}, queries over {2, 3}, so that only a planted copy matches
def start_row_pair(rng, tlen, span, empty=False):
    """The query is `span` residues long and its copy fills target[te - span + 1 .. te] with te = tlen - 1 (ends = 0 or QEND alike): the
    start pass's best row is span - 1, tb = te - span + 1.  empty: no copy at all and a query of one residue, dearer to align than to
    insert under a mismatch of -4 and costs (1, 1)."""
    t = rng.integers(0, 2, tlen, dtype=np.uint8)
    q = rng.integers(2, 4, 1 if empty else span, dtype=np.uint8)
    if not empty:
        t[tlen - span:] = q
    return q, t


def qbeg_start_pair(rng, te, qb, qlen):
    """The target (te + 1 residues) is a copy of query[qb .. qb + te]; with the query's start free the best start is (0, qb) and the last
    row of the reversed rectangle is row te"""
    q = rng.integers(2, 4, qlen, dtype=np.uint8)
    assert qb + te + 1 <= qlen
    t = q[qb:qb + te + 1].copy()
    return q, t


def tie_cases():
    """-> queries, targets, ends, expected (score, qb, qe, tb, te) under unit_mat(5) = +2 / -4 and costs (4, 2), written out by hand.
    Code 4 scores -4 against everything but itself."""
    W = lambda *a: np.array(a, np.uint8)
    out = []
    # row 0 against the corner: query 0 1 0, target 1 0, start free.  Cell (te 1, qe 2) = 4 by "1 0" x "1 0": G(0, 1) = 4, the corner
    # G(0, 0) = 4 - 6 and G(1, 0) = "0 1 0" x "0" = 2 - 8 lose
    out.append((W(0, 1, 0), W(1, 0), 1, (4, 1, 2, 0, 1)))
    # a homopolymer: query 0 0 0, target 0 0, start free.  Cell (1, 2) = 4 by the last two residues, qb = 1; the corner pays a gap
    out.append((W(0, 0, 0), W(0, 0), 1, (4, 1, 2, 0, 1)))
    # a start inside the target beats the corner and row 0: query 0 1, target 3 0 1, both ends free.  Cell (2, 1) = 4; G(1, 0) = 4
    # (target 0 1), G(0, 0) = 4 - 6: tb = 1
    out.append((W(0, 1), W(3, 0, 1), 3, (4, 0, 1, 1, 2)))
    # two copies in row 0: query 0 1 3 0 1, target 0 1, start free, end fixed.  Cell (1, 4) = 4 by the second 0 1: qb = 3, the shortest
    # query interval; qb = 0 would be "0 1 3 0 1" x "0 1" = 4 - 10
    out.append((W(0, 1, 3, 0, 1), W(0, 1), 1, (4, 3, 4, 0, 1)))
    # ... with the end free as well the forward cell is (1, 1), the smaller qe, whose only start is the corner (0, 0)
    out.append((W(0, 1, 3, 0, 1), W(0, 1), 3, (4, 0, 1, 0, 1)))
    # the corner (0, 0) against a larger qb: query 2 0 1, target 0 1, start free.  Cell (1, 2) = 4; G(0, 1) = 4, G(0, 0) = 4 - 6
    out.append((W(2, 0, 1), W(0, 1), 1, (4, 1, 2, 0, 1)))
    # the empty target interval: two mismatches cost what inserting both residues costs, -8 = -cost(2).  te = 0 is the smallest row that
    # reaches it, and of its starts G(1, 0) = -8 and G(0, 0) = -4 - 6 the empty interval is the one.  (Under these costs a start that
    # uses a residue of the target differs from -cost(qe + 1) by 2 at least, so the empty interval's TRUE ties are the random groups' under
    # free gaps and matrices with a 0.)
    out.append((W(0, 0), W(1, 1), 0, (-8, 0, 1, 1, 0)))
    # ... with the end free one mismatch in the last row is better: cell (1, 0) = -4, the interval target[1..1]
    out.append((W(0, 0), W(1, 1), 2, (-4, 0, 0, 1, 1)))
    # the empty query interval loses where the real cell is better: one residue each, start free, a mismatch (-4) against deleting the
    # target's residue (-6)
    out.append((W(0), W(1), 1, (-4, 0, 0, 0, 0)))
    qs, ts, es, exp = [c[0] for c in out], [c[1] for c in out], [c[2] for c in out], [c[3] for c in out]
    return qs, ts, es, exp


def dear_mismatch_mat(m=5, match=2, mismatch=9):
    """a match / mismatch matrix whose mismatch is dearer than one deletion under costs (4, 2): with the query's start free and a target of
    one residue that the query's last residue does not match, the empty query interval (qb = qe + 1, CIGAR 1 D, score -6) is the optimum"""
    mat = np.full((m, m), -mismatch, np.int8)
    np.fill_diagonal(mat, match)
    return mat.reshape(-1)


def write_input(path, q, t, mat, m, costs, ends, flag):
    """the input file of tests/dropin/ova_caller.c"""
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d\n%s\n%d\n" % ((m,) + four(costs) + (ends, flag, " ".join(str(int(x)) for x in mat), len(q))))
        for x, y in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(x), " ".join(map(str, x.tolist())), len(y), " ".join(map(str, y.tolist()))))


# ---- the golden file (tests/gen_ova_golden.py writes it from the compiled reference; data only)
def save_golden(path, cases):
    """cases: per group of tests/sg_util.golden_inputs() a dict (kind, ends) -> (qb (n,), tb (n,), {flag: [cigar lists]}), kind "ov" / "ovd";
    the inputs stay in sg_cases.npz, (score, qe, te) in ov_cases.npz"""
    out = dict(ngroups=np.int32(len(cases)))
    for k, c in enumerate(cases):
        for (kind, e), (qb, tb, cig) in c.items():
            p = "g%d_%s%d_" % (k, kind, e)
            out[p + "qb"] = np.asarray(qb, dtype=np.int32)
            out[p + "tb"] = np.asarray(tb, dtype=np.int32)
            for fl in GOLDEN_FLAGS:
                out[p + "ncig%d" % fl] = np.array([len(x) for x in cig[fl]], dtype=np.int32)
                out[p + "cig%d" % fl] = np.array([y for x in cig[fl] for y in x], dtype=np.uint32)
    np.savez_compressed(path, **out)


_golden = None


def load_golden():
    """[(name, m, mat, costs, costs4, queries, targets, {(kind, ends): (cells (n, 5) score qb qe tb te, {flag: [cigar lists]})})].  Loaded
    once; treat it as read-only."""
    global _golden
    if _golden is None:
        z = np.load(GOLDEN)
        out = []
        for k, (name, m, mat, c2, c4, qs, ts, e1, e2) in enumerate(ov.load_golden()):
            n = len(qs)
            per = {}
            for kind, exp in (("ov", e1), ("ovd", e2)):
                for e in ENDS:
                    p = "g%d_%s%d_" % (k, kind, e)
                    cells = np.zeros((n, 5), np.int32)
                    cells[:, 0], cells[:, 2], cells[:, 4] = exp[e][:, 0], exp[e][:, 1], exp[e][:, 2]
                    cells[:, 1], cells[:, 3] = z[p + "qb"], z[p + "tb"]
                    cig = {}
                    for fl in GOLDEN_FLAGS:
                        offs = np.concatenate([[0], np.cumsum(z[p + "ncig%d" % fl])])
                        flat = z[p + "cig%d" % fl]
                        cig[fl] = [[int(x) for x in flat[offs[i]:offs[i + 1]]] for i in range(n)]
                    per[(kind, e)] = (cells, cig)
            out.append((name, m, mat, c2, c4, qs, ts, per))
        assert len(out) == int(z["ngroups"])
        _golden = out
    return _golden
