"""Deterministic edge cases of the local-alignment kernels (ksw2_lane_ll.h, k2a_ll_task), shared by tests/test_local_edges_cpu.py (the
lock-step simulator) and tests/test_gpu_local_edges.py (the device).  No randomness beyond seeded default_rng.

A case is a dict: name, q, t, mat, m, go, ge and, for a planted case, planted = (qb, qe, tb, te).  Cases that share a matrix and gap
costs form a set (one batch call); sets() returns them all.

Planted pairs: the query's background is code 0 and the target's is code 1, every off-diagonal entry of the matrix is negative and no
core code occurs in a background, so every cell outside the core scores 0 and the optimum is the core's diagonal -- with at most one
indel whose extra residues are background -- from a chosen start cell to a chosen end cell.  plant() builds them in row / column
coordinates of the schedule (rows = the longer sequence: 16 rows per lane, 1 024 per generation) for either orientation, and
verify_planted() asserts that the scalar oracle returns exactly the planted cells: a check of the input, not of the product."""
import functools

import numpy as np

from tests import ll_util as u
from tests import lla_util as la

SEAM_ROWS = (15, 16, 1023, 1024, 1025, 2048)
GRID_ROWS = (1, 15, 16, 17, 1023, 1024, 1025, 2049)
GRID_COLS = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65)
_DIAG = (5, 4, 6, 3, 7, 5)
SET_NAMES = ("planted-m5", "planted-m6", "planted-m3", "planted-m4", "grid-m5", "grid-m5-linear", "grid-m3", "grid-m4", "grid-m6",
             "grid-m1-s3", "grid-m1-s-2", "grid-m127")


def asym_mat(m, mixed=False):
    """m x m, a distinct value in every off-diagonal entry, so s(a, b) != s(b, a) for every a != b and the row of a code differs from
    its column.  mixed = False: every off-diagonal entry negative (-3, -4, ...: the planted pairs); True: consecutive values that end
    at 7 or below (from -12 at m <= 5, from -22 at m = 6), a few of them positive and all below the diagonal's 11..15 (the mutated
    copies of the shape grid)."""
    a = np.zeros((m, m), dtype=np.int64)
    k, lo = 0, min(-12, 8 - m * (m - 1))
    for s in range(1, m):                      # by cyclic distance: (i, j) and (j, i) never neighbours in value
        for i in range(m):
            a[i, (i + s) % m] = (lo + k) if mixed else -(3 + k)
            k += 1
    for i in range(m):
        a[i, i] = _DIAG[i % len(_DIAG)] + (8 if mixed else 0)
    off = a[~np.eye(m, dtype=bool)]
    assert len(set(off.tolist())) == m * (m - 1) and off.max() < a.diagonal().min() and -128 <= off.min()
    return a.astype(np.int8).reshape(-1)


def plant(name, mat, m, go, ge, sw, rows, cols, r0, c0, core, gap=None):
    """One planted case.  rows > cols are the sequences' lengths; sw: rows = the query (else the target).  The core starts in cell
    (r0, c0); gap = (kind, o, g): 'v': g extra residues in the row sequence after core[:o] (a gap that runs down the rows), 'h': in
    the column sequence."""
    assert rows > cols
    core = np.asarray(core, dtype=np.uint8)
    rbg, cbg = (0, 1) if sw else (1, 0)          # the query's background is 0, the target's 1
    assert not np.isin(core, (0, 1)).any()
    rc = cc = core
    if gap is not None:
        kind, o, g = gap
        assert 0 < o < len(core) and g > 0
        if kind == "v":
            rc = np.concatenate([core[:o], np.full(g, rbg, np.uint8), core[o:]])
        else:
            cc = np.concatenate([core[:o], np.full(g, cbg, np.uint8), core[o:]])
    r1, c1 = r0 + len(rc) - 1, c0 + len(cc) - 1
    assert 0 <= r0 and r1 < rows and 0 <= c0 and c1 < cols, (name, r0, r1, rows, c0, c1, cols)
    rs, cs = np.full(rows, rbg, np.uint8), np.full(cols, cbg, np.uint8)
    rs[r0:r1 + 1] = rc
    cs[c0:c1 + 1] = cc
    q, t = (rs, cs) if sw else (cs, rs)
    planted = (r0, r1, c0, c1) if sw else (c0, c1, r0, r1)
    return dict(name="%s/sw%d" % (name, sw), q=q, t=t, mat=mat, m=m, go=go, ge=ge, planted=planted, rows_end=r1, rows_start=r0)


def _zero(name, mat, m, go, ge, sw, rows, cols):
    """a pair of backgrounds only: score 0"""
    q, t = np.zeros(rows if sw else cols, np.uint8), np.ones(cols if sw else rows, np.uint8)
    return dict(name="%s/sw%d" % (name, sw), q=q, t=t, mat=mat, m=m, go=go, ge=ge, planted=(-1, -1, -1, -1))


def planted_cases(m, go=6, ge=2, full=True):
    """The planted grid for one alphabet size (m >= 3; cores from codes 2..m-1, code 4 among them at m >= 5).  Cases come in twos of
    one shape that no other two share, so that form 1 packs exactly them into one task -- always two different end cells -- but
    for the one three-generation case of each orientation.  full = False: the seams 16 and 1024, the generation seam's gaps, the
    last cell, column 0 and the mixed REV tasks only."""
    mat = asym_mat(m)
    rng = np.random.default_rng(1000 + m)
    out = []
    shape = [0]

    def core(n):
        return rng.integers(2, m, n, dtype=np.uint8)

    def two(rows, cols, a, b):
        """a, b: functions (rows, cols, sw) -> case; both orientations, every two in a shape of their own"""
        for sw in (0, 1):
            c = cols + shape[0]
            shape[0] += 1
            out.append(a(rows, c, sw))
            out.append(b(rows, c, sw))

    def end_at(tag, r1, c1, n):
        return lambda rows, cols, sw: plant(tag, mat, m, go, ge, sw, rows, cols, r1 - n + 1, c1 - n + 1, core(n))

    def lone(rows, cols, a):
        """one case in a shape of its own (form 1 leaves it to the int32 kernel, form 2 packs it alone); both orientations"""
        for sw in (0, 1):
            out.append(a(rows, cols + shape[0], sw))
            shape[0] += 1

    seams = SEAM_ROWS if full else (16, 1024)
    # the end cell on a seam row; its partner ends inside a lane's strip of another generation.  No more rows than the two need.
    for k, r in enumerate(seams):
        pr = r + 1040 if r < 1000 else r - 700
        two(max(r, pr) + 30, 80, end_at("end-row%d" % r, r, 36 + k, min(30, r + 1)), end_at("end-row%d-partner" % r, pr, 70, 30))
    # the start cell on a seam row of the REV pass: the alignment spans r + 1 rows, so the pair has more than r + 1 columns too.
    # 15 with 16 and 1023 with 1024 share a shape; 1025 has a short partner
    rev = lambda r: (lambda R, C, sw: plant("rev-row%d" % r, mat, m, go, ge, sw, R, C, 7, 3, core(r + 1)))
    short = lambda r: (lambda R, C, sw: plant("rev-row%d-partner" % r, mat, m, go, ge, sw, R, C, R - 25, C - 22, core(20)))
    if full:
        two(60, 30, rev(15), rev(16))
        two(1024 + 50, 1024 + 12, rev(1023), rev(1024))
        two(1025 + 50, 1025 + 12, rev(1025), short(1025))
    else:
        two(60, 30, rev(16), short(16))
    # the last row and the last column; column 0 as the end cell (one matching residue) and as the start cell
    two(1040, 70, lambda R, C, sw: plant("last-cell", mat, m, go, ge, sw, R, C, R - 50, C - 50, core(50)),
        lambda R, C, sw: plant("end-col0", mat, m, go, ge, sw, R, C, 1024, 0, core(1)))
    if full:
        two(1040, 80, lambda R, C, sw: plant("start-col0", mat, m, go, ge, sw, R, C, 1000, 0, core(40)),
            lambda R, C, sw: plant("end-col0-row0", mat, m, go, ge, sw, R, C, 0, 0, core(1)))
    # one indel open across a strip seam (15 -> 16) and across the generation seam (1023 -> 1024): the vertical gap's rows are
    # seam - 1, seam, seam + 1; the horizontal gap lies in row seam, the diagonal goes on in row seam + 1
    for seam in ((15, 1023) if full else (1023,)):
        o = min(40, seam - 2)
        two(seam + 160, 100, lambda R, C, sw, o=o, s=seam: plant("vgap-row%d" % s, mat, m, go, ge, sw, R, C, s - 1 - o, 5, core(o + 40), ("v", o, 3)),
            lambda R, C, sw, o=o, s=seam: plant("hgap-row%d" % s, mat, m, go, ge, sw, R, C, s + 1 - o, 9, core(o + 40), ("h", o, 3)))
    # a core over three generations whose start cell lies on row 2048 of the REV pass: 2 049 rows and columns, so one case per
    # orientation, in a shape of its own
    if full:
        lone(2049 + 40, 2049 + 12, lambda R, C, sw: plant("three-gen-rev-row2048", mat, m, go, ge, sw, R, C, 7, 3, core(2049)))
    # mixed packed tasks of the REV pass: one half scores 0; end cells in different generations; identical end cells
    two(1500, 100, lambda R, C, sw: _zero("mixed-zero", mat, m, go, ge, sw, R, C),
        lambda R, C, sw: plant("mixed-zero-partner", mat, m, go, ge, sw, R, C, 1100, 20, core(60)))
    two(1500, 110, lambda R, C, sw: plant("mixed-zero-partner-first", mat, m, go, ge, sw, R, C, 1001, 20, core(60)),
        lambda R, C, sw: _zero("mixed-zero-second", mat, m, go, ge, sw, R, C))
    two(2300, 120, lambda R, C, sw: plant("mixed-gen0", mat, m, go, ge, sw, R, C, 400, 10, core(70)),
        lambda R, C, sw: plant("mixed-gen2", mat, m, go, ge, sw, R, C, 2100, 40, core(50)))
    two(1500, 130, lambda R, C, sw: plant("mixed-same-end-long", mat, m, go, ge, sw, R, C, 1030 - 90, 100 - 90, core(91)),
        lambda R, C, sw: plant("mixed-same-end-short", mat, m, go, ge, sw, R, C, 1030 - 10, 100 - 10, core(11)))
    return out


def _window(rows, cols, k):
    """start of the row window that the column sequence copies: over the last seam below `rows` (first copy), elsewhere (second)"""
    seam = max([s for s in (16, 1024, 2048) if s < rows] or [0])
    pos = seam - cols // 2 if k == 0 else (rows - cols) // 3
    return min(max(pos, 0), rows - cols)


def grid_cases(m, mat, go, ge, rows_set=GRID_ROWS, cols_set=GRID_COLS, both=((17, 9), (1025, 65), (2049, 4))):
    """The unplanted shape grid: the column sequence is a mutated copy of a window of the row sequence.  Every shape twice (form 1 packs
    the two), orientations alternating from shape to shape; the shapes in `both` in either orientation."""
    rng = np.random.default_rng(2000 + m)
    out, k = [], 0
    for rows in rows_set:
        for cols in cols_set:
            if cols > rows:
                continue
            for sw in ((0, 1) if (rows, cols) in both else (k % 2,)):
                for copy in (0, 1):
                    rs = rng.integers(0, m, rows, dtype=np.uint8)
                    w = _window(rows, cols, copy)
                    cs = u.mutate(rng, rs[w:w + cols], m, 0.06, 0.04)[:cols]
                    cs = np.concatenate([cs, rng.integers(0, m, cols - len(cs), dtype=np.uint8)])
                    if rows == cols:
                        sw = 0                     # equal lengths: rows = the target
                    q, t = (rs, cs) if sw else (cs, rs)
                    out.append(dict(name="grid-%dx%d/sw%d/%d" % (rows, cols, sw, copy), q=q, t=t, mat=mat, m=m, go=go, ge=ge))
            k += 1
    return out


def verify_planted(cases):
    """the scalar oracle (forward, then on the reversed prefixes) returns exactly the planted cells of every planted case"""
    pl = [c for c in cases if "planted" in c]
    if not pl:
        return
    c0 = pl[0]
    cells = la.start_cells([c["q"] for c in pl], [c["t"] for c in pl], c0["mat"], c0["go"], c0["ge"], c0["m"])
    for c, (s, qb, qe, tb, te, s2) in zip(pl, cells.tolist()):
        assert (qb, qe, tb, te) == tuple(c["planted"]), (c["name"], (s, qb, qe, tb, te), c["planted"])
        assert s == s2 and (s > 0) == (qe >= 0), (c["name"], s, s2)


@functools.lru_cache(maxsize=None)
def sets():
    """Every set of the edge grid: list of dicts name, mat, m, go, ge, cases."""
    out = []

    def add(name, m, mat, go, ge, cases):
        mat = cases[0]["mat"]
        assert all(c["m"] == m and c["go"] == go and c["ge"] == ge and c["mat"] is mat for c in cases)
        verify_planted(cases)
        out.append(dict(name=name, m=m, mat=mat, go=go, ge=ge, cases=cases))

    small = dict(rows_set=(1, 17, 1025), cols_set=(1, 4, 9, 65), both=((17, 9),))
    for m in (5, 6, 3, 4):                                       # the whole planted grid at m = 5, its short form elsewhere
        add("planted-m%d" % m, m, asym_mat(m), 6, 2, planted_cases(m, full=(m == 5)))
    mat = asym_mat(5, mixed=True)
    add("grid-m5", 5, mat, 4, 2, grid_cases(5, mat, 4, 2))
    mat = asym_mat(5)
    add("grid-m5-linear", 5, mat, 0, 1, grid_cases(5, mat, 0, 1, **small))
    for m in (3, 4, 6):
        mat = asym_mat(m, mixed=True)
        add("grid-m%d" % m, m, mat, 4, 2, grid_cases(m, mat, 4, 2, **small))
    for s in (3, -2):                                            # m = 1: the matrix is [s]; a negative one scores nothing
        mat = np.array([s], dtype=np.int8)
        add("grid-m1-s%d" % s, 1, mat, 2, 1, grid_cases(1, mat, 2, 1, **small))
    rng = np.random.default_rng(127)
    mat = rng.integers(-128, 128, 127 * 127).astype(np.int8)
    mat[:2] = (127, -128)                                        # both ends of the range are in: pen = 0 and 255, oe = 254
    add("grid-m127", 127, mat, 127, 127, grid_cases(127, mat, 127, 127, **small))
    return out


def saturation_cases():
    """(name, mat, n, admitted): two identical pairs of length n over four letters.  smax = 85: (770 + 1) * 85 = 65 535, the packed
    format's last admissible pair (H + smax = 65 535 exactly); 771 is refused.  smax = 127 with mismatch -128 (pen = 255): 515 / 516."""
    return [("smax85", u.simple_mat(4, 85, 3), 770, True), ("smax85", u.simple_mat(4, 85, 3), 771, False),
            ("smax127", u.simple_mat(4, 127, 128), 515, True), ("smax127", u.simple_mat(4, 127, 128), 516, False)]


def saturation_pair(n):
    x = np.random.default_rng(n).integers(0, 4, n, dtype=np.uint8)
    return [x, x.copy()], [x.copy(), x.copy()]


def seqs(s):
    return [c["q"] for c in s["cases"]], [c["t"] for c in s["cases"]]


def twins(s):
    """how many twos of one (query length, target length) a set holds: at least so many packed tasks under forms 1 and 2"""
    shapes = [(len(c["q"]), len(c["t"])) for c in s["cases"]]
    return sum(shapes.count(x) // 2 for x in set(shapes))


def planted_dicts(s):
    """{index in the set: (score > 0, qb, qe, tb, te)} of the set's planted cases"""
    return {i: tuple(c["planted"]) for i, c in enumerate(s["cases"]) if "planted" in c}
