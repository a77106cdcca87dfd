"""Golden vectors at the Z-drop and score-window edges (tests/edge_util.py): inputs + every ksw_extz_t field + CIGAR of the
UNMODIFIED reference at the large scorings of the packed window checks, each case at its critical threshold Z* (the smallest
zdrop / xdrop >= 0 at which the reference does not drop, found by bisection against the reference itself) and at Z* - 1.

Functions: scalar ksw_extz / ksw_extd, ksw_extz2_sse / ksw_extd2_sse (their own anti-diagonal Z*), ksw_exts2_sse, ksw_extf2_sse.
Run in the build container only (needs oracle/_ref):   python oracle/gen_golden_edges.py   ->   tests/golden/edge_cases.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po                       # noqa: E402
from tests.edge_util import WINDOW_SCORINGS, critical_zdrop, zdrop_pairs     # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FIELDS = ["score", "max", "max_t", "max_q", "mqe", "mqe_t", "mte", "mte_q", "zdropped", "reach_end", "n_cigar"]   # = tests/golden_util.FIELDS
EXTS_SCORINGS = [(1, 2, 0, 2, 1, 32, 4), (2, 4, -1, 4, 2, 24, 5), (1, 3, 0, 2, 1, 20, 9)]      # a, b, sc_n, q, e, q2, noncan
KINDS = ["extz", "extd", "extz2_sse", "extd2_sse", "exts2", "extf2"]


def run_ref(kind, q, t, a, b, sc_n, gq, ge, gq2, ge2, w, z, flag):
    mat = po.simple_mat(5, a, b, sc_n)
    if kind in ("extz", "extd"):
        return po.align("ref", kind, q, t, mat, gq, ge, gq2, ge2, w=w, zdrop=z, flag=flag)
    if kind in ("extz2_sse", "extd2_sse"):
        return po.align("ref", kind, q, t, mat, gq, ge, gq2, ge2, w=w, zdrop=z, flag=flag)
    if kind == "exts2":
        return po.exts2("ref", q, t, mat, gq, ge, gq2, ge2, zdrop=z, flag=flag)          # (ge2: the non-canonical splice penalty)
    return po.extf2("ref", q, t, a, -b, ge, w, z)


def main(n_cases=360, seed=20261015):
    rng = np.random.Generator(np.random.PCG64(seed))
    seqs, seq_off, params, expect, cigs, cig_off = [], [0], [], [], [], [0]
    pq, pt = zdrop_pairs(seed, n_cases, 0.6)
    kept = 0
    for it in range(n_cases):
        kind = KINDS[it % len(KINDS)]
        a, b, gq, ge, gq2, ge2 = WINDOW_SCORINGS[(it // len(KINDS)) % len(WINDOW_SCORINGS)]
        sc_n = 0 if a == b == 0 else -1
        if kind in ("extd", "extd2_sse") and ge == ge2:
            continue                                    # (the reference divides by e - e2)
        q, t = pq[it], pt[it]
        if kind in ("exts2", "extf2"):
            q, t = np.minimum(q, 3), np.minimum(t, 3)
        if kind == "exts2":                             # its 8-bit differences hold at the splice scorings only (gen_golden_exts.py)
            a, b, sc_n, gq, ge, gq2, ge2 = EXTS_SCORINGS[it % len(EXTS_SCORINGS)]
        elif kind == "extf2":
            ge = max(ge, 1)
        w = int(rng.choice([-1, 8, 30, 100]))
        if kind in ("extz", "extd") and w >= 0:
            w = max(w, abs(len(q) - len(t)))            # (a band that misses the corner is outside the scalar contract: SURVEY F6)
        flag = 0
        if kind in ("extz2_sse", "extd2_sse"):
            flag = int(rng.choice([0, po.SCORE_ONLY, po.RIGHT, po.EXTZ_ONLY, po.GENERIC_SC]))
        elif kind in ("extz", "extd"):
            flag = int(rng.choice([0, po.RIGHT]))
        elif kind == "exts2":
            flag = int(rng.choice([0, po.SPLICE_FOR, po.SPLICE_REV | po.SCORE_ONLY, po.RIGHT]))
        zs = critical_zdrop(lambda z: run_ref(kind, q, t, a, b, sc_n, gq, ge, gq2, ge2, w, z, flag)["zdropped"] == 1)
        if not zs:
            continue
        for z in (zs, zs - 1):
            res = run_ref(kind, q, t, a, b, sc_n, gq, ge, gq2, ge2, w, z, flag)
            seqs += [q, t]
            seq_off += [seq_off[-1] + len(q), seq_off[-1] + len(q) + len(t)]
            params.append([KINDS.index(kind), a, b, sc_n, gq, ge, gq2, ge2, w, z, flag, zs])
            expect.append([res[f] for f in FIELDS])
            cigs += res["cigar"]
            cig_off.append(len(cigs))
        kept += 1
    out = os.path.join(GOLD, "edge_cases.npz")
    np.savez_compressed(out, seq=np.concatenate(seqs).astype(np.uint8), seq_off=np.array(seq_off, dtype=np.int64),
                        params=np.array(params, dtype=np.int32), expect=np.array(expect, dtype=np.int64),
                        cigar=np.array(cigs, dtype=np.uint32), cigar_off=np.array(cig_off, dtype=np.int64))
    ex = np.array(expect)
    print("wrote", kept, "cases at Z* and Z* - 1,", os.path.getsize(out) // 1024, "KiB; zdropped", int(ex[:, 8].sum()), "with CIGAR", int((ex[:, 10] > 0).sum()))


if __name__ == "__main__":
    main()
