#!/usr/bin/env python3
"""Writes tests/golden/ov_cases.npz: for the 324 pairs of tests/sg_util.golden_inputs() (their inputs stay in tests/golden/sg_cases.npz), under
each group's own single-piece costs and under the two-piece costs tests/sgd_util.GOLDEN_COSTS pairs it with, the (score, qe, te) of the overlap
entries for ends 1, 2, 3 as the compiled reference gives them (oracle/_ref/libksw2ref.so, built by build() where the reference's sources
exist).  The reference has no overlap entry; its scalar ksw_extz / ksw_extd give one end cell at a time.  With cost(l) the entry's gap cost,
the value of a cell (te, qe) is

    r = ksw_extz(reverse(query[0..qe]), reverse(target[0..te]), w = -1, zdrop = -1, SCORE_ONLY)          (ksw_extd for the two pieces)
    v = max(r.mqe, -cost(qe + 1))                                    without the query's start free
    v = max(r.mqe, -cost(qe + 1), r.mte, -cost(te + 1))              with it

-- r.mqe covers the starts (x - 1, -1), r.mte the starts (-1, y - 1), the constants the two corner starts an extension cannot express -- and
the result is the best v over the candidate cells (the last column; with the query's end free the last row as well) under the tie rule:
largest v, smallest te, smallest qe.  The extension calls of a pair are shared between the values of ends.

On EVERY pair and every ends in 0..3 the result is asserted equal to the contract's scalar statement (tests/ov_oracle.c), and for ends == 0
equal to the numbers in sg_cases.npz / sgd_cases.npz.  No pair is set aside.  Data only: the expected arrays.

usage: python tests/gen_ov_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle as po     # noqa: E402
from tests import lla_util as la      # noqa: E402
from tests import ov_util as o        # noqa: E402
from tests import sg_util as s        # noqa: E402
from tests import sgd_util as d       # noqa: E402


def ref_pair(q, t, mat, costs, m):
    """{ends: (score, qe, te)} for ends 0..3 from tlen + qlen - 1 extension calls of the compiled reference"""
    nq, nt = len(q), len(t)

    def ext(te, qe):
        rq, rt = np.ascontiguousarray(q[qe::-1]), np.ascontiguousarray(t[te::-1])
        if len(costs) == 4:
            r = po.align("ref", "extd", rq, rt, mat, costs[0], costs[1], costs[2], costs[3], w=-1, zdrop=-1, flag=po.SCORE_ONLY, m=m)
        else:
            r = po.align("ref", "extz", rq, rt, mat, costs[0], costs[1], w=-1, zdrop=-1, flag=po.SCORE_ONLY, m=m)
        fixed = max(int(r["mqe"]), -o.gap_cost(costs, qe + 1))
        return fixed, max(fixed, int(r["mte"]), -o.gap_cost(costs, te + 1))      # (the start inserted, the start free)

    col = [ext(te, nq - 1) + (te, nq - 1) for te in range(nt)]
    row = [ext(nt - 1, qe) + (nt - 1, qe) for qe in range(nq - 1)]              # the corner is in col
    out = {}
    for ends in range(4):
        cands = col + (row if ends & o.QEND else [])
        out[ends] = o.pick([(c[1] if ends & o.QBEG else c[0], c[2], c[3]) for c in cands])
    return out


def main():
    if not la.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else o.GOLDEN
    groups, dgroups = s.load_golden(), d.load_golden()
    gen = s.golden_inputs()
    assert len(groups) == len(gen) == len(d.GOLDEN_COSTS)
    single, dual, total, stats = [], [], 0, dict(last_row=0, negative=0)
    for k, (name, m, mat, gapo, gape, qs, ts, exp0) in enumerate(groups):
        assert all((a == b).all() for a, b in zip(qs + ts, gen[k][5] + gen[k][6])), name      # the inputs are the generator's
        for costs, dest, ref0 in (((gapo, gape), single, exp0), (d.GOLDEN_COSTS[k], dual, dgroups[k][6][:, [0, 2, 4]])):
            res = [ref_pair(q, t, mat, costs, m) for q, t in zip(qs, ts)]
            per = {e: np.array([r[e] for r in res], dtype=np.int32) for e in range(4)}
            for e in range(4):                                                 # the identity, on every pair
                want = o.oracle_batch(qs, ts, mat, costs, e, m)
                bad = np.nonzero((per[e] != want).any(1))[0]
                assert len(bad) == 0, (name, costs, e, bad[:8], per[e][bad[:8]], want[bad[:8]])
            assert (per[0] == ref0).all(), (name, costs)
            stats["last_row"] += int(((per[3][:, 1] < np.array([len(q) - 1 for q in qs])) & (per[3][:, 0] > per[1][:, 0])).sum())
            stats["negative"] += int((per[3][:, 0] < 0).sum())
            dest.append(per)
            total += len(qs)
    o.save_golden(out, single, dual)
    print(out, os.path.getsize(out), "bytes,", total, "pair x cost sets,", stats)


if __name__ == "__main__":
    main()
