#!/usr/bin/env python3
"""Writes tests/golden/sgd_cases.npz: for the 324 pairs of tests/sg_util.golden_inputs() (their inputs stay in tests/golden/sg_cases.npz),
each group under the two-piece cost tests/sgd_util.GOLDEN_COSTS gives it, what the compiled reference (oracle/_ref/libksw2ref.so, built by
build() where the reference's sources exist) gives through its scalar ksw_extd.  The reference has no semi-global entry; per pair, with
cost(l) = min(gapo + l * gape, gapo2 + l * gape2):

    r(te)  = ksw_extd(reverse(query), reverse(target[0..te]), w = -1, zdrop = -1, SCORE_ONLY)       for every te
    v(te)  = max(r(te).mqe, -cost(qlen));   score = the largest v(te), te = the smallest te that reaches it, qe = qlen - 1
    tb     = te - r(te).mqe_t  when r(te).mqe > -cost(qlen),  te + 1 otherwise (the empty interval)
    cigar  = ksw_extd(query, target[tb..te], w = -1, zdrop = -1, GENERIC_SC | flag).cigar for flag in 0, RIGHT, REV_CIGAR;
             the empty interval: qlen I

and on EVERY pair it asserts max(r.mqe, -cost(qlen)) == score and, for a non-empty interval, ez.score == score.  No pair is set aside.
Data only.

usage: python tests/gen_sgd_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle as po     # noqa: E402
from tests import lla_util as la      # noqa: E402
from tests import sg_util as s        # noqa: E402
from tests import sgd_util as d       # noqa: E402


def ref_pair(q, t, mat, costs, m):
    go, ge, go2, ge2 = costs
    allins = -d.gap_cost(costs, len(q))
    rq = np.ascontiguousarray(q[::-1])
    best, bte, br = None, -1, None
    for te in range(len(t)):
        r = po.align("ref", "extd", rq, np.ascontiguousarray(t[te::-1]), mat, go, ge, go2, ge2, w=-1, zdrop=-1, flag=po.SCORE_ONLY, m=m)
        v = max(int(r["mqe"]), allins)
        if best is None or v > best:
            best, bte, br = v, te, r
    assert max(int(br["mqe"]), allins) == best
    tb = bte - int(br["mqe_t"]) if int(br["mqe"]) > allins else bte + 1
    cig = {}
    for fl in d.FLAGS:
        if tb <= bte:
            gs, cig[fl] = d.global_extd(q, t[tb:bte + 1], mat, m, costs, fl, "ref")
            assert gs == best, (best, tb, bte, gs, fl)
        else:
            cig[fl] = [len(q) << 4 | 1]
    return (best, 0, len(q) - 1, tb, bte), cig


def main():
    if not la.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else d.GOLDEN
    cases, total, empty, negative = [], 0, 0, 0
    groups = s.golden_inputs()
    assert len(groups) == len(d.GOLDEN_COSTS)
    for (name, m, mat, gapo, gape, qs, ts), costs in zip(groups, d.GOLDEN_COSTS):
        cells, cigs = [], {fl: [] for fl in d.FLAGS}
        for q, t in zip(qs, ts):
            c, cig = ref_pair(q, t, mat, costs, m)
            cells.append(c)
            for fl in d.FLAGS:
                cigs[fl].append(cig[fl])
            empty += c[3] > c[4]
            negative += c[0] < 0 and c[3] <= c[4]
        cases.append((name, costs, cells, cigs))
        total += len(qs)
    d.save_golden(out, cases)
    print(out, os.path.getsize(out), "bytes,", total, "pairs,", empty, "empty intervals,", negative, "negative optima with an interval")


if __name__ == "__main__":
    main()
