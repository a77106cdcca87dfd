#!/usr/bin/env python3
"""Writes tests/golden/sg_cases.npz: the inputs of tests/sg_util.golden_inputs() and, for every pair, the (score, qe, te) that the compiled
reference gives (oracle/_ref/libksw2ref.so, built by build() where the reference's sources exist).  The reference has no semi-global
entry; its scalar ksw_extz gives one target end at a time: for every te,

    v(te) = max(ksw_extz(reverse(query), reverse(target[0..te]), w = -1, zdrop = -1, SCORE_ONLY).mqe, -(gapo + qlen * gape))

-- the best extension from the cell (te, qlen - 1) backwards that uses the whole query, or the whole query inserted -- and the pair's
expected result is the largest v(te) at the smallest te, qe = qlen - 1.  Data only.

usage: python tests/gen_sg_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle as po     # noqa: E402
from tests import lla_util as la      # noqa: E402
from tests import sg_util as s        # noqa: E402


def ref_pair(q, t, mat, gapo, gape, m):
    rq = np.ascontiguousarray(q[::-1])
    best, bte = None, -1
    for te in range(len(t)):
        r = po.align("ref", "extz", rq, np.ascontiguousarray(t[te::-1]), mat, gapo, gape, w=-1, zdrop=-1, flag=po.SCORE_ONLY, m=m)
        v = max(int(r["mqe"]), -(gapo + len(q) * gape))
        if best is None or v > best:
            best, bte = v, te
    return best, len(q) - 1, bte


def main():
    if not la.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else s.GOLDEN
    cases = []
    for name, m, mat, gapo, gape, qs, ts in s.golden_inputs():
        exp = np.array([ref_pair(q, t, mat, gapo, gape, m) for q, t in zip(qs, ts)], dtype=np.int32)
        cases.append((name, m, mat, gapo, gape, qs, ts, exp))
    s.save_golden(out, cases)
    print(out, os.path.getsize(out), "bytes,", sum(len(c[5]) for c in cases), "pairs")


if __name__ == "__main__":
    main()
