#!/usr/bin/env python3
"""Writes tests/golden/sga_cases.npz: for the 324 pairs of tests/sg_util.golden_inputs() (their inputs, scores and te stay in
tests/golden/sg_cases.npz), what the compiled reference (oracle/_ref/libksw2ref.so, built by build() where the reference's sources exist)
gives for the start of the interval and for the CIGAR.  Per pair, with (score, te) of sg_cases.npz:

    r  = ksw_extz(reverse(query), reverse(target[0..te]), w = -1, zdrop = -1, SCORE_ONLY)
    tb = te - r.mqe_t  when r.mqe > -(gapo + qlen * gape),  te + 1 otherwise (the empty interval)
    cigar = ksw_extz(query, target[tb..te], w = -1, zdrop = -1, GENERIC_SC | flag).cigar for flag in 0, RIGHT, REV_CIGAR;
            the empty interval: qlen I

and on EVERY pair it asserts max(r.mqe, -(gapo + qlen * gape)) == score and, for a non-empty interval, ez.score == score.  Data only.

usage: python tests/gen_sga_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle as po     # noqa: E402
from tests import lla_util as la      # noqa: E402
from tests import sg_util as s        # noqa: E402
from tests import sga_util as a       # noqa: E402


def ref_pair(q, t, mat, gapo, gape, m, score, te):
    allins = -(gapo + len(q) * gape)
    r = po.align("ref", "extz", np.ascontiguousarray(q[::-1]), np.ascontiguousarray(t[te::-1]), mat, gapo, gape, w=-1, zdrop=-1, flag=po.SCORE_ONLY, m=m)
    assert max(int(r["mqe"]), allins) == score, (score, te, r)
    tb = te - int(r["mqe_t"]) if int(r["mqe"]) > allins else te + 1
    cig = {}
    for fl in a.FLAGS:
        if tb <= te:
            gs, cig[fl] = la.global_extz(q, t[tb:te + 1], mat, m, gapo, gape, fl, "ref")
            assert gs == score, (score, tb, te, gs, fl)
        else:
            cig[fl] = [len(q) << 4 | 1]
    return tb, cig


def main():
    if not la.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else a.GOLDEN
    cases, total, empty = [], 0, 0
    for (name, m, mat, gapo, gape, qs, ts), g in zip(s.golden_inputs(), s.load_golden()):
        assert name == g[0]
        tbs, cigs = [], {fl: [] for fl in a.FLAGS}
        for q, t, (score, qe, te) in zip(qs, ts, g[7]):
            tb, cig = ref_pair(q, t, mat, gapo, gape, m, int(score), int(te))
            tbs.append(tb)
            for fl in a.FLAGS:
                cigs[fl].append(cig[fl])
            empty += tb > te
        cases.append((name, tbs, cigs))
        total += len(qs)
    a.save_golden(out, cases)
    print(out, os.path.getsize(out), "bytes,", total, "pairs,", empty, "empty intervals")


if __name__ == "__main__":
    main()
