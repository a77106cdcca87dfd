#!/usr/bin/env python3
"""Writes tests/golden/lld_cases.npz: the inputs of tests/lld_util.golden_inputs() and, for every pair, the expected
(score, qb, qe, tb, te, CIGAR) of ksw2amd_lld_align_batch -- cells from tests/lld_oracle.c (forward and on the reversed prefixes), the
CIGAR from the compiled reference's scalar ksw_extd on the interval (oracle/_ref/libksw2ref.so, built by build() where the reference's
sources exist).  Data only.

usage: python tests/gen_lld_golden.py [out.npz]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import lla_util as la      # noqa: E402
from tests import lld_util as d       # noqa: E402


def main():
    if not la.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else d.GOLDEN
    cases = []
    for name, m, mat, costs, q, t in d.golden_inputs():
        exp = d.expected(q, t, mat, costs, m, which="ref")
        assert all(e["gscore"] == e["score"] and e["rscore"] == e["score"] for e in exp), name
        cases.append((name, m, mat, costs, q, t, exp))
    d.save_golden(out, cases)
    print(out, os.path.getsize(out), "bytes,", sum(len(c[4]) for c in cases), "pairs")


if __name__ == "__main__":
    main()
