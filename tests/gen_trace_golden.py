#!/usr/bin/env python3
"""Writes tests/golden/trace_cases.npz: the planted pairs of tests/trace_util.golden_inputs() and, for each, every field of the record
and the CIGAR that the compiled reference's scalar ksw_extz / ksw_extd give (oracle/_ref/libksw2ref.so, built by build() where the
reference's sources exist).  The subset is chosen by coverage (golden_inputs) and the coverage is asserted on the reference's own
records before the file is written.  This pins the tie-breaking on exactly the shapes the traceback grid depends on.  Data only.

usage: python tests/gen_trace_golden.py [out.npz]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import pyoracle as po     # noqa: E402
from tests import trace_util as tu    # noqa: E402


def main():
    if po.ref_lib() is None:
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else tu.GOLDEN
    cases = tu.golden_inputs()
    q, e, q2, e2 = tu.GAPS
    exp = [po.align("ref", "extd", c[2], c[3], tu.MAT, q, e, q2, e2, w=c[4], zdrop=c[5], flag=c[6]) if c[1] else
           po.align("ref", "extz", c[2], c[3], tu.MAT, q, e, w=c[4], zdrop=c[5], flag=c[6]) for c in cases]
    tu.golden_coverage(cases, exp)      # every event the reference can express, per form row and value of KSW_EZ_RIGHT
    tu.save_golden(out, cases, exp)
    print(out, os.path.getsize(out), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
