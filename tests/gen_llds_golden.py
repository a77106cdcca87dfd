#!/usr/bin/env python3
"""Writes tests/golden/llds_cases.npz: the inputs of tests/llds_util.golden_inputs() and, for every pair, the expected (score, qe, te,
score2, qe2, te2) of ksw2amd_lld_sub_batch from the scalar oracle tests/llds_oracle.c.  Data only.

usage: python tests/gen_llds_golden.py [out.npz]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import llds_util as x      # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else x.GOLDEN
    sets = [(q, t, mat, m, costs, excl, x.oracle_batch(q, t, mat, costs, excl, m)) for q, t, mat, m, costs, excl in x.golden_inputs()]
    x.save_golden(out, sets)
    print(out, os.path.getsize(out), "bytes,", sum(len(c[0]) for c in sets), "pairs")


if __name__ == "__main__":
    main()
