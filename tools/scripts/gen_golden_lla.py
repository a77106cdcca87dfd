#!/usr/bin/env python3
"""Writes tests/golden/lla_cases.npz: inputs, parameters and the expected results of ksw2amd_ll_align_batch (score, qb, qe, tb, te,
CIGAR) by the contract's formula -- tests/ll_oracle.c forward and on the reversed prefixes, then the COMPILED REFERENCE's scalar
ksw_extz (oracle/_ref/libksw2ref.so) on the interval.  Data only; fixed seed.

usage: python tools/scripts/gen_golden_lla.py        (needs oracle/_ref, which __graft_entry__.build() makes where the reference exists)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import ll_util as u          # noqa: E402
from tests import lla_util as a         # noqa: E402


def main():
    if not a.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    rng = np.random.default_rng(20261016)
    m5, m20 = u.simple_mat(5, 2, 4, -1), u.random_mat(rng, 20)
    sets = []
    q, t = u.ragged(rng, 150, 5, 1, 400, related=0.6)
    sets.append((q, t, m5, 5, 4, 2, 0))
    q, t = u.ragged(rng, 100, 20, 1, 300, related=0.6)
    sets.append((q, t, m20, 20, 6, 1, 0))
    q, t = u.ragged(rng, 100, 5, 1, 300, related=0.6)
    sets.append((q, t, m5, 5, 0, 1, a.RIGHT))
    q, t = a.new_ground(rng, 5, small=True)
    sets.append((q, t, m5, 5, 4, 2, a.REV_CIGAR))
    out = dict(nsets=np.int32(len(sets)))
    for k, (q, t, mat, m, go, ge, flag) in enumerate(sets):
        exp = a.expected(q, t, mat, go, ge, m, flag, which="ref")
        for e in exp:
            assert e["rscore"] == e["score"] and e["gscore"] == e["score"], e
        out["s%d_par" % k] = np.array([m, go, ge, flag], dtype=np.int32)
        out["s%d_mat" % k] = np.asarray(mat, dtype=np.int8)
        out["s%d_qlen" % k] = np.array([len(x) for x in q], dtype=np.int32)
        out["s%d_tlen" % k] = np.array([len(x) for x in t], dtype=np.int32)
        out["s%d_q" % k] = np.concatenate(q).astype(np.uint8)
        out["s%d_t" % k] = np.concatenate(t).astype(np.uint8)
        out["s%d_res" % k] = np.array([[e["score"], e["qb"], e["qe"], e["tb"], e["te"], e["n_cigar"]] for e in exp], dtype=np.int32)
        out["s%d_cig" % k] = np.array([c for e in exp for c in e["cigar"]], dtype=np.uint32)
    path = os.path.join(ROOT, "tests", "golden", "lla_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", sum(len(s[0]) for s in sets), "pairs")


if __name__ == "__main__":
    main()
