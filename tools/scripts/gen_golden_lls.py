#!/usr/bin/env python3
"""Writes tests/golden/lls_cases.npz: inputs, parameters and the six expected numbers of ksw2amd_ll_sub_batch (score, qe, te, score2,
qe2, te2) from the scalar oracle tests/lls_oracle.c, after that oracle's pin to the COMPILED REFERENCE's scalar ksw_extz has passed
(tests/test_local_sub_cpu.py::test_oracle_pinned_to_reference_extz).  Data only; fixed seed.

usage: python tools/scripts/gen_golden_lls.py        (needs oracle/_ref, which __graft_entry__.build() makes where the reference exists)
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import ll_util as u          # noqa: E402
from tests import lls_util as s         # noqa: E402


def main():
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libksw2ref.so")):
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    pin = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.join(ROOT, "tests", "test_local_sub_cpu.py"),
                          "-k", "pinned_to_reference or brute_force"], cwd=ROOT, capture_output=True, text=True)
    if pin.returncode != 0 or "skipped" in pin.stdout:
        sys.exit("the oracle's pin did not pass:\n" + pin.stdout[-2000:])
    rng = np.random.default_rng(20261017)
    m20 = u.random_mat(rng, 20)
    sets = []
    q, t = u.ragged(rng, 120, 5, 1, 400, related=0.6)
    sets.append((q, t, s.M5, 5, 4, 2, -1))
    q, t = u.ragged(rng, 80, 20, 1, 300, related=0.6)
    sets.append((q, t, m20, 20, 6, 1, -1))
    q, t = s.differing_halves(rng)
    sets.append((q, t, s.M5, 5, 0, 1, 10))
    q, t = s.generation_edges(rng)
    q2, t2 = s.tandem_repeats(rng)
    sets.append((q[:8] + q2, t[:8] + t2, s.M5, 5, 4, 2, -1))
    q, t = s.forced_orientation(rng)
    sets.append((q, t, s.M5, 5, 4, 2, 0))
    out = dict(nsets=np.int32(len(sets)))
    for k, (q, t, mat, m, go, ge, excl) in enumerate(sets):
        out["s%d_par" % k] = np.array([m, go, ge, excl], dtype=np.int32)
        out["s%d_mat" % k] = np.asarray(mat, dtype=np.int8)
        out["s%d_qlen" % k] = np.array([len(x) for x in q], dtype=np.int32)
        out["s%d_tlen" % k] = np.array([len(x) for x in t], dtype=np.int32)
        out["s%d_q" % k] = np.concatenate(q).astype(np.uint8)
        out["s%d_t" % k] = np.concatenate(t).astype(np.uint8)
        out["s%d_res" % k] = s.oracle_batch(q, t, mat, go, ge, excl, m)
    path = os.path.join(ROOT, "tests", "golden", "lls_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", sum(len(x[0]) for x in sets), "pairs")


if __name__ == "__main__":
    main()
