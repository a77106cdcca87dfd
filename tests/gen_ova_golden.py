#!/usr/bin/env python3
"""Writes tests/golden/ova_cases.npz: for the 324 pairs of tests/sg_util.golden_inputs() (their inputs stay in tests/golden/sg_cases.npz; the
(score, qe, te) of the overlap entries are tests/golden/ov_cases.npz and are this generator's input), under each group's single-piece costs
and under the two-piece costs tests/sgd_util.GOLDEN_COSTS pairs it with, for ends 1, 2, 3: the start cell (qb, tb) and the CIGARs for flag 0
and KSW_EZ_RIGHT of ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch, every value from the compiled reference (oracle/_ref/libksw2ref.so,
built by build() where the reference's sources exist).

The start is found by the definition.  The candidate start cells are taken in the contract's order -- (tb, 0) for tb = te + 1 down to 1, with
the query's start free (0, qb) for qb = qe + 1 down to 1, then (0, 0) -- and each one's G is the score of the reference's global ksw_extz
(ksw_extd) call on query[qb..qe] x target[tb..te] (w = -1, zdrop = -1), -cost of the other interval where one is empty; the first candidate
with G == score is the start, and no candidate may exceed the score.  The CIGAR is that call's on the chosen intervals; (qe + 1) I or
(te + 1) D for an empty one.

On EVERY pair and every ends in 0..3 the start is asserted equal to the contract's scalar statement (tests/ova_oracle.c), and for ends == 0
the start and the CIGARs equal to tests/golden/sga_cases.npz / sgd_cases.npz.  No pair is set aside.  Data only.

usage: python tests/gen_ova_golden.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import lla_util as la      # noqa: E402
from tests import ov_util as o        # noqa: E402
from tests import ova_util as a       # noqa: E402
from tests import sga_util as sa      # noqa: E402
from tests import sgd_util as d       # noqa: E402


def ref_start(q, t, mat, costs, m, ends, sc, qe, te, memo):
    """(qb, tb) by the definition; memo: G by (tb, qb, qe, te), shared between the values of ends"""
    best = None
    for tb, qb in a.candidates(qe, te, ends):
        key = (tb, qb, qe, te)
        if key not in memo:
            if tb > te:
                memo[key] = -o.gap_cost(costs, qe - qb + 1)
            elif qb > qe:
                memo[key] = -o.gap_cost(costs, te - tb + 1)
            else:
                memo[key] = a.global_ext(q[qb:qe + 1], t[tb:te + 1], mat, m, costs, 0, "ref")[0]
        assert memo[key] <= sc, (key, memo[key], sc)
        if memo[key] == sc:
            return qb, tb                        # (the candidates behind it lose the tie whatever they score: tests/ova_util.brute looks at all)
    raise AssertionError((ends, sc, qe, te))


def ref_cigar(q, t, mat, costs, m, flag, sc, qb, qe, tb, te):
    if tb > te:
        return [(qe + 1) << 4 | 1]
    if qb > qe:
        return [(te + 1) << 4 | 2]
    g, cig = a.global_ext(q[qb:qe + 1], t[tb:te + 1], mat, m, costs, flag, "ref")
    assert g == sc, (g, sc)
    return cig


def main():
    if not la.have_ref():
        sys.exit("oracle/_ref/libksw2ref.so is not built")
    out = sys.argv[1] if len(sys.argv) > 1 else a.GOLDEN
    sga, sgd = sa.load_golden(), d.load_golden()
    cases, total, stats = [], 0, dict(row0=0, empty_t=0, empty_q=0, inside=0)
    for k, (name, m, mat, c2, c4, qs, ts, e1, e2) in enumerate(o.load_golden()):
        per = {}
        for kind, costs, exp, ref0 in (("ov", c2, e1, (sga[k][7], sga[k][8])), ("ovd", c4, e2, (sgd[k][6], sgd[k][7]))):
            memos = [dict() for _ in qs]
            for e in range(4):
                fwd = exp[e] if e else ref0[0][:, [0, 2, 4]]
                want = a.oracle_cells(qs, ts, mat, costs, e, m)
                assert (want[:, [0, 2, 4]] == fwd).all(), (name, kind, e)
                st = np.array([ref_start(q, t, mat, costs, m, e, int(f[0]), int(f[1]), int(f[2]), mm) for q, t, f, mm in zip(qs, ts, fwd, memos)], dtype=np.int32)
                bad = np.nonzero((st != want[:, [1, 3]]).any(1))[0]
                assert len(bad) == 0, (name, kind, e, bad[:8], st[bad[:8]], want[bad[:8]])                 # the identity, on every pair
                cig = {fl: [ref_cigar(q, t, mat, costs, m, fl, *map(int, w)) for q, t, w in zip(qs, ts, want)] for fl in a.GOLDEN_FLAGS}
                if e == 0:
                    assert (want == ref0[0]).all(), (name, kind)
                    assert all(cig[fl] == ref0[1][fl] for fl in a.GOLDEN_FLAGS), (name, kind)
                    continue
                per[(kind, e)] = (st[:, 0], st[:, 1], cig)
                stats["row0"] += int((st[:, 0] > 0).sum())
                stats["empty_t"] += int((st[:, 1] > want[:, 4]).sum())
                stats["empty_q"] += int((st[:, 0] > want[:, 2]).sum())
                stats["inside"] += int(((st[:, 1] > 0) & (st[:, 1] <= want[:, 4])).sum())
                total += len(qs)
        cases.append(per)
    a.save_golden(out, cases)
    print(out, os.path.getsize(out), "bytes,", total, "pair x cost set x ends,", stats)


if __name__ == "__main__":
    main()
