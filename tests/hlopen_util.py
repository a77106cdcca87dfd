"""Shared by tests/test_hlopen_cpu.py (simulator build) and tests/test_gpu_hlopen.py (the real kernels): scorings that sit on the
boundaries of the packed kernels' profile bytes -- a byte is q + e + s(t, q) - pk_base (K2aScoring.cp, ksw2_lane_pk.h "Open form") --
and the forms every one of them is run through.  Everything is compared with the oracle on every ksw_extz_t field and the CIGAR;
which kernel ran, and the constant its table is short of, are read from the plan's description; packed_pairs() must be every pair.

expected `base` per scoring (what plan.describe() reports as base=): 0 while every byte fits 0..255 as it is, else the signed constant
that brings them in.  They follow from the scoring alone:
  preset      2 / -4 / N -1, q 4, e 2      bytes 8, 2, 5                      0
  floor       mismatch -6                  the smallest byte is exactly 0     0
  below       mismatch -7                  -1 would not fit                  -1
  deep        1 / -36, q 18, e 1           -17 would not fit                -17
  top         match 100, q 100, e 55       the largest byte is exactly 255    0
  over        match 100, q 101, e 55       256 would not fit                 +1
  m4          4 x 4, 2 / -7, q 4, e 2      no wildcard row: no pk_tn1        -1
"""
import numpy as np

from ksw2_amd import synth
from oracle import pyoracle as po
from tests import edge_util as eu
from tests import parity_util as pu


def _m4(a, b):
    mat = np.full((4, 4), -abs(b), dtype=np.int8)
    np.fill_diagonal(mat, a)
    return mat.reshape(-1).copy()


# name -> (matrix, m, q, e, q2, e2, extra flag, expected base, target wildcards are rows (pk_tn1), wildcard runs go into the targets)
SCORINGS = {
    "preset": (synth.simple_mat(5, 2, 4, -1), 5, 4, 2, 24, 1, 0, 0, 1, True),
    "floor": (synth.simple_mat(5, 2, 6, -1), 5, 4, 2, 24, 1, 0, 0, 1, True),
    "below": (synth.simple_mat(5, 2, 7, -1), 5, 4, 2, 24, 1, 0, -1, 1, True),
    "deep": (synth.simple_mat(5, 1, 36, -1), 5, 18, 1, 40, 1, 0, -17, 1, False),
    "top": (synth.simple_mat(5, 100, 4, -1), 5, 100, 55, 127, 40, 0, 0, 1, False),
    "over": (synth.simple_mat(5, 100, 4, -1), 5, 101, 55, 127, 40, 0, 1, 1, False),
    "m4": (_m4(2, 7), 4, 4, 2, 24, 1, po.GENERIC_SC, -1, 0, False),
}
SHORT = ("top", "over")                 # gap costs this large fit the plain 16-bit window on short pairs only
# (-17 as "match 1 / mismatch -19, q 1, e 1" is no batch the library runs: a mismatch below -2 (q + e) is rejected outright, as the
#  reference's own entry points do; gap costs are int8_t, so 255 is reached with q + e = 155 and a match of 100)


def pairs(seed, n, ql, tl, m, wild_targets, zdrop):
    """n pairs of one shape: mutated copies with unrelated tails on half of them where a Z-drop is set; query wildcards for m = 5;
    runs of the target wildcard in every second target where asked for"""
    tails = zdrop >= 0
    qs, ts = synth.fixed_batch(seed, n, ql, tl, sub=0.05, ind=0.06, tail_random_frac=0.3 if tails else 0.0, tail_pairs=0.5 if tails else 0.0)
    qs = [np.array(x, dtype=np.uint8) for x in qs]
    ts = [np.array(x, dtype=np.uint8) for x in ts]
    if m == 5:
        for i in range(0, n, 3):
            qs[i][len(qs[i]) // 3] = 4
    if wild_targets:
        ts = pu.sprinkle_target_wildcards(np.random.Generator(np.random.PCG64(seed + 1)), ts, every=2, runs=(1, min(50, tl)))
    return qs, ts


def run_case(lib, setenv, delenv, scoring, env, dual, flag, qs, ts, w, zdrop, want):
    """One batch through `lib` under `env`: the plan's description satisfies want(d), reports the scoring's base and target-wildcard
    rule, every pair is packed, and every field and CIGAR equals the oracle's.  Returns the description."""
    mat, m, q, e, q2, e2, xflag, base, tn, _ = SCORINGS[scoring]
    if not dual:
        q2 = e2 = 0
    flag |= xflag
    eu.set_env(setenv, delenv, env)
    p = lib.make_batch(qs, ts, mat, q, e, q2, e2, w=w, zdrop=zdrop, flag=flag, m=m).plan(dual)
    d, npk = p.describe(), p.packed_pairs()
    p.close()
    assert npk == len(qs), (scoring, env, npk, len(qs), d)
    assert d and all(c["kernel"] in ("pk", "solo", "pkmp") and c["base"] == base and c["tn"] == tn for c in d), (scoring, env, d)
    assert want(d), (scoring, env, d)
    n, _ = pu.check_batch(lib, dual, qs, ts, mat, q, e, q2, e2, w=w, zdrop=zdrop, flag=flag, m=m)
    assert n == len(qs)
    return d
