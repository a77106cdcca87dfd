"""CPU: semi-global alignment under the two-piece gap cost (ksw2amd_sgd_batch / ksw2amd_sgd_align_batch, their flat forms and the
single-pair entries; include/ksw2_amd.h).  The contract (tests/sgd_oracle.c) is pinned to the compiled reference's
scalar ksw_extd through tests/golden/sgd_cases.npz and to a brute-force statement in plain Python; the product's host code and lane code
(K2aLaneLL<.., DUAL = true, FIT = true>, with and without REV, both number formats and both score lookups) run on a test-local lock-step
simulator build against that oracle; a C caller compiled against include/ksw2_amd.h prints the contract's answers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import llf_util as lf
from tests import lla_util as la
from tests import sg_util as s
from tests import sga_util as a
from tests import sgd_util as d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2, 24, 1), (24, 1, 4, 2), (0, 1, 5, 0), (6, 3, 0, 0))
NAMES = ("ksw2amd_sgd_batch", "ksw2amd_sgd_batch_flat", "ksw2amd_sgd", "ksw2amd_sgd_align_batch", "ksw2amd_sgd_align_batch_flat", "ksw2amd_sgd_align")
RESET = dict(score=0, qb=-1, qe=-1, tb=-1, te=-1, n_cigar=0, cigar=[])
E_PARAM = -2


@pytest.fixture(scope="module")
def simso(tmp_path_factory):
    return d.sim_library(str(tmp_path_factory.mktemp("sgdsim") / "libksw2_amd.so"))


@pytest.fixture(scope="module")
def sim(simso):
    return ksw2_amd.Library(simso)


@pytest.fixture(autouse=True)
def _env():
    keys = ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS", "KSW2AMD_TRACE", "KSW2AMD_ABORT_ON_ERROR")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 3)
    return mat.reshape(-1)


def _both(lib, q, t, mat, costs, m, flag=0, exp=None, msg=""):
    """the pointer and the flat align entry (host arena, bytes that no matrix admits between the sequences) against the contract; the score
    entries return its score, qe and te bit for bit"""
    exp = d.expected(q, t, mat, costs, m, flag) if exp is None else exp
    d.assert_same(lib.sgd_align_batch(list(q), list(t), mat, *costs, flag=flag, m=m), exp, str(msg))
    ar = lf.arena(q, t, lead=3, gap=2)
    d.assert_same(lib.sgd_align_batch_flat(*ar, mat, *costs, flag=flag, m=m), exp, str((msg, "flat")))
    want = [(e["score"], e["qe"], e["te"]) for e in exp]
    assert want == [tuple(int(x) for x in r) for r in lib.sgd_batch(list(q), list(t), mat, *costs, m=m)], msg
    assert want == [tuple(int(x) for x in r) for r in lib.sgd_batch_flat(*ar, mat, *costs, m=m)], msg
    return exp


# ---------------------------------------------------------------- the oracle itself

def test_oracle_equals_the_golden_file_of_the_compiled_reference():
    total = empty = negative = 0
    seen = set()
    for name, m, mat, costs, q, t, cells, cig in d.load_golden():
        np.testing.assert_array_equal(d.oracle_cells(q, t, mat, costs, m), cells, name)
        total += len(q)
        empty += int((cells[:, 3] == cells[:, 4] + 1).sum())
        negative += int(((cells[:, 0] < 0) & (cells[:, 3] <= cells[:, 4])).sum())
        seen.add(costs)
    assert total == 324 and empty >= 10 and negative >= 10
    assert {(4, 2, 24, 1), (24, 1, 4, 2), (0, 1, 5, 0), (6, 3, 0, 0)} <= seen and any(c[:2] == c[2:] for c in seen)


def test_golden_file_is_data_only():
    z = np.load(d.GOLDEN)
    assert all(re.fullmatch(r"ngroups|g\d+_(name|costs|cells|ncig\d+|cig\d+)", k) for k in z.files), z.files
    assert os.path.getsize(d.GOLDEN) < 200 << 10


def test_golden_cigars_rescore_under_the_two_piece_cost():
    for name, m, mat, costs, q, t, cells, cig in d.load_golden():
        for i, (sc, qb, qe, tb, te) in enumerate(cells.tolist()):
            for fl in d.FLAGS:
                want = (sc, len(q[i]), te - tb + 1)
                assert ld_rescore(cig[fl][i], q[i], t[i][tb:te + 1], mat, m, costs, bool(fl & d.REV_CIGAR)) == want, (name, i, fl)


def ld_rescore(cigar, query, target, mat, m, costs, rev):
    from tests import lld_util as ld
    return ld.rescore(cigar, query, target, mat, m, costs, rev=rev)


def test_oracle_and_library_by_brute_force(sim):
    """tests/sgd_oracle.c against plain Python over full matrices (forward formula, then G(x) for EVERY x), the four costs drawn
    independently so that the pieces come in both orders, matrices without a positive entry, homopolymers (every row ties); the library
    (simulator build, biased and clamped values) returns the same, and differs from the single-piece result often enough."""
    rng = np.random.default_rng(5)
    seen_empty = seen_neg = seen_diff = 0
    pool = (0, 0, 1, 2, 3, 5, 9)
    for ci in range(14):
        costs = tuple(int(rng.choice(pool)) for _ in range(4)) if ci >= 4 else COSTS[ci]
        m, mat = ((3, np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)), (4, u.random_mat(rng, 4, -6, 1)), (2, u.random_mat(rng, 2)))[ci % 3]
        qs, ts = [], []
        for k in range(30):
            al = 1 if k % 5 == 0 else m
            q = rng.integers(0, al, int(rng.integers(1, 9)), dtype=np.uint8)
            t = rng.integers(0, al, int(rng.integers(1, 15)), dtype=np.uint8)
            if k % 4 == 0:                           # a copy with a deletion planted
                t = np.concatenate([t[:3], q[:len(q) // 2], t[3:5], q[len(q) // 2:], t[5:]]).astype(np.uint8)
            qs.append(q); ts.append(t)
        exp = np.array([d.brute(q, t, mat, costs, m) for q, t in zip(qs, ts)], dtype=np.int32)
        np.testing.assert_array_equal(d.oracle_cells(qs, ts, mat, costs, m), exp, str((costs, m)))
        seen_empty += int((exp[:, 3] == exp[:, 4] + 1).sum())
        seen_neg += int(((exp[:, 0] < 0) & (exp[:, 3] <= exp[:, 4])).sum())
        seen_diff += int((a.oracle_cells(qs, ts, mat, costs[0], costs[1], m) != exp).any(axis=1).sum())
        os.environ["KSW2AMD_LL_FORM"] = str(ci % 3)
        got = sim.sgd_align_batch(qs, ts, mat, *costs, flag=d.SCORE_ONLY, m=m)
        assert d.cells_of(got) == exp.tolist(), (costs, m)
    assert seen_empty > 30 and seen_neg > 30 and seen_diff > 30


# ---------------------------------------------------------------- the library on the simulator

@pytest.mark.parametrize("form", ["0", "1", "2"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_ragged_batch_every_form(sim, form, lds):
    rng = np.random.default_rng(11 + int(form))
    os.environ["KSW2AMD_LL_FORM"] = form
    os.environ["KSW2AMD_LL_LDS"] = lds
    for m, mat in ((5, u.simple_mat(5, 2, 4, -1)), (20, _m20(rng)), (4, u.random_mat(rng, 4, -6, 1))):
        q, t = u.ragged(rng, 12, m, 1, 90, related=0.6)
        t = [np.concatenate([rng.integers(0, m, int(rng.integers(0, 120)), dtype=np.uint8), x, rng.integers(0, m, int(rng.integers(0, 80)), dtype=np.uint8)]) for x in t]
        q += [q[0], q[0], q[1]]
        t += [t[0], t[0][::-1].copy(), t[1]]                               # same-shape partners for form 1
        t[3] = np.concatenate([rng.integers(0, m, 1100, dtype=np.uint8), q[3]])    # two generations in the reversed pass as well
        t[4] = np.concatenate([q[4], rng.integers(0, m, 1030, dtype=np.uint8)])
        for costs in COSTS[:2] if m == 20 else COSTS:
            _both(sim, q, t, mat, costs, m, msg=(form, lds, m, costs))


@pytest.mark.parametrize("form", ["0", "2"])
def test_golden_file_on_the_simulator(sim, form):
    os.environ["KSW2AMD_LL_FORM"] = form
    for name, m, mat, costs, q, t, cells, cig in d.load_golden():
        for fl in d.FLAGS if form == "0" else (0,):
            got = sim.sgd_align_batch(q, t, mat, *costs, flag=fl, m=m)
            assert d.cells_of(got) == cells.tolist(), (name, fl)
            assert [g["cigar"] for g in got] == cig[fl], (name, fl)


@pytest.mark.parametrize("form", ["0", "2"])
def test_edge_grid(sim, form):
    """the best row planted at 15 / 16 / 1 023 / 1 024 / tlen - 1 for queries of 1 .. 65 in targets of 1 .. 2 049"""
    rng = np.random.default_rng(77)
    os.environ["KSW2AMD_LL_FORM"] = form
    qs, ts = s.edge_grid(rng, 5, tlens=(1, 16, 17, 1024, 1025, 2049), qlens=(1, 2, 5, 63, 65))
    exp = _both(sim, qs, ts, s.unit_mat(5), d.CROSS, 5, flag=d.SCORE_ONLY, msg=form)
    assert {15, 16, 1023, 1024, 2048} <= {e["te"] for e in exp}


def test_the_second_piece_along_both_axes(sim):
    """a 40-residue deletion (E2 down the rows, across the lane rotate and -- rows 1 000 .. 1 039 -- the 16-byte boundary) and a 40-residue
    insertion (F2 along the columns, in row 63 / 1 023): under (4, 2, 24, 1) the long gap costs 64, not 84, and the gap of one beside it 6,
    not 25 -- neither single-piece result"""
    rng = np.random.default_rng(8)
    mat = s.unit_mat(5)
    for form in ("0", "2"):
        os.environ["KSW2AMD_LL_FORM"] = form
        qs, ts, want = [], [], []
        for deletion, at, gap_at in ((True, 0, 60), (True, 950, 50), (False, 0, 64), (False, 950, 74)):
            q, t, (tb, te) = d.gapped_copy(rng, 1300, 200, at, gap_at, 40, deletion, short_at=170)
            qs.append(q); ts.append(t); want.append((2 * (199 if deletion else 159) - 64 - 6, tb, te))
        exp = _both(sim, qs, ts, mat, d.CROSS, 5, msg=form)
        assert [(e["score"], e["tb"], e["te"]) for e in exp] == want
        for go, ge in ((4, 2), (24, 1)):
            one = sim.sg_batch(qs, ts, mat, go, ge, m=5)
            assert all(int(r[0]) < w[0] for r, w in zip(one, want)), (go, ge)
    assert ts[1][1000:1040].max() <= 1                 # the deletion is open when lane 63 hands E2 to the boundary


def test_row_minus_one_and_column_minus_one_under_the_second_piece(sim):
    """target = query[30:] + other letters: the first 30 query residues are inserted before target[0] at cost(30) = 54, not 64 (fit_top);
    the mirror image ends the query with a 30-residue insertion, which the reverse pass takes along its row -1, and its column -1 runs
    past row 20 where the pieces cross (fit_left)"""
    rng = np.random.default_rng(12)
    mat = s.unit_mat(5)
    for form in ("0", "2"):
        os.environ["KSW2AMD_LL_FORM"] = form
        q1, t1 = d.suffix_copy(rng, 100, 30, 60)
        q2, t2 = d.suffix_copy(rng, 100, 30, 60, mirror=True)
        exp = _both(sim, [q1, q2], [t1, t2], mat, d.CROSS, 5, msg=form)
        assert (exp[0]["score"], exp[0]["tb"], exp[0]["te"], exp[0]["cigar"]) == (140 - 54, 0, 69, [30 << 4 | 1, 70 << 4])
        assert (exp[1]["score"], exp[1]["tb"], exp[1]["te"]) == (140 - 54, 60, 129)
        c = exp[1]["cigar"]                          # (ksw_extd places the insertion as far left as the tail's own repeats allow)
        assert [x >> 4 for x in c if x & 0xf == 1] == [30] and sum(x >> 4 for x in c if x & 0xf == 0) == 70 and all(x & 0xf < 2 for x in c)


def test_ties_take_the_smallest_te(sim):
    qs, ts, tes = s.tie_pairs(5)
    for form in ("0", "2"):
        os.environ["KSW2AMD_LL_FORM"] = form
        exp = _both(sim, qs, ts, u.simple_mat(5, 2, 4, -1), d.CROSS, 5, flag=d.SCORE_ONLY, msg=form)
        assert [e["te"] for e in exp] == tes and all(e["score"] == 12 and e["tb"] == e["te"] - 5 for e in exp)


@pytest.mark.parametrize("order", [0, 1])
def test_uneven_halves_of_a_packed_task(sim, order, capfd):
    rng = np.random.default_rng(31 + order)
    os.environ["KSW2AMD_LL_FORM"] = "1"
    os.environ["KSW2AMD_TRACE"] = "1"
    mat = s.unit_mat(5)
    qs, ts = a.uneven_halves(rng, 5, 2100, 40, (45, 2090))
    if order:
        qs, ts = qs[::-1], ts[::-1]
    capfd.readouterr()
    exp = _both(sim, qs, ts, mat, d.CROSS, 5, msg=order)
    err = capfd.readouterr().err
    assert "sgda: pairs=2 pk_tasks=1 int32_tasks=0" in err and "sgda-rev: pk_tasks=1 int32_tasks=0" in err and "sgd: pairs=2 pk_tasks=1" in err, err
    assert " pk_profile=lds" not in err
    assert sorted(e["te"] for e in exp) == [45, 2090] and all(e["te"] - e["tb"] + 1 == 40 for e in exp)
    # the whole query inserted at cost(40) = 64 beside a copy that ends in row 2 090
    q1, t1 = a.planted_copy(rng, 5, 2100, 40, 2090)
    q2, t2 = rng.integers(2, 4, 40, dtype=np.uint8), rng.integers(0, 2, 2100, dtype=np.uint8)
    qs, ts = ([q1, q2], [t1, t2]) if order == 0 else ([q2, q1], [t2, t1])
    exp = _both(sim, qs, ts, mat, d.CROSS, 5, msg=("empty", order))
    e = exp[1 - order]
    assert (e["score"], e["tb"], e["te"], e["cigar"]) == (-64, 1, 0, [40 << 4 | 1])


def test_admission_bound(sim, capfd):
    """smax = 127, costs (5, 3, 60, 1): B = min(5 + 3 q, 60 + q) = 60 + q from q = 28 on, so B + (qlen + 1) * smax = 128 qlen + 187 <= 65 535
    up to qlen 510; under the first piece alone (130 qlen + 132) a query of 510 would not be admitted"""
    os.environ["KSW2AMD_LL_FORM"] = "2"
    os.environ["KSW2AMD_TRACE"] = "1"
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    costs = (5, 3, 60, 1)
    for ql, packed in ((510, True), (511, False)):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q, rng.integers(0, 4, 9, dtype=np.uint8)])
        capfd.readouterr()
        got = sim.sgd_align_batch([q], [t], mat, *costs, m=4)
        err = capfd.readouterr().err
        assert (got[0]["score"], got[0]["tb"], got[0]["te"], got[0]["cigar"]) == (127 * ql, 20, 20 + ql - 1, [ql << 4])
        d.assert_same(got, d.expected([q], [t], mat, costs, 4))
        assert ("sgda: pairs=1 pk_tasks=%d int32_tasks=%d" % ((1, 0) if packed else (0, 1))) in err, err
        assert ("sgda-rev: pk_tasks=%d int32_tasks=%d" % ((1, 0) if packed else (0, 1))) in err, err
    capfd.readouterr()
    sim.sg_batch([q[:510]], [t], mat, 5, 3, m=4)
    assert "sg: pairs=1 pk_tasks=0 int32_tasks=1" in capfd.readouterr().err


def test_scores_beyond_16_bits_and_negative_optima(sim):
    rng = np.random.default_rng(4)
    os.environ["KSW2AMD_LL_FORM"] = "2"
    q = rng.integers(0, 4, 1700, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q, rng.integers(0, 4, 11, dtype=np.uint8)])
    exp = _both(sim, [q], [t], u.simple_mat(4, 40, 30), d.CROSS, 4)
    assert exp[0]["score"] == 40 * 1700 > 65535 and (exp[0]["tb"], exp[0]["te"]) == (30, 1729)
    q, t = np.zeros(40, np.uint8), np.ones(300, np.uint8)
    exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), (120, 110, 127, 100), 4)
    assert exp[0]["score"] < -100 and exp[0]["tb"] <= exp[0]["te"]
    exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), (2, 1, 30, 0), 4)
    assert (exp[0]["score"], exp[0]["tb"], exp[0]["te"], exp[0]["cigar"]) == (-30, 1, 0, [40 << 4 | 1])


@pytest.mark.parametrize("costs", [(4, 2, 4, 2), (4, 2, 9, 5), (0, 1, 0, 1), (3, 0, 3, 2)])
def test_equal_or_dominated_second_piece_equals_the_single_piece_entries(sim, costs):
    rng = np.random.default_rng(19)
    os.environ["KSW2AMD_LL_FORM"] = "1"
    for mat in (u.simple_mat(5, 2, 4, -1), u.random_mat(rng, 5, -6, 1)):
        q, t = u.ragged(rng, 14, 5, 1, 90, related=0.6)
        t = [np.concatenate([rng.integers(0, 5, int(rng.integers(0, 200)), dtype=np.uint8), x]) for x in t]
        q += [np.zeros(0, np.uint8), q[0]]
        t += [t[0], np.zeros(0, np.uint8)]
        for fl in (0, d.RIGHT):
            one = sim.sg_align_batch(q, t, mat, costs[0], costs[1], flag=fl, m=5)
            two = sim.sgd_align_batch(q, t, mat, *costs, flag=fl, m=5)
            assert [{f: g[f] for f in d.FIELDS} for g in two] == [{f: g[f] for f in d.FIELDS} for g in one], (costs, fl)
        np.testing.assert_array_equal(sim.sgd_batch(q, t, mat, *costs, m=5), sim.sg_batch(q, t, mat, costs[0], costs[1], m=5))
        ar = lf.arena(q, t, lead=1, gap=1)
        np.testing.assert_array_equal(sim.sgd_batch_flat(*ar, mat, *costs, m=5), sim.sg_batch_flat(*ar, mat, costs[0], costs[1], m=5))


def test_all_three_flags_and_buffer_reuse(sim):
    rng = np.random.default_rng(6)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 20, 120, related=1.0)
    t = [np.concatenate([rng.integers(0, 5, 40, dtype=np.uint8), x]) for x in t]
    q.append(np.array([0, 0, 1, 1], np.uint8)); t.append(np.array([0, 0, 0, 1, 1], np.uint8))      # left / right placement of a gap differs
    q.append(np.full(9, 2, np.uint8)); t.append(np.full(50, 1, np.uint8))                            # an empty interval: qlen I from the host
    cig = {}
    for fl in (0, d.RIGHT, d.REV_CIGAR, d.RIGHT | d.REV_CIGAR):
        cig[fl] = [e["cigar"] for e in _both(sim, q, t, mat, d.CROSS, 5, flag=fl, msg=fl)]
    assert cig[0] != cig[d.RIGHT] and cig[d.REV_CIGAR] == [c[::-1] for c in cig[0]]
    exp = d.expected(q, t, mat, d.CROSS, 5)
    assert exp[-1]["cigar"] == [9 << 4 | 1]
    # a second call into the same records must not reallocate a buffer that is large enough; SCORE_ONLY leaves the buffers alone
    n = len(q)
    aln = (ksw2_amd.LocalAln * n)()
    sim.sgd_align_batch(q, t, mat, *d.CROSS, m=5, aln=aln)
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    assert all(p and mc >= x.n_cigar > 0 for (p, mc), x in zip(first, aln))
    got = sim.sgd_align_batch(q[::-1], t[::-1], mat, *d.CROSS, m=5, aln=aln)
    d.assert_same(got, exp[::-1])
    for k, x in enumerate(aln):
        if x.n_cigar <= first[k][1]:
            assert (ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) == first[k]
    second = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    got = sim.sgd_align_batch(q, t, mat, *d.CROSS, flag=d.SCORE_ONLY, m=5, aln=aln)
    assert all(g["n_cigar"] == 0 for g in got) and d.cells_of(got) == d.cells_of(exp)
    assert [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == second
    for x in aln:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


def test_corner_results_launch_nothing(sim):
    e = np.zeros(0, np.uint8)
    q = np.array([0, 1, 2, 3, 0] * 6, np.uint8)          # 30 residues: cost(30) = 54 under (4, 2, 24, 1), 64 under its first piece
    mat = u.simple_mat(5, 2, 4, -1)
    ins = dict(score=-54, qb=0, qe=29, tb=0, te=-1, n_cigar=1, cigar=[30 << 4 | 1])
    d.launches(sim, reset=True)
    for costs in (d.CROSS, (24, 1, 4, 2)):
        got = sim.sgd_align_batch([e, q, e], [q, e, e], mat, *costs, m=5)
        assert [{f: g[f] for f in d.FIELDS} for g in got] == [RESET, ins, RESET]
        d.assert_same(got, d.expected([e, q, e], [q, e, e], mat, costs, 5))
        got = sim.sgd_align_batch_flat(*lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, *costs, m=5)
        assert [{f: g[f] for f in d.FIELDS} for g in got] == [RESET, ins, RESET]
        got = sim.sgd_align_batch([e, q, e], [q, e, e], mat, *costs, flag=d.SCORE_ONLY, m=5)
        assert [{f: g[f] for f in d.FIELDS} for g in got] == [RESET, dict(ins, n_cigar=0, cigar=[]), RESET]
        assert sim.sgd_batch([e, q, e], [q, e, e], mat, *costs, m=5).tolist() == [[0, -1, -1], [-54, 29, -1], [0, -1, -1]]
        assert sim.sgd_batch_flat(*lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, *costs, m=5).tolist() == [[0, -1, -1], [-54, 29, -1], [0, -1, -1]]
    assert d.launches(sim)[:3] == (0, 0, 0)
    assert sim.sgd_align_batch([], [], mat, *d.CROSS, m=5) == [] and len(sim.sgd_batch([], [], mat, *d.CROSS, m=5)) == 0
    # corners beside a real pair; the single-pair entries
    got = sim.sgd_align_batch([q, e, q], [e, q, q], mat, *d.CROSS, m=5)
    assert {f: got[0][f] for f in d.FIELDS} == ins and {f: got[1][f] for f in d.FIELDS} == RESET
    assert {f: got[2][f] for f in d.FIELDS} == dict(score=60, qb=0, qe=29, tb=0, te=29, n_cigar=1, cigar=[30 << 4])
    assert {f: sim.sgd_align(q, e, mat, *d.CROSS)[f] for f in d.FIELDS} == ins
    assert {f: sim.sgd_align(e, q, mat, *d.CROSS)[f] for f in d.FIELDS} == RESET
    assert sim.sgd_align(q, q, mat, *d.CROSS)["cigar"] == [30 << 4]
    assert sim.sgd(q, e, mat, *d.CROSS) == (-54, 29, -1) and sim.sgd(e, q, mat, *d.CROSS) == (0, -1, -1) and sim.sgd(q, q, mat, *d.CROSS) == (60, 29, 29)
    # m = 1 is legal for the score entries
    one = np.array([3], np.int8)
    z = np.zeros(7, np.uint8)
    assert sim.sgd_batch([z[:4]], [z], one, *d.CROSS, m=1).tolist() == [[12, 3, 3]]


def test_bad_arguments(sim):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = sim.local_pairs(q, t)
    aln = (ksw2_amd.LocalAln * 6)()
    res = np.zeros((6, 3), np.int32)
    rp = res.ctypes.data_as(ctypes.POINTER(ksw2_amd.LocalResult))
    L = sim.lib
    mp = mat.ctypes.data_as(_i8p)
    ar = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = sim._local_flat(*ar, None)
    E = E_PARAM
    d.launches(sim, reset=True)
    bad = [(0, mp, 4, 2, 24, 1), (128, mp, 4, 2, 24, 1), (5, None, 4, 2, 24, 1), (5, mp, 128, 2, 24, 1), (5, mp, 4, 128, 24, 1), (5, mp, 4, 2, 128, 1),
           (5, mp, 4, 2, 24, 128), (5, mp, -1, 2, 24, 1), (5, mp, 4, -1, 24, 1), (5, mp, 4, 2, -1, 1), (5, mp, 4, 2, 24, -1)]
    for args in bad:
        assert L.ksw2amd_sgd_align_batch(None, *args, 0, 6, pairs, aln) == E, args
        assert L.ksw2amd_sgd_align_batch_flat(None, *args, 0, 6, ctypes.byref(f), aln) == E, args
        assert L.ksw2amd_sgd_batch(*args, 6, pairs, rp) == E, args
        assert L.ksw2amd_sgd_batch_flat(*args, 6, ctypes.byref(f), rp) == E, args
    # m = 1: the align entries only
    one = np.array([3], np.int8)
    z = [np.zeros(4, np.uint8)] * 6
    zp, keepz = sim.local_pairs(z, z)
    fz, _, keepz2 = sim._local_flat(*lf.arena(z, z, lead=1, gap=1), None)
    assert L.ksw2amd_sgd_align_batch(None, 1, one.ctypes.data_as(_i8p), 4, 2, 24, 1, 0, 6, zp, aln) == E and "m >= 2" in sim.last_error()
    assert L.ksw2amd_sgd_align_batch_flat(None, 1, one.ctypes.data_as(_i8p), 4, 2, 24, 1, 0, 6, ctypes.byref(fz), aln) == E
    dd = sim.sgd_align(z[0], z[0], one, 4, 2, 24, 1, m=1)
    assert {k: dd[k] for k in d.FIELDS} == RESET and "m >= 2" in sim.last_error()
    for flag in (0x04, 0x08, 0x10, 0x20, 0x40, 0x100, 0x03 | 0x400):           # anything but SCORE_ONLY / RIGHT / REV_CIGAR
        assert L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, flag, 6, pairs, aln) == E, flag
        assert L.ksw2amd_sgd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, flag, 6, ctypes.byref(f), aln) == E, flag
    assert "flag accepts" in sim.last_error()
    assert L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, 0, 6, None, aln) == E and L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, 0, 6, pairs, None) == E
    assert L.ksw2amd_sgd_align_batch(None, 5, mp, 4, 2, 24, 1, 0, -1, pairs, aln) == E
    assert L.ksw2amd_sgd_batch(5, mp, 4, 2, 24, 1, 6, None, rp) == E and L.ksw2amd_sgd_batch(5, mp, 4, 2, 24, 1, 6, pairs, None) == E
    assert L.ksw2amd_sgd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, 0, 6, None, aln) == E
    assert L.ksw2amd_sgd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, 0, 6, ctypes.byref(f), None) == E
    # a code >= m: named by the pointer entry before anything runs
    bad_t = [x.copy() for x in t]
    bad_t[4][3] = 5
    bad_t[2][len(bad_t[2]) - 1] = 9
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        sim.sgd_align_batch(q, bad_t, mat, *d.CROSS, m=5)
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        sim.sgd_batch(q, bad_t, mat, *d.CROSS, m=5)
    assert d.launches(sim)[:3] == (0, 0, 0)
    # the range limit: cost(qlen) + (qlen + 1) * smax > 0x3fffffff, with cost() the min -- the second piece decides (only the length is looked at)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    bp = big.ctypes.data_as(_i8p)
    lim = 0x3fffffff

    def total(ql, c):
        return d.gap_cost(c, ql) + (ql + 1) * 127
    c = (127, 127, 0, 0)
    ql = (lim - 127) // 127 + 1
    assert total(ql, c) > lim >= total(ql - 1, c) and 127 + ql * 254 + 127 > lim
    pairs[1].qlen = ql
    assert L.ksw2amd_sgd_align_batch(None, 5, bp, *c, 0, 1, ctypes.byref(pairs[1]), aln) == E and "0x3fffffff" in sim.last_error()
    assert L.ksw2amd_sgd_batch(5, bp, *c, 1, ctypes.byref(pairs[1]), rp) == E
    pairs[1].qlen = len(q[1])
    ql_arr = ar[2].copy()
    ql_arr[3] = ql
    f2, _, keep3 = sim._local_flat(ar[0], ar[1], ql_arr, ar[3], ar[4], None)
    assert L.ksw2amd_sgd_align_batch_flat(None, 5, bp, *c, 0, 6, ctypes.byref(f2), aln) == E and "pair 3" in sim.last_error()
    assert L.ksw2amd_sgd_batch_flat(5, bp, *c, 6, ctypes.byref(f2), rp) == E
    assert d.launches(sim) == (0, 0, 0, 0)                                   # nothing of all this launched anything
    # the single-pair entries report like ksw_ll_i16: 0 with the reset values, the error counted
    before = sim.error_count()
    rec = ksw2_amd.LocalAln()
    rec.score = 5; rec.tb = 5
    tp = t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.ksw2amd_sgd_align(None, None, 3, tp, 4, 2, 24, 1, 0, ctypes.byref(rec)) == 0
    assert (rec.score, rec.qb, rec.qe, rec.tb, rec.te, rec.n_cigar) == (0, -1, -1, -1, -1, 0)
    assert sim.error_count() > before and "NULL profile" in sim.last_error()
    assert sim.sgd(q[0], t[0], mat, 4, 2, 200, 1) == (0, -1, -1) and "gapo and gape" in sim.last_error()


def test_chunked_flat_batches(sim):
    """KSW2AMD_LL_CHUNK_BYTES cuts the flat batch into several chunks: the same results; a bad code in a later chunk resets EVERY entry"""
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 40, 5, 10, 200)
    q[7], t[9] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    exp = d.expected(q, t, mat, d.CROSS, 5)
    ar = lf.arena(q, t, lead=1, gap=1)
    os.environ["KSW2AMD_LL_CHUNK_BYTES"] = "4000"
    d.launches(sim, reset=True)
    d.assert_same(sim.sgd_align_batch_flat(*ar, mat, *d.CROSS, m=5), exp)
    n = d.launches(sim)
    assert n[3] > 3 and n[0] > 3 and n[1] == n[0] and n[2] == 0              # a start pass behind every forward launch, no single-piece twin
    assert sim.sgd_batch_flat(*ar, mat, *d.CROSS, m=5).tolist() == [[e["score"], e["qe"], e["te"]] for e in exp]
    bad = ar[0].copy()
    bad[int(ar[3][30]) + 1] = 6
    aln = (ksw2_amd.LocalAln * 40)()
    for x in aln:
        x.score = 7; x.qb = x.qe = x.tb = x.te = 7
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
        sim.sgd_align_batch_flat(bad, *ar[1:], mat, *d.CROSS, m=5, aln=aln)
    assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)
    out = np.full((40, 3), 7, np.int32)
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
        sim.sgd_batch_flat(bad, *ar[1:], mat, *d.CROSS, m=5, out=out)
    assert (out[30:] == [0, -1, -1]).all()                                   # the failing chunk and the later ones: reset values


# ---------------------------------------------------------------- the drop-in boundary

def test_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ksw2_amd.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in ksw2_amd.EXPORTS and name in ksw2_amd._ENV_ENTRIES
    if not os.path.exists(ksw2_amd.DEFAULT_SO):
        subprocess.run(["make", "-C", os.path.join(ROOT, "ksw2_amd", "csrc")], check=True, capture_output=True)
    lib = ctypes.CDLL(ksw2_amd.DEFAULT_SO)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_c_caller(simso, tmp_path):
    exe = str(tmp_path / "sgd_caller")
    libdir = os.path.dirname(simso)
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "sgd_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 10, 5, 1, 80, related=0.8)
    t = [np.concatenate([rng.integers(0, 5, 100, dtype=np.uint8), x, rng.integers(0, 5, 200, dtype=np.uint8)]) for x in t]
    q.append(np.zeros(0, np.uint8)); t.append(t[0])
    q.append(q[0]); t.append(np.zeros(0, np.uint8))
    q.append(np.full(6, 2, np.uint8)); t.append(np.full(30, 1, np.uint8))    # an empty interval
    q2, t2, _ = d.gapped_copy(rng, 300, 120, 40, 50, 40, True)
    q.append(q2); t.append(t2)
    for flag in (0, d.RIGHT | d.REV_CIGAR):
        inp = str(tmp_path / "pairs.txt")
        d.write_input(inp, q, t, mat, 5, d.CROSS, flag)
        out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
        batch, single, _ = la.parse_caller(out)
        exp = d.expected(q, t, mat, d.CROSS, 5, flag)
        d.assert_same(batch, exp, "batch")
        d.assert_same(single, exp, "single")


def test_only_the_new_host_object_names_the_two_piece_launchers(tmp_path):
    """the other tests' simulator builds link the other host objects against twins without k2a_shim_launch_sgd / _rev and load with
    immediate binding"""
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    for src in sorted(os.listdir(csrc)):
        if not re.fullmatch(r"ksw2_host_\w+\.c", src):
            continue
        o = str(tmp_path / (src[:-2] + ".o"))
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, src), "-o", o], check=True)
        undefined = subprocess.run(["nm", "-u", o], check=True, capture_output=True, text=True).stdout.split()
        for sym in ("k2a_shim_launch_sgd", "k2a_shim_launch_sgd_rev"):
            assert (sym in undefined) == (src == "ksw2_host_sgd.c"), (src, sym)
        if src == "ksw2_host_sgd.c":
            assert "k2a_shim_launch_sg" not in undefined and "k2a_shim_launch_sg_rev" not in undefined
