"""CPU: overlap alignment with the start cell and a CIGAR (ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch, their flat forms and the
single-pair entries; include/ksw2_amd.h).  The contract's start cell (tests/ova_oracle.c) is pinned to the compiled
reference's scalar ksw_extz / ksw_extd through tests/golden/ova_cases.npz and to a brute-force statement of the candidate set and the tie
rule; the product's host code and lane code (K2aLaneLL<.., REV, .., FIT, OV>, both number formats, both score lookups, both gap costs) run
on a test-local lock-step simulator build against that oracle; a C caller compiled against include/ksw2_amd.h prints the contract's answers."""
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
from tests import ov_util as o
from tests import ova_util as a
from tests import sg_util as s
from tests import sga_util as sa
from tests import sgd_util as d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (0, 0), (4, 2, 24, 1), (24, 1, 4, 2))
NAMES = ("ksw2amd_ov_align_batch", "ksw2amd_ov_align_batch_flat", "ksw2amd_ov_align",
         "ksw2amd_ovd_align_batch", "ksw2amd_ovd_align_batch_flat", "ksw2amd_ovd_align")
RESET = dict(score=0, qb=-1, qe=-1, tb=-1, te=-1, n_cigar=0, cigar=[])
E_PARAM = -2


@pytest.fixture(scope="module")
def simso(tmp_path_factory):
    return a.sim_library(str(tmp_path_factory.mktemp("ovasim") / "libksw2_amd.so"))


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


def _form(form, lds="0"):
    os.environ["KSW2AMD_LL_FORM"] = form
    os.environ["KSW2AMD_LL_LDS"] = lds


def _both(lib, q, t, mat, costs, ends, m, flag=0, exp=None, msg="", flat=True):
    """the pointer entry and the flat entry (host arena with bytes that no matrix admits between the sequences) against the contract;
    score, qe, te are ksw2amd_ov_batch's bit for bit"""
    exp = a.expected(q, t, mat, costs, ends, m, flag) if exp is None else exp
    a.assert_same(a.call(lib, q, t, mat, costs, ends, m, flag), exp, str((msg, costs, ends)))
    if flat:
        a.assert_same(a.call_flat(lib, lf.arena(q, t, lead=3, gap=2), mat, costs, ends, m, flag), exp, str((msg, costs, ends, "flat")))
    fwd = o.call(lib, q, t, mat, costs, ends, m)
    assert [(e["score"], e["qe"], e["te"]) for e in exp] == [tuple(int(x) for x in r) for r in fwd], msg
    return exp


def _cells(lib, q, t, mat, costs, ends, m):
    return np.array(a.cells_of(a.call(lib, q, t, mat, costs, ends, m, a.SCORE_ONLY)), dtype=np.int32).reshape(-1, 5)


# ---------------------------------------------------------------- 1. the oracle itself

def test_oracle_equals_the_golden_file_of_the_compiled_reference():
    total = row0 = empty_t = empty_q = 0
    for name, m, mat, c2, c4, q, t, per in a.load_golden():
        for (kind, e), (cells, cig) in per.items():
            np.testing.assert_array_equal(a.oracle_cells(q, t, mat, c2 if kind == "ov" else c4, e, m), cells, str((name, kind, e)))
            row0 += int((cells[:, 1] > 0).sum())
            empty_t += int((cells[:, 3] > cells[:, 4]).sum())
            empty_q += int((cells[:, 1] > cells[:, 2]).sum())
        total += len(q)
    assert total == 324 and row0 > 100 and empty_t > 20 and empty_q > 20


def test_golden_file_is_data_only_and_small():
    z = np.load(a.GOLDEN)
    assert all(re.fullmatch(r"ngroups|g\d+_ovd?[123]_(qb|tb|ncig\d+|cig\d+)", k) for k in z.files), z.files
    assert os.path.getsize(a.GOLDEN) < 1 << 18


def test_ends_0_of_the_oracle_is_the_semiglobal_golden_file():
    for g, gd in zip(sa.load_golden(), d.load_golden()):
        name, m, mat, gapo, gape, q, t, cells, _ = g
        np.testing.assert_array_equal(a.oracle_cells(q, t, mat, (gapo, gape), 0, m), cells, name)
        np.testing.assert_array_equal(a.oracle_cells(q, t, mat, gd[3], 0, m), gd[6], name)


def test_oracle_is_the_contract_by_brute_force(sim):
    """tests/ova_oracle.c against G of EVERY candidate start cell by a global matrix of its own in plain Python and the tie rule; costs
    with 0, two pieces in both orders, matrices without a positive entry, homopolymers (everything ties), every ends; the library
    (simulator build, biased and clamped values) returns the same."""
    rng = np.random.default_rng(5)
    seen = dict(row0=0, empty_t=0, empty_q=0, inside=0, tie_empty=0)
    for ci, costs in enumerate(((4, 2), (0, 1), (3, 0), (0, 0), (1, 1), (4, 2, 24, 1), (24, 1, 4, 2), (0, 1, 5, 0))):
        for m, mat in ((3, np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)), (4, u.random_mat(rng, 4, -6, 1)), (2, u.random_mat(rng, 2))):
            qs, ts = [], []
            for k in range(24):
                al = 1 if k % 5 == 0 else m                                  # homopolymers: everything ties
                q = rng.integers(0, al, int(rng.integers(1, 11)), dtype=np.uint8)
                t = rng.integers(0, al, int(rng.integers(1, 19)), dtype=np.uint8)
                if k % 3 == 0:
                    p = int(rng.integers(1, len(q) + 1))
                    t = np.concatenate([q[len(q) - p:], t, q[:p]]).astype(np.uint8)      # a suffix at the head, a prefix at the tail
                qs.append(q); ts.append(t)
            for ends in range(4):
                exp = np.array([a.brute(q, t, mat, costs, ends, m) for q, t in zip(qs, ts)], dtype=np.int32)
                np.testing.assert_array_equal(a.oracle_cells(qs, ts, mat, costs, ends, m), exp, str((costs, m, ends)))
                _form(str(ci % 3), str(ci % 2))
                np.testing.assert_array_equal(_cells(sim, qs, ts, mat, costs, ends, m), exp, str((costs, m, ends)))
                seen["row0"] += int((exp[:, 1] > 0).sum())
                seen["empty_t"] += int((exp[:, 3] > exp[:, 4]).sum())
                seen["empty_q"] += int((exp[:, 1] > exp[:, 2]).sum())
                seen["inside"] += int(((exp[:, 3] > 0) & (exp[:, 3] <= exp[:, 4])).sum())
                for q, t, e in zip(qs[:4], ts[:4], exp[:4]):                 # the empty target interval in a true tie
                    if e[3] == e[4] + 1:
                        c4 = a.four(costs)
                        seen["tie_empty"] += any(a.brute_G(list(map(int, q)), list(map(int, t)), mat, m, c4, tb, qb, int(e[2]), int(e[4])) == e[0]
                                                 for tb, qb in a.candidates(int(e[2]), int(e[4]), ends)[1:])
    assert seen["row0"] > 50 and seen["empty_t"] > 50 and seen["empty_q"] > 20 and seen["inside"] > 50 and seen["tie_empty"] > 5, seen


def test_hand_built_ties(sim):
    qs, ts, es, exp = a.tie_cases()
    mat = s.unit_mat(5)
    for form in ("0", "2"):
        _form(form)
        for q, t, e, x in zip(qs, ts, es, exp):
            assert tuple(int(v) for v in a.oracle_cells([q], [t], mat, (4, 2), e, 5)[0]) == x, (q, t, e)
            assert tuple(_cells(sim, [q], [t], mat, (4, 2), e, 5)[0]) == x, (form, q, t, e)
            assert tuple(_cells(sim, [q], [t], mat, (4, 2, 4, 2), e, 5)[0]) == x, (form, q, t, e, "two-piece")
    # the empty query interval: a mismatch dearer than one deletion, the target one residue long -> (te + 1) D
    dm = a.dear_mismatch_mat()
    got = a.call(sim, [np.array([0, 0], np.uint8)], [np.array([1], np.uint8)], dm, (4, 2), 1, 5)[0]
    assert {f: got[f] for f in a.FIELDS} == dict(score=-6, qb=2, qe=1, tb=0, te=0, n_cigar=1, cigar=[1 << 4 | 2])


# ---------------------------------------------------------------- 2. the library on the simulator

@pytest.mark.parametrize("form,lds", [(f, l) for f in ("0", "1", "2") for l in ("0", "1")])
def test_ragged_batch_every_form(sim, form, lds):
    rng = np.random.default_rng(11 + int(form))
    _form(form, lds)
    for m, mat in ((5, u.simple_mat(5, 2, 4, -1)), (20, u.random_mat(rng, 20, -5, 4)), (4, u.random_mat(rng, 4, -6, 1))):
        q, t = o.ragged_batch(rng, n=24, m=m, qmax=90, tmax=260, long_targets=0)
        q += [q[0], q[0], q[1]]
        t += [t[0], t[0][::-1].copy(), t[1]]                               # same-shape partners for form 1
        t[3] = np.concatenate([rng.integers(0, m, 1100, dtype=np.uint8), q[3][:len(q[3]) // 2 + 1]])      # two generations, a prefix at the tail
        t[4] = np.concatenate([q[4][len(q[4]) // 2:], rng.integers(0, m, 1030, dtype=np.uint8)])
        for costs in COSTS:
            if m == 1:
                continue
            for ends in (0,) + o.ENDS:
                _both(sim, q, t, mat, costs, ends, m, msg=(form, lds, m), flat=ends == 3)


@pytest.mark.parametrize("form", ["0", "2"])
def test_golden_file_on_the_simulator(sim, form):
    _form(form)
    for name, m, mat, c2, c4, q, t, per in a.load_golden():
        for (kind, e), (cells, cig) in per.items():
            costs = c2 if kind == "ov" else c4
            for fl in a.GOLDEN_FLAGS if form == "0" else (0,):
                got = a.call(sim, q, t, mat, costs, e, m, fl)
                assert a.cells_of(got) == cells.tolist(), (name, kind, e, fl)
                assert [g["cigar"] for g in got] == cig[fl], (name, kind, e, fl)


@pytest.mark.parametrize("form", ["0", "2"])
def test_start_row_and_last_column_grids(sim, form):
    """the reversed rectangle's rows (te - tb on both sides of 15 / 16 / 17 and 1 023 / 1 024 / 1 025, tb = 0, tb = 1, the empty target
    interval) and its column limit (qe at the prefetch depth, the 63-step skew, qlen - 2 and qlen - 1 with te = tlen - 1)"""
    rng = np.random.default_rng(70)
    _form(form)
    mat = s.unit_mat(5)
    qs, ts, want = [], [], []
    for span in (15, 16, 17, 18, 1023, 1024, 1025, 1026):
        for lead in (0, 1, 7):
            q, t = a.start_row_pair(rng, span + lead, span)
            qs.append(q); ts.append(t); want.append((lead, span + lead - 1))
    exp = _both(sim, qs, ts, mat, (4, 2), 2, 5, flag=a.SCORE_ONLY, msg=form, flat=False)
    assert [(e["tb"], e["te"]) for e in exp] == want and all(e["qb"] == 0 for e in exp)
    qs, ts, what = o.qend_grid(rng, tlens=(8, 17, 1025), qlens=(5, 64, 65, 130))
    exp = _both(sim, qs, ts, mat, (4, 2, 24, 1), 2, 5, flag=a.SCORE_ONLY, msg=form, flat=False)
    seen = {e["qe"] for (tl, ql, p), e in zip(what, exp) if e["te"] == tl - 1}
    assert {0, 1, 3, 4, 62, 63, 64, 128, 129} <= seen, sorted(seen)
    # the empty target interval beside them (costs (1, 1), a mismatch of -4: inserting the one residue is better)
    q, t = a.start_row_pair(rng, 1030, 1, empty=True)
    e = _both(sim, [q], [t], mat, (1, 1), 2, 5, msg="empty")[0]
    assert (e["score"], e["tb"], e["te"], e["cigar"]) == (-2, 1, 0, [1 << 4 | 1])


@pytest.mark.parametrize("form", ["0", "2"])
def test_last_row_grid(sim, form):
    """the query's start free and the best start in row 0: qb around the prefetch depth and the skew, the last row te at 0, 15, 16, 1 023,
    1 024; the shortest query interval qb = qe; the empty query interval"""
    rng = np.random.default_rng(71)
    _form(form)
    mat = s.unit_mat(5)
    qs, ts, want = [], [], []
    for te in (0, 15, 16, 1023, 1024):
        for qb in (1, 3, 4, 5, 63, 64, 65):
            q, t = a.qbeg_start_pair(rng, te, qb, qb + te + 1)
            qs.append(q); ts.append(t); want.append((qb, qb + te, 0, te))
    for costs in ((4, 2), (4, 2, 24, 1)):
        exp = _both(sim, qs, ts, mat, costs, 1, 5, flag=a.SCORE_ONLY, msg=form, flat=False)
        assert [(e["qb"], e["qe"], e["tb"], e["te"]) for e in exp] == want
        exp = _both(sim, qs, ts, mat, costs, 3, 5, flag=a.SCORE_ONLY, msg=form, flat=False)
        assert [(e["qb"], e["tb"], e["te"]) for e, w in zip(exp, want) if w[3] > 0] == [(w[0], w[2], w[3]) for w in want if w[3] > 0]      # (a target of one residue: the first match wins)
    dm = a.dear_mismatch_mat()
    for tl, ends in ((1, 1), (3, 1), (3, 3)):
        e = _both(sim, [np.array([0, 0, 0], np.uint8)], [np.full(tl, 1, np.uint8)], dm, (4, 2), ends, 5, msg="empty query")[0]
        assert (e["score"], e["qb"], e["tb"], e["te"], e["cigar"]) == (-6, e["qe"] + 1, 0, 0, [1 << 4 | 2])


@pytest.mark.parametrize("order", [0, 1])
def test_packed_halves_that_disagree(sim, order, capfd):
    """pairs of ONE shape in one packed task (asserted from the trace line): te differs, qe differs (one half ends in the last column, the
    other in the last row), one half has an empty interval, the last row's owning generation differs (te 1 000 against 1 030)"""
    rng = np.random.default_rng(31 + order)
    os.environ["KSW2AMD_LL_FORM"] = "1"
    os.environ["KSW2AMD_TRACE"] = "1"
    mat = s.unit_mat(5)

    def run(qs, ts, costs, ends, name):
        if order:
            qs, ts = qs[::-1], ts[::-1]
        capfd.readouterr()
        exp = _both(sim, qs, ts, mat, costs, ends, 5, msg=(name, order), flat=False)
        err = capfd.readouterr().err
        tn = "ovda" if len(costs) == 4 else "ova"
        assert "%s: pairs=2 pk_tasks=1 int32_tasks=0" % tn in err and a.trace_tasks(err, tn)[0] == (1, 0), err
        return exp[::-1] if order else exp

    for costs in ((4, 2), (4, 2, 24, 1)):
        # te differs: copies that end at rows 45 and 2 090
        qs, ts = sa.uneven_halves(rng, 5, 2100, 40, (45, 2090))
        exp = run(qs, ts, costs, 3, "te")
        assert [e["te"] for e in exp] == [45, 2090]
        # qe differs: one half ends in the last column (a whole copy inside), the other in the last row (a prefix at the tail)
        q1, t1 = s.planted(rng, 5, 300, 70, 200)
        q2, t2 = o.qend_pair(rng, 300, 70, 9)
        exp = run([q1, q2], [t1, t2], costs, 2, "qe")
        assert (exp[0]["qe"], exp[1]["qe"], exp[1]["te"]) == (69, 8, 299)
        # the owning generation of the last row differs: the query's start free, targets that are copies of query[qb .. qb + te]
        q1 = rng.integers(2, 4, 1100, dtype=np.uint8)
        q2 = rng.integers(2, 4, 1100, dtype=np.uint8)
        t1 = np.concatenate([q1[60:1061], rng.integers(0, 2, 99, dtype=np.uint8)])          # te = 1 000, qb = 60
        t2 = np.concatenate([q2[30:1061], rng.integers(0, 2, 69, dtype=np.uint8)])          # te = 1 030, qb = 30
        exp = run([q1, q2], [t1, t2], costs, 3, "generation")
        assert [(e["qb"], e["tb"], e["te"]) for e in exp] == [(60, 0, 1000), (30, 0, 1030)]
    # one half with an empty interval (costs (1, 1): a residue without a partner is inserted) beside a copy that ends in row 2 090
    q1, t1 = sa.planted_copy(rng, 5, 2100, 1, 2090)
    q2, t2 = rng.integers(2, 4, 1, dtype=np.uint8), rng.integers(0, 2, 2100, dtype=np.uint8)
    exp = run([q1, q2], [t1, t2], (1, 1), 2, "empty")
    assert (exp[1]["score"], exp[1]["tb"], exp[1]["te"], exp[1]["cigar"]) == (-2, 1, 0, [1 << 4 | 1]) and exp[0]["tb"] == exp[0]["te"] == 2090


def test_int32_form_beyond_the_packed_range(sim, capfd):
    """a score above 65 535 and a query beyond the 16-bit column index take the int32 form, with the same results"""
    rng = np.random.default_rng(4)
    os.environ["KSW2AMD_LL_FORM"] = "2"
    os.environ["KSW2AMD_TRACE"] = "1"
    q = rng.integers(0, 4, 1700, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q[:1500]])
    capfd.readouterr()
    exp = _both(sim, [q], [t], u.simple_mat(4, 40, 30), (4, 2), 3, 4, flag=a.SCORE_ONLY, flat=False)
    assert "ova: pairs=1 pk_tasks=0 int32_tasks=1" in capfd.readouterr().err
    assert exp[0]["score"] == 40 * 1500 and (exp[0]["qb"], exp[0]["qe"], exp[0]["tb"], exp[0]["te"]) == (0, 1499, 30, 1529)
    zero = np.zeros(25, np.int8)                                             # no positive entry, free gaps: B = 0, every length is admitted
    q = rng.integers(0, 5, 65540, dtype=np.uint8)
    t = rng.integers(0, 5, 3, dtype=np.uint8)
    for ends, packed in ((0, True), (1, False), (2, False)):
        capfd.readouterr()
        got = _cells(sim, [q], [t], zero, (0, 0), ends, 5)
        assert ("ova: pairs=1 pk_tasks=%d int32_tasks=%d" % ((1, 0) if packed else (0, 1))) in capfd.readouterr().err
        np.testing.assert_array_equal(got, a.oracle_cells([q], [t], zero, (0, 0), ends, 5))


def test_negative_optima_nonpositive_matrices_free_gaps(sim):
    rng = np.random.default_rng(8)
    _form("2")
    for mat, costs in ((u.random_mat(rng, 5, -7, 1), (3, 1)), (u.random_mat(rng, 5, -7, 1), (0, 0)), (u.simple_mat(5, 2, 4, -1), (0, 0)),
                       (u.simple_mat(5, 1, 100), (120, 110)), (u.random_mat(rng, 5, -7, 1), (0, 0, 3, 0))):
        qs, ts = u.ragged(rng, 10, 5, 1, 60)
        for ends in o.ENDS:
            _both(sim, qs, ts, mat, costs, ends, 5, msg=costs, flat=False)


def test_identities(sim):
    """ends == 0 is the semi-global align entry in every field; equal or dominated second pieces are the single-piece entry"""
    rng = np.random.default_rng(12)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=30, m=5, qmax=80, tmax=200, long_targets=0)
    F = lambda got: [{f: g[f] for f in a.FIELDS} for g in got]
    assert F(a.call(sim, q, t, mat, (4, 2), 0, 5)) == F(sim.sg_align_batch(q, t, mat, 4, 2, m=5))
    assert F(a.call(sim, q, t, mat, (4, 2, 24, 1), 0, 5)) == F(sim.sgd_align_batch(q, t, mat, 4, 2, 24, 1, m=5))
    for ends in o.ENDS:
        one = F(a.call(sim, q, t, mat, (4, 2), ends, 5))
        assert F(a.call(sim, q, t, mat, (4, 2, 4, 2), ends, 5)) == one and F(a.call(sim, q, t, mat, (4, 2, 9, 3), ends, 5)) == one


def test_flags_buffers_and_single_pair_entries(sim):
    rng = np.random.default_rng(6)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=18, m=5, qmax=90, tmax=200, long_targets=0)
    q.append(np.array([0, 0, 1, 1], np.uint8)); t.append(np.array([0, 0, 0, 1, 1], np.uint8))      # left / right placement of a gap differs
    q.append(np.array([0, 0], np.uint8)); t.append(np.array([1], np.uint8))
    for costs in ((4, 2), (4, 2, 24, 1)):
        cig = {}
        for fl in (0, a.RIGHT, a.REV_CIGAR, a.RIGHT | a.REV_CIGAR):
            cig[fl] = [e["cigar"] for e in _both(sim, q, t, mat, costs, 3, 5, flag=fl, msg=fl)]
        assert cig[0] != cig[a.RIGHT] and cig[a.REV_CIGAR] == [c[::-1] for c in cig[0]]
        assert all(g["n_cigar"] == 0 for g in a.call(sim, q, t, mat, costs, 3, 5, a.SCORE_ONLY))
        exp = a.expected(q, t, mat, costs, 1, 5)
        for k in (0, 5, len(q) - 2, len(q) - 1):
            got = sim.ov_align(q[k], t[k], mat, costs[0], costs[1], 1, costs2=costs[2:] if len(costs) == 4 else None)
            assert {f: got[f] for f in a.FIELDS} == {f: exp[k][f] for f in a.FIELDS}
    # a second call into the same records does not reallocate a buffer that is large enough; SCORE_ONLY leaves the buffers alone
    exp = a.expected(q, t, mat, (4, 2), 3, 5)
    aln = (ksw2_amd.LocalAln * len(q))()
    pairs, keep = sim.local_pairs(q, t)
    mp = mat.ctypes.data_as(_i8p)
    assert sim.lib.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, 0, len(q), pairs, aln) == 0
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    assert sim.lib.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, 0, len(q), pairs, aln) == 0
    assert [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    assert all([int(x.cigar[j]) for j in range(x.n_cigar)] == e["cigar"] for x, e in zip(aln, exp))
    assert sim.lib.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, a.SCORE_ONLY, len(q), pairs, aln) == 0
    assert all(x.n_cigar == 0 for x in aln) and [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == first
    for x in aln:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


def test_corners_and_bad_arguments_launch_nothing(sim):
    e = np.zeros(0, np.uint8)
    q = np.array([0, 1, 2, 3, 0], np.uint8)
    mat = u.simple_mat(5, 2, 4, -1)
    mp = mat.ctypes.data_as(_i8p)
    ins = dict(score=-14, qb=0, qe=4, tb=0, te=-1, n_cigar=1, cigar=[5 << 4 | 1])
    hang = dict(score=0, qb=5, qe=4, tb=0, te=-1, n_cigar=0, cigar=[])
    F = lambda got: [{f: g[f] for f in a.FIELDS} for g in got]
    a.launches(sim, reset=True)
    for costs in ((4, 2), (4, 2, 24, 1)):
        for ends in range(4):
            want = [RESET, hang if ends & 1 else ins, RESET]
            assert F(a.call(sim, [e, q, e], [q, e, e], mat, costs, ends, 5)) == want, (costs, ends)
            assert F(a.call_flat(sim, lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, costs, ends, 5)) == want
            assert F(a.call(sim, [e, q, e], [q, e, e], mat, costs, ends, 5, a.SCORE_ONLY)) == [RESET, dict(want[1], n_cigar=0, cigar=[]), RESET]
            a.assert_same(a.call(sim, [e, q, e], [q, e, e], mat, costs, ends, 5), a.expected([e, q, e], [q, e, e], mat, costs, ends, 5))
        assert a.call(sim, [], [], mat, costs, 3, 5) == []
    assert {f: sim.ov_align(q, e, mat, 4, 2, 1)[f] for f in a.FIELDS} == hang
    assert {f: sim.ov_align(q, e, mat, 4, 2, 2)[f] for f in a.FIELDS} == ins
    # bad arguments: m, mat, the costs, ends, flag, the arrays, m = 1 for the two-piece entries, a code >= m, the range
    rng = np.random.default_rng(9)
    qs, ts = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = sim.local_pairs(qs, ts)
    aln = (ksw2_amd.LocalAln * 6)()
    L = sim.lib
    ar = lf.arena(qs, ts, lead=1, gap=2)
    f, n, keep2 = sim._local_flat(*ar, None)
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, -1)):
        assert L.ksw2amd_ov_align_batch(None, *args, 3, 0, 6, pairs, aln) == E_PARAM, args
        assert L.ksw2amd_ov_align_batch_flat(None, *args, 3, 0, 6, ctypes.byref(f), aln) == E_PARAM, args
        assert L.ksw2amd_ovd_align_batch(None, *args, 24, 1, 3, 0, 6, pairs, aln) == E_PARAM, args
    assert L.ksw2amd_ovd_align_batch(None, 5, mp, 4, 2, 128, 1, 3, 0, 6, pairs, aln) == E_PARAM
    for ends in (4, 8, -1, 7):
        assert L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, ends, 0, 6, pairs, aln) == E_PARAM and "ends must be" in sim.last_error()
        assert L.ksw2amd_ov_align_batch_flat(None, 5, mp, 4, 2, ends, 0, 6, ctypes.byref(f), aln) == E_PARAM
        assert L.ksw2amd_ovd_align_batch(None, 5, mp, 4, 2, 24, 1, ends, 0, 6, pairs, aln) == E_PARAM
        assert L.ksw2amd_ovd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, ends, 0, 6, ctypes.byref(f), aln) == E_PARAM
    for flag in (0x04, 0x08, 0x10, 0x40, 0x100):
        assert L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, flag, 6, pairs, aln) == E_PARAM and "flag accepts" in sim.last_error()
        assert L.ksw2amd_ovd_align_batch_flat(None, 5, mp, 4, 2, 24, 1, 3, flag, 6, ctypes.byref(f), aln) == E_PARAM
    assert L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, 0, 6, None, aln) == E_PARAM and L.ksw2amd_ov_align_batch(None, 5, mp, 4, 2, 3, 0, 6, pairs, None) == E_PARAM
    assert L.ksw2amd_ov_align_batch_flat(None, 5, mp, 4, 2, 3, 0, 6, ctypes.byref(f), None) == E_PARAM
    one = np.zeros(1, np.int8)
    z = [np.zeros(4, np.uint8)]
    p1, k1 = sim.local_pairs(z, z)
    assert L.ksw2amd_ovd_align_batch(None, 1, one.ctypes.data_as(_i8p), 4, 2, 24, 1, 3, 0, 1, p1, aln) == E_PARAM and "m >= 2" in sim.last_error()
    assert L.ksw2amd_ov_align_batch(None, 1, one.ctypes.data_as(_i8p), 4, 2, 3, a.SCORE_ONLY, 1, p1, aln) == 0      # (the single-piece entry takes m = 1)
    a.launches(sim, reset=True)
    bad_t = [x.copy() for x in ts]
    bad_t[2][len(bad_t[2]) - 1] = 9
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        a.call(sim, qs, bad_t, mat, (4, 2), 3, 5)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    pairs[1].qlen = (0x3fffffff - 127 - 127) // (127 + 127) + 1
    assert L.ksw2amd_ov_align_batch(None, 5, big.ctypes.data_as(_i8p), 127, 127, 3, 0, 1, ctypes.byref(pairs[1]), aln) == E_PARAM and "0x3fffffff" in sim.last_error()
    pairs[1].qlen = len(qs[1])
    assert a.launches(sim)[:3] == (0, 0, 0)
    # the single-pair entries report like ksw_ll_i16: 0 with the reset values, the error counted
    before = sim.error_count()
    rec = ksw2_amd.LocalAln()
    rec.score = 5; rec.tb = 5
    tp = ts[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.ksw2amd_ov_align(None, None, 3, tp, 4, 2, 3, 0, ctypes.byref(rec)) == 0 and L.ksw2amd_ovd_align(None, None, 3, tp, 4, 2, 24, 1, 3, 0, ctypes.byref(rec)) == 0
    assert (rec.score, rec.qb, rec.qe, rec.tb, rec.te, rec.n_cigar) == (0, -1, -1, -1, -1, 0)
    assert sim.error_count() > before and "NULL profile" in sim.last_error()
    got = sim.ov_align(qs[0], ts[0], mat, 4, 2, 4)
    assert {k: got[k] for k in a.FIELDS} == RESET and "ends must be" in sim.last_error()


def test_chunked_flat_batches(sim):
    """KSW2AMD_LL_CHUNK_BYTES cuts the flat batch into several chunks: the same results, a start pass behind every forward launch; a bad
    code in a later chunk resets EVERY entry"""
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=40, m=5, qmax=90, tmax=200, long_targets=0)
    q[7], t[9] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    ar = lf.arena(q, t, lead=1, gap=1)
    os.environ["KSW2AMD_LL_CHUNK_BYTES"] = "2000"
    for costs in ((4, 2), (24, 1, 4, 2)):
        exp = a.expected(q, t, mat, costs, 3, 5)
        a.launches(sim, reset=True)
        a.assert_same(a.call_flat(sim, ar, mat, costs, 3, 5), exp)
        n = a.launches(sim)
        assert n[3] > 3 and n[0] > 3 and n[1] == n[0] and n[2] == 0, n
    bad = ar[0].copy()
    bad[int(ar[3][30]) + 1] = 6
    aln = (ksw2_amd.LocalAln * 40)()
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
        a.call_flat(sim, (bad,) + tuple(ar[1:]), mat, (4, 2), 3, 5, aln=aln)
    assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)


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


@pytest.mark.parametrize("mode", ["", "pool", "dual"])
def test_c_caller(simso, tmp_path, mode):
    exe = str(tmp_path / "ova_caller")
    libdir = os.path.dirname(simso)
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "ova_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = o.ragged_batch(rng, n=12, m=5, qmax=80, tmax=150, long_targets=0)
    q.append(np.zeros(0, np.uint8)); t.append(t[0])
    q.append(q[0]); t.append(np.zeros(0, np.uint8))
    costs = (4, 2, 24, 1) if mode == "dual" else (4, 2)
    for ends, flag in ((3, 0), (1, a.RIGHT | a.REV_CIGAR)):
        inp = str(tmp_path / "pairs.txt")
        a.write_input(inp, q, t, mat, 5, costs, ends, flag)
        out = subprocess.run([exe, inp] + ([mode] if mode else []), check=True, capture_output=True, text=True).stdout
        batch, single, reallocs = la.parse_caller(out)
        exp = a.expected(q, t, mat, costs, ends, 5, flag)
        a.assert_same(batch, exp, "batch")
        a.assert_same(single, exp, "single")
        assert (reallocs is not None and reallocs > len(q)) if mode == "pool" else reallocs is None


def test_only_the_new_host_object_names_the_start_pass_launchers(tmp_path):
    """the other tests' simulator builds link the other host objects without k2a_shim_launch_ov_rev / _ovd_rev and load with immediate binding"""
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    for src in sorted(os.listdir(csrc)):
        if not re.fullmatch(r"ksw2_host_\w+\.c", src):
            continue
        obj = str(tmp_path / (src[:-2] + ".o"))
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, src), "-o", obj], check=True)
        undefined = subprocess.run(["nm", "-u", obj], check=True, capture_output=True, text=True).stdout
        for name in ("k2a_shim_launch_ov_rev", "k2a_shim_launch_ovd_rev"):
            assert (name in undefined) == (src == "ksw2_host_ova.c"), (src, name)
