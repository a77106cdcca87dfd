"""CPU: semi-global alignment with the start of the interval and a CIGAR (ksw2amd_sg_align_batch / ksw2amd_sg_align_batch_flat /
ksw2amd_sg_align; include/ksw2_amd.h).  The contract's tb (tests/sga_oracle.c) is pinned to the compiled reference's
scalar ksw_extz through tests/golden/sga_cases.npz and to a brute-force statement of "the largest x with G(x) == score"; the product's host
code and lane code (K2aLaneLL<.., REV = true, .., FIT = true>, both number formats and both score lookups) run on a test-local lock-step
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i8p = ctypes.POINTER(ctypes.c_int8)
COSTS = ((4, 2), (0, 1), (6, 1), (0, 0))
NAMES = ("ksw2amd_sg_align_batch", "ksw2amd_sg_align_batch_flat", "ksw2amd_sg_align")
RESET = dict(score=0, qb=-1, qe=-1, tb=-1, te=-1, n_cigar=0, cigar=[])


@pytest.fixture(scope="module")
def simso(tmp_path_factory):
    return a.sim_library(str(tmp_path_factory.mktemp("sgasim") / "libksw2_amd.so"))


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


def _both(lib, q, t, mat, gapo, gape, m, flag=0, exp=None, msg=""):
    """ksw2amd_sg_align_batch and ksw2amd_sg_align_batch_flat (host arena, bytes that no matrix admits between the sequences) against the
    contract; score, qe, te are ksw2amd_sg_batch's bit for bit"""
    exp = a.expected(q, t, mat, gapo, gape, m, flag) if exp is None else exp
    a.assert_same(lib.sg_align_batch(list(q), list(t), mat, gapo, gape, flag=flag, m=m), exp, str(msg))
    a.assert_same(lib.sg_align_batch_flat(*lf.arena(q, t, lead=3, gap=2), mat, gapo, gape, flag=flag, m=m), exp, str((msg, "flat")))
    fwd = lib.sg_batch(list(q), list(t), mat, gapo, gape, m=m)
    assert [(e["score"], e["qe"], e["te"]) for e in exp] == [tuple(int(x) for x in r) for r in fwd], msg
    return exp


def _raw(lib, q, t, mat, gapo, gape, flag, aln, m=5):
    pairs, keep = lib.local_pairs(q, t)
    return lib.lib.ksw2amd_sg_align_batch(None, m, mat.ctypes.data_as(_i8p), gapo, gape, flag, len(q), pairs, aln), keep


# ---------------------------------------------------------------- the oracle itself

def test_oracle_equals_the_golden_file_of_the_compiled_reference():
    total = empty = 0
    for name, m, mat, gapo, gape, q, t, cells, cig in a.load_golden():
        np.testing.assert_array_equal(a.oracle_cells(q, t, mat, gapo, gape, m), cells, name)
        total += len(q)
        empty += int((cells[:, 3] == cells[:, 4] + 1).sum())
    assert total == 324 and empty >= 10


def test_golden_file_is_no_larger_than_its_cigars():
    """data only: names, tb and three CIGAR arrays per group, inputs and scores stay in sg_cases.npz"""
    z = np.load(a.GOLDEN)
    assert all(re.fullmatch(r"ngroups|g\d+_(name|tb|ncig\d+|cig\d+)", k) for k in z.files), z.files
    assert os.path.getsize(a.GOLDEN) < 1 << 20


def test_oracle_is_the_largest_start_by_brute_force(sim):
    """tests/sga_oracle.c against G(x) for EVERY x by a global matrix of its own in plain Python, gapo / gape including 0, matrices
    without a positive entry, homopolymers (every row ties); the library (simulator build, biased and clamped values) returns the same."""
    rng = np.random.default_rng(5)
    seen_empty = seen_tie = 0
    for ci, (gapo, gape) in enumerate(((4, 2), (0, 1), (3, 0), (0, 0), (2, 1), (1, 0), (5, 0))):
        for m, mat in ((3, np.array([2, -3, -1, -3, 2, -2, -1, -2, 1], np.int8)), (4, u.random_mat(rng, 4, -6, 1)), (2, u.random_mat(rng, 2))):
            qs, ts = [], []
            for k in range(36):
                al = 1 if k % 5 == 0 else m
                q = rng.integers(0, al, int(rng.integers(1, 8)), dtype=np.uint8)
                t = rng.integers(0, al, int(rng.integers(1, 23)), dtype=np.uint8)
                if k % 4 == 0:
                    t = np.concatenate([t[:5], q, t[5:]]).astype(np.uint8)
                qs.append(q); ts.append(t)
            exp = np.array([a.brute(q, t, mat, gapo, gape, m) for q, t in zip(qs, ts)], dtype=np.int32)
            np.testing.assert_array_equal(a.oracle_cells(qs, ts, mat, gapo, gape, m), exp, str((gapo, gape, m)))
            seen_empty += int((exp[:, 3] == exp[:, 4] + 1).sum())
            for q, t, e in zip(qs[:6], ts[:6], exp[:6]):                     # ties: more than one x reaches the score
                G = [la.brute_global(q, t[x:e[4] + 1], mat, m, gapo, gape) for x in range(e[4] + 1)]
                seen_tie += sum(g == e[0] for g in G) > 1
            os.environ["KSW2AMD_LL_FORM"] = str(ci % 3)
            got = sim.sg_align_batch(qs, ts, mat, gapo, gape, flag=a.SCORE_ONLY, m=m)
            assert [[g[f] for f in ("score", "qb", "qe", "tb", "te")] for g in got] == exp.tolist(), (gapo, gape, m)
    assert seen_empty > 50 and seen_tie > 5


# ---------------------------------------------------------------- the library on the simulator

@pytest.mark.parametrize("form", ["0", "1", "2"])
@pytest.mark.parametrize("lds", ["0", "1"])
def test_ragged_batch_every_form(sim, form, lds):
    rng = np.random.default_rng(11 + int(form))
    os.environ["KSW2AMD_LL_FORM"] = form
    os.environ["KSW2AMD_LL_LDS"] = lds
    for m, mat in ((5, u.simple_mat(5, 2, 4, -1)), (20, _m20(rng)), (4, u.random_mat(rng, 4, -6, 1))):
        q, t = u.ragged(rng, 20, m, 1, 90, related=0.6)
        t = [np.concatenate([rng.integers(0, m, int(rng.integers(0, 120)), dtype=np.uint8), x, rng.integers(0, m, int(rng.integers(0, 80)), dtype=np.uint8)]) for x in t]
        q += [q[0], q[0], q[1]]
        t += [t[0], t[0][::-1].copy(), t[1]]                               # same-shape partners for form 1
        t[3] = np.concatenate([rng.integers(0, m, 1100, dtype=np.uint8), q[3]])    # two generations in the reversed pass as well
        t[4] = np.concatenate([q[4], rng.integers(0, m, 1030, dtype=np.uint8)])
        for gapo, gape in COSTS:
            _both(sim, q, t, mat, gapo, gape, m, msg=(form, lds, m, gapo, gape))


@pytest.mark.parametrize("form", ["0", "2"])
def test_golden_file_on_the_simulator(sim, form):
    os.environ["KSW2AMD_LL_FORM"] = form
    for name, m, mat, gapo, gape, q, t, cells, cig in a.load_golden():
        for fl in a.FLAGS if form == "0" else (0,):
            got = sim.sg_align_batch(q, t, mat, gapo, gape, flag=fl, m=m)
            assert [[g[f] for f in ("score", "qb", "qe", "tb", "te")] for g in got] == cells.tolist(), (name, fl)
            assert [g["cigar"] for g in got] == cig[fl], (name, fl)


@pytest.mark.parametrize("form", ["0", "2"])
def test_edge_grid(sim, form):
    """qlen 1 .. 1 025 in targets of 17 / 1 025 / 2 049, a lightly mutated copy of the query ending at te in {qlen - 1, 15, 16, 1 023,
    1 024, tlen - 1}: rl = te + 1 and the interval's length sit on either side of a lane and of a generation"""
    rng = np.random.default_rng(77)
    os.environ["KSW2AMD_LL_FORM"] = form
    cases = [c for c in a.edge_cases() if form == "0" or c[1] <= 65]       # (the packed form of the long queries: test_uneven_halves)
    qs, ts = a.edge_grid(rng, 5, cases)
    exp = _both(sim, qs, ts, s.unit_mat(5), 4, 2, 5, flag=a.SCORE_ONLY, msg=form)
    lens, ends = set(), set()
    for (tl, ql, te), e in zip(cases, exp):
        assert e["te"] == te and ql - 2 <= te - e["tb"] + 1 <= ql, (tl, ql, te, e)
        lens.add(te - e["tb"] + 1); ends.add(te)
    assert {15, 16, 1023, 1024, 2048} <= ends and {1, 15, 16, 17, 63, 64, 65} <= lens
    assert form != "0" or {1023, 1024, 1025} <= lens


@pytest.mark.parametrize("order", [0, 1])
def test_uneven_halves_of_a_packed_task(sim, order, capfd):
    """two pairs of one shape whose copies end at rows 45 and 2 090, in both orders, and an empty interval beside a long one: one packed
    task over the bounding rectangle, each half with its own rows"""
    rng = np.random.default_rng(31 + order)
    os.environ["KSW2AMD_LL_FORM"] = "1"
    os.environ["KSW2AMD_TRACE"] = "1"
    mat = s.unit_mat(5)
    for ql in (40, 1030):
        qs, ts = a.uneven_halves(rng, 5, 2100, ql, (ql + 5, 2090))
        if order:
            qs, ts = qs[::-1], ts[::-1]
        capfd.readouterr()
        exp = _both(sim, qs, ts, mat, 4, 2, 5, msg=(order, ql))
        err = capfd.readouterr().err
        assert "sga: pairs=2 pk_tasks=1 int32_tasks=0" in err and "sga-rev: pk_tasks=1 int32_tasks=0" in err, err
        assert sorted(e["te"] for e in exp) == [ql + 5, 2090] and all(e["te"] - e["tb"] + 1 == ql for e in exp)
    # the whole query inserted (no letter in common, 40 mismatches cost more than one gap) beside a copy that ends in row 2 090
    q1, t1 = a.planted_copy(rng, 5, 2100, 40, 2090)
    q2, t2 = rng.integers(2, 4, 40, dtype=np.uint8), rng.integers(0, 2, 2100, dtype=np.uint8)
    qs, ts = ([q1, q2], [t1, t2]) if order == 0 else ([q2, q1], [t2, t1])
    capfd.readouterr()
    exp = _both(sim, qs, ts, mat, 4, 2, 5, msg=("empty", order))
    assert "sga: pairs=2 pk_tasks=1" in capfd.readouterr().err
    e = exp[1 - order]
    assert (e["score"], e["tb"], e["te"], e["cigar"]) == (-84, 1, 0, [40 << 4 | 1])


def test_admission_bound(sim, capfd):
    """smax = 127, costs (5, 1): B + (qlen + 1) * smax = 128 qlen + 132 <= 65 535 up to qlen 510, the same bound for the start pass"""
    os.environ["KSW2AMD_LL_FORM"] = "2"
    os.environ["KSW2AMD_TRACE"] = "1"
    rng = np.random.default_rng(3)
    mat = np.full((4, 4), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    for ql, packed in ((510, True), (511, False)):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), q, rng.integers(0, 4, 9, dtype=np.uint8)])
        capfd.readouterr()
        got = sim.sg_align_batch([q], [t], mat, 5, 1, m=4)
        err = capfd.readouterr().err
        assert (got[0]["score"], got[0]["tb"], got[0]["te"], got[0]["cigar"]) == (127 * ql, 20, 20 + ql - 1, [ql << 4])
        a.assert_same(got, a.expected([q], [t], mat, 5, 1, 4))
        assert ("sga: pairs=1 pk_tasks=%d int32_tasks=%d" % ((1, 0) if packed else (0, 1))) in err, err
        assert ("sga-rev: pk_tasks=%d int32_tasks=%d" % ((1, 0) if packed else (0, 1))) in err, err


def test_negative_optima_free_gaps_and_scores_beyond_16_bits(sim):
    rng = np.random.default_rng(4)
    os.environ["KSW2AMD_LL_FORM"] = "2"
    q = rng.integers(0, 4, 1700, dtype=np.uint8)
    t = np.concatenate([rng.integers(0, 4, 30, dtype=np.uint8), q, rng.integers(0, 4, 11, dtype=np.uint8)])
    exp = _both(sim, [q], [t], u.simple_mat(4, 40, 30), 4, 2, 4)
    assert exp[0]["score"] == 40 * 1700 > 65535 and (exp[0]["tb"], exp[0]["te"]) == (30, 1729)
    # an unrelated pair under +1 / -100 with dear gaps: strongly negative, a real interval
    q, t = np.zeros(40, np.uint8), np.ones(300, np.uint8)
    exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), 120, 110, 4)
    assert exp[0]["score"] < -100 and exp[0]["tb"] <= exp[0]["te"]
    # inserting the whole query is best: te = 0, tb = 1, qlen I
    exp = _both(sim, [q], [t], u.simple_mat(4, 1, 100), 2, 1, 4)
    assert (exp[0]["score"], exp[0]["tb"], exp[0]["te"], exp[0]["cigar"]) == (-42, 1, 0, [40 << 4 | 1])
    # matrices without a positive entry; free gaps (0, 0): every row ties, the shortest interval is the answer
    for mat, gapo, gape in ((u.random_mat(rng, 5, -7, 1), 3, 1), (u.random_mat(rng, 5, -7, 1), 0, 0), (u.simple_mat(5, 2, 4, -1), 0, 0)):
        qs, ts = u.ragged(rng, 12, 5, 1, 60)
        _both(sim, qs, ts, mat, gapo, gape, 5, msg=(gapo, gape))


def test_all_three_flags(sim):
    rng = np.random.default_rng(6)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 16, 5, 20, 120, related=1.0)
    t = [np.concatenate([rng.integers(0, 5, 40, dtype=np.uint8), x]) for x in t]
    q.append(np.array([0, 0, 1, 1], np.uint8)); t.append(np.array([0, 0, 0, 1, 1], np.uint8))      # left / right placement of a gap differs
    cig = {}
    for fl in (0, a.RIGHT, a.REV_CIGAR, a.RIGHT | a.REV_CIGAR):
        cig[fl] = [e["cigar"] for e in _both(sim, q, t, mat, 4, 2, 5, flag=fl, msg=fl)]
    assert cig[0] != cig[a.RIGHT] and cig[a.REV_CIGAR] == [c[::-1] for c in cig[0]]
    for e, qq, tt in zip(a.expected(q, t, mat, 4, 2, 5), q, t):
        assert la.rescore(e["cigar"], qq, tt[e["tb"]:e["te"] + 1], mat, 5, 4, 2) == (e["score"], len(qq), e["te"] - e["tb"] + 1)
    got = sim.sg_align_batch(q, t, mat, 4, 2, flag=a.SCORE_ONLY)
    assert all(g["n_cigar"] == 0 for g in got)


def test_corner_results_launch_nothing(sim):
    e = np.zeros(0, np.uint8)
    q = np.array([0, 1, 2, 3, 0], np.uint8)
    mat = u.simple_mat(5, 2, 4, -1)
    ins = dict(score=-14, qb=0, qe=4, tb=0, te=-1, n_cigar=1, cigar=[5 << 4 | 1])
    a.launches(sim, reset=True)
    got = sim.sg_align_batch([e, q, e], [q, e, e], mat, 4, 2, m=5)
    assert [{f: g[f] for f in a.FIELDS} for g in got] == [RESET, ins, RESET]
    a.assert_same(got, a.expected([e, q, e], [q, e, e], mat, 4, 2, 5))
    got = sim.sg_align_batch_flat(*lf.arena([e, q, e], [q, e, e], lead=2, gap=1), mat, 4, 2, m=5)
    assert [{f: g[f] for f in a.FIELDS} for g in got] == [RESET, ins, RESET]
    got = sim.sg_align_batch([e, q, e], [q, e, e], mat, 4, 2, flag=a.SCORE_ONLY, m=5)
    assert [{f: g[f] for f in a.FIELDS} for g in got] == [RESET, dict(ins, n_cigar=0, cigar=[]), RESET]
    assert a.launches(sim)[:3] == (0, 0, 0)
    assert sim.sg_align_batch([], [], mat, 4, 2, m=5) == []
    # corners beside a real pair; the single-pair entry
    got = sim.sg_align_batch([q, e, q], [e, q, q], mat, 4, 2, m=5)
    assert {f: got[0][f] for f in a.FIELDS} == ins and {f: got[1][f] for f in a.FIELDS} == RESET
    assert {f: got[2][f] for f in a.FIELDS} == dict(score=10, qb=0, qe=4, tb=0, te=4, n_cigar=1, cigar=[5 << 4])
    assert {f: sim.sg_align(q, e, mat, 4, 2)[f] for f in a.FIELDS} == ins
    assert {f: sim.sg_align(e, q, mat, 4, 2)[f] for f in a.FIELDS} == RESET
    assert sim.sg_align(q, q, mat, 4, 2)["cigar"] == [5 << 4]


def test_cigar_buffer_reuse(sim):
    """a second call into the same records must not reallocate a buffer that is large enough; SCORE_ONLY leaves the buffers alone"""
    rng = np.random.default_rng(41)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 40, 200, related=1.0)
    q[3], t[3] = np.full(9, 2, np.uint8), np.full(50, 1, np.uint8)          # an empty interval among them: qlen I from the host
    exp = a.expected(q, t, mat, 4, 2, 5)
    assert exp[3]["cigar"] == [9 << 4 | 1]
    aln = (ksw2_amd.LocalAln * len(q))()
    rc, _ = _raw(sim, q, t, mat, 4, 2, 0, aln)
    assert rc == 0
    first = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    assert all(p and mc >= x.n_cigar > 0 for (p, mc), x in zip(first, aln))
    rc, _ = _raw(sim, q[::-1], t[::-1], mat, 4, 2, 0, aln)                   # other alignments into the same buffers
    assert rc == 0
    for k, x in enumerate(aln):
        e = exp[len(q) - 1 - k]
        assert [int(x.cigar[j]) for j in range(x.n_cigar)] == e["cigar"] and x.score == e["score"]
        if x.n_cigar <= first[k][1]:
            assert (ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) == first[k]
    second = [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln]
    rc, _ = _raw(sim, q[::-1], t[::-1], mat, 4, 2, a.SCORE_ONLY, aln)
    assert rc == 0 and all(x.n_cigar == 0 for x in aln)
    assert [(ctypes.cast(x.cigar, ctypes.c_void_p).value, x.m_cigar) for x in aln] == second
    for x in aln:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))


def test_bad_arguments(sim):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 6, 5, 5, 60)
    pairs, keep = sim.local_pairs(q, t)
    aln = (ksw2_amd.LocalAln * 6)()
    L = sim.lib
    mp = mat.ctypes.data_as(_i8p)
    ar = lf.arena(q, t, lead=1, gap=2)
    f, n, keep2 = sim._local_flat(*ar, None)
    E = ksw2_amd.KSW2AMD_E_PARAM if hasattr(ksw2_amd, "KSW2AMD_E_PARAM") else -2
    a.launches(sim, reset=True)
    for args in ((0, mp, 4, 2), (128, mp, 4, 2), (5, None, 4, 2), (5, mp, 128, 2), (5, mp, 4, 128), (5, mp, -1, 2), (5, mp, 4, -1)):
        assert L.ksw2amd_sg_align_batch(None, *args, 0, 6, pairs, aln) == E, args
        assert L.ksw2amd_sg_align_batch_flat(None, *args, 0, 6, ctypes.byref(f), aln) == E, args
    for flag in (0x04, 0x08, 0x10, 0x20, 0x40, 0x100, 0x03 | 0x400):           # anything but SCORE_ONLY / RIGHT / REV_CIGAR
        assert L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, flag, 6, pairs, aln) == E, flag
        assert L.ksw2amd_sg_align_batch_flat(None, 5, mp, 4, 2, flag, 6, ctypes.byref(f), aln) == E, flag
    assert "flag accepts" in sim.last_error()
    assert L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, 0, 6, None, aln) == E and L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, 0, 6, pairs, None) == E
    assert L.ksw2amd_sg_align_batch(None, 5, mp, 4, 2, 0, -1, pairs, aln) == E
    assert L.ksw2amd_sg_align_batch_flat(None, 5, mp, 4, 2, 0, 6, None, aln) == E and L.ksw2amd_sg_align_batch_flat(None, 5, mp, 4, 2, 0, 6, ctypes.byref(f), None) == E
    # a code >= m: named by the pointer entry before anything runs, caught on the "device" by the flat entry with the lowest pair named
    bad_t = [x.copy() for x in t]
    bad_t[4][3] = 5
    bad_t[2][len(bad_t[2]) - 1] = 9
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        sim.sg_align_batch(q, bad_t, mat, 4, 2, m=5)
    keepaln = (ksw2_amd.LocalAln * 6)()
    for x in keepaln:
        x.score = 7; x.qb = x.qe = x.tb = x.te = 7; x.n_cigar = 0
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 2: residue code >= m"):
        sim.sg_align_batch_flat(*lf.arena(q, bad_t, lead=1, gap=2), mat, 4, 2, m=5, aln=keepaln)
    assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in keepaln)
    # the range limit: gapo + qlen * (gape + smax) + smax > 0x3fffffff (only the length is looked at before the rejection)
    big = np.full((5, 5), 127, np.int8).reshape(-1)
    ql = (0x3fffffff - 127 - 127) // (127 + 127) + 1
    pairs[1].qlen = ql
    assert L.ksw2amd_sg_align_batch(None, 5, big.ctypes.data_as(_i8p), 127, 127, 0, 1, ctypes.byref(pairs[1]), aln) == E
    assert "0x3fffffff" in sim.last_error()
    pairs[1].qlen = len(q[1])
    ql_arr = ar[2].copy()
    ql_arr[3] = ql
    f2, _, keep3 = sim._local_flat(ar[0], ar[1], ql_arr, ar[3], ar[4], None)
    assert L.ksw2amd_sg_align_batch_flat(None, 5, big.ctypes.data_as(_i8p), 127, 127, 0, 6, ctypes.byref(f2), aln) == E
    assert "pair 3" in sim.last_error()
    assert a.launches(sim)[:3] == (0, 0, 0)                                 # nothing of all this launched an alignment kernel
    # ksw2amd_sg_align reports like ksw_ll_i16: 0 with the reset values, the error counted
    before = sim.error_count()
    one = ksw2_amd.LocalAln()
    one.score = 5; one.tb = 5
    assert L.ksw2amd_sg_align(None, None, 3, t[0].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 2, 0, ctypes.byref(one)) == 0
    assert (one.score, one.qb, one.qe, one.tb, one.te, one.n_cigar) == (0, -1, -1, -1, -1, 0)
    assert sim.error_count() > before and "NULL profile" in sim.last_error()
    d = sim.sg_align(q[0], t[0], mat, 200, 2)
    assert {k: d[k] for k in a.FIELDS} == RESET and "gapo and gape" in sim.last_error()


def test_chunked_flat_batches(sim):
    """KSW2AMD_LL_CHUNK_BYTES cuts the flat batch into several chunks: the same results; a bad code in a later chunk resets EVERY entry"""
    rng = np.random.default_rng(13)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 40, 5, 10, 200)
    q[7], t[9] = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    exp = a.expected(q, t, mat, 4, 2, 5)
    ar = lf.arena(q, t, lead=1, gap=1)
    os.environ["KSW2AMD_LL_CHUNK_BYTES"] = "4000"
    a.launches(sim, reset=True)
    a.assert_same(sim.sg_align_batch_flat(*ar, mat, 4, 2, m=5), exp)
    n = a.launches(sim)
    assert n[3] > 3 and n[0] > 3 and n[1] == n[0] and n[2] == 0              # a start pass behind every forward launch, no local twin
    bad = ar[0].copy()
    bad[int(ar[3][30]) + 1] = 6
    aln = (ksw2_amd.LocalAln * 40)()
    with pytest.raises(ksw2_amd.Ksw2Error, match=r"pair 30: residue code >= m"):
        sim.sg_align_batch_flat(bad, *ar[1:], mat, 4, 2, m=5, aln=aln)
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


@pytest.mark.parametrize("pool", [False, True])
def test_c_caller_with_and_without_pool(simso, tmp_path, pool):
    exe = str(tmp_path / "sga_caller")
    libdir = os.path.dirname(simso)
    subprocess.run(["gcc", "-O1", "-Wall", "-Wextra", "-rdynamic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "sga_caller.c"), "-L" + libdir, "-lksw2_amd", "-Wl,-rpath," + libdir], check=True)
    rng = np.random.default_rng(21)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 12, 5, 1, 80, related=0.8)
    t = [np.concatenate([rng.integers(0, 5, 100, dtype=np.uint8), x, rng.integers(0, 5, 200, dtype=np.uint8)]) for x in t]
    q.append(np.zeros(0, np.uint8)); t.append(t[0])
    q.append(q[0]); t.append(np.zeros(0, np.uint8))
    q.append(np.full(6, 2, np.uint8)); t.append(np.full(30, 1, np.uint8))    # an empty interval
    for flag in (0, a.RIGHT | a.REV_CIGAR):
        inp = str(tmp_path / "pairs.txt")
        la.write_input(inp, q, t, mat, 5, 4, 2, flag)
        out = subprocess.run([exe, inp] + (["pool"] if pool else []), check=True, capture_output=True, text=True).stdout
        batch, single, reallocs = la.parse_caller(out)
        exp = a.expected(q, t, mat, 4, 2, 5, flag)
        a.assert_same(batch, exp, "batch")
        a.assert_same(single, exp, "single")
        assert (reallocs is not None and reallocs > len(q)) if pool else reallocs is None


def test_only_the_new_host_object_names_the_start_pass_launcher(tmp_path):
    """ksw2_host_sg.o, ksw2_host_ll.o, ksw2_host_llf.o and ksw2_host_lla.o are linked by the other tests' simulator builds, which have
    no k2a_shim_launch_sg_rev and load with immediate binding"""
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    for src in sorted(os.listdir(csrc)):
        if not re.fullmatch(r"ksw2_host_\w+\.c", src):
            continue
        o = str(tmp_path / (src[:-2] + ".o"))
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, src), "-o", o], check=True)
        undefined = subprocess.run(["nm", "-u", o], check=True, capture_output=True, text=True).stdout
        assert ("k2a_shim_launch_sg_rev" in undefined) == (src == "ksw2_host_sga.c"), (src, undefined)
