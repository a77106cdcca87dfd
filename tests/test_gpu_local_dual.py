"""GPU: local alignment under the two-piece gap cost (ksw2amd_lld_batch / ksw2amd_lld_align_batch and their flat forms) on libksw2_amd.so
against the contract's formula (tests/lld_util.py: tests/lld_oracle.c forward and on the reversed prefixes, then the project's
restatement of the scalar ksw_extd on the interval) and against tests/golden/lld_cases.npz, which the compiled reference produced.
The shapes are the smallest at which the second piece's state can go wrong: the lane hand-over of E2 (rows 15 / 16 / 17 / 33), its
way through the generation boundary in HBM (rows 1 024 / 1 025 / 2 049), gaps at the crossover of the two pieces, the packed admission
limit, packed halves that end in different cells.  Each runs in the packed and the int32 form inside a decoy batch, m = 5 and 20."""
import contextlib
import os
import re

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_util as u
from tests import lla_util as la
from tests import llf_util as lf
from tests import lld_util as d

pytestmark = pytest.mark.gpu
FORMS = [("2", 5), ("0", 5), ("2", 20), ("0", 20)]          # (KSW2AMD_LL_FORM: 2 = packed for every admissible pair, 0 = int32 only), m


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for k in ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")


@contextlib.contextmanager
def device_arena(lib, base):
    p = lib.device_copy(base)
    try:
        yield p
    finally:
        lib.device_free(p)


def _m20(rng):
    mat = u.random_mat(rng, 20, -6, 0).reshape(20, 20)
    np.fill_diagonal(mat, 3)
    return mat.reshape(-1)


def _mat(rng, m):
    return u.simple_mat(5, 2, 4, -1) if m == 5 else _m20(rng)


def _decoyed(rng, m, q, t, letters=None):
    """the case's pairs with unrelated pairs in front of and behind them -> (queries, targets, slice of the case)"""
    a, b = d.decoy(rng, letters or m, 5)
    c, e = d.decoy(rng, letters or m, 4)
    return a + list(q) + c, b + list(t) + e, slice(len(a), len(a) + len(q))


def _check(lib, q, t, mat, costs, m, capfd, form=None, flat=True, flag=0, exp=None, msg=""):
    """all of the pairs against the formula through ksw2amd_lld_batch and ksw2amd_lld_align_batch (flat: the two flat entries from a host
    arena as well); returns the aligned records and the trace"""
    exp = d.expected(q, t, mat, costs, m, flag) if exp is None else exp
    fwd = np.array([[e["score"], e["qe"], e["te"]] for e in exp], dtype=np.int32).reshape(-1, 3)
    capfd.readouterr()
    np.testing.assert_array_equal(lib.lld_batch(q, t, mat, *costs, m=m), fwd, str(msg))
    got = lib.lld_align_batch(q, t, mat, *costs, flag=flag, m=m)
    err = capfd.readouterr().err
    d.assert_same(got, exp, msg)
    if flat:
        a = lf.arena(q, t, lead=3, gap=2)
        np.testing.assert_array_equal(lib.lld_batch_flat(*a, mat, *costs, m=m), fwd, str(msg))
        d.assert_same(lib.lld_align_batch_flat(*a, mat, *costs, flag=flag, m=m), exp, (msg, "flat"))
    if form is not None:
        line = re.search(r"lld-rev: pk_tasks=(\d+) int32_tasks=(\d+)", err)
        assert line, err
        assert (int(line.group(1)) == 0) if form == "0" else (int(line.group(1)) > 0), (form, err)
    return got, err


@pytest.mark.parametrize("form,m", FORMS)
def test_lane_handover_and_generation_boundary(lib, monkeypatch, capfd, form, m):
    """E2 from lane to lane (rows 15 / 16 / 17 / 33) and through the 16-byte boundary entries in HBM (rows 1 024 / 1 025 / 2 049), against
    columns 1, 2, 63, 64, 65 and 300, with rows = target and with qlen > tlen; two cost pairs under which both pieces are used"""
    rng = np.random.default_rng(500 + m)
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = _mat(rng, m)
    q1, t1 = d.shape_grid(rng, m, (15, 16, 17, 33), (1, 2, 15, 17))
    q2, t2 = d.shape_grid(rng, m, (1024, 1025, 2049), (1, 2, 63, 64, 65, 300))
    q, t, _ = _decoyed(rng, m, q1 + q2, t1 + t2)
    for costs in ((4, 2, 5, 1), (1, 3, 6, 1)):
        _check(lib, q, t, mat, costs, m, capfd, form, msg=(form, m, costs))


@pytest.mark.parametrize("form,m", FORMS)
def test_crossover_of_the_two_pieces(lib, monkeypatch, capfd, form, m):
    """planted gaps of 19, 20, 21 and 60 under (4, 2, 24, 1), crossover at l = 20: across rows 15 -> 16, rows 1 023 -> 1 024 and from
    column 0, in the query and in the target.  Above the crossover the scores differ from ksw2amd_ll_batch's with (4, 2)"""
    rng = np.random.default_rng(600 + m)
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = d.cross_mat(m)
    cq, ct, lns = d.crossover_pairs(rng, m, big=True)
    q, t, sl = _decoyed(rng, m, cq, ct, letters=4)
    got, _ = _check(lib, q, t, mat, d.CROSS, m, capfd, form, msg=(form, m))
    single = lib.ll_batch(q, t, mat, 4, 2, m=m)[sl]
    for g, s, ln in zip(got[sl], single, lns):
        assert (g["score"] != int(s[0])) == (ln > 20), (ln, g["score"], s)
        assert g["score"] - int(s[0]) in ((0,) if ln <= 20 else (1,) if ln == 21 else (40, 16)), (ln, g["score"], s)
        assert any((c & 0xf) in (1, 2) and (c >> 4) == ln for c in g["cigar"]), (ln, g["cigar"])       # the planted gap is in the CIGAR


@pytest.mark.parametrize("form,m", FORMS)
@pytest.mark.parametrize("costs", [(6, 3, 2, 1), (0, 0, 0, 0), (127, 127, 127, 127)])
def test_other_cost_shapes(lib, monkeypatch, capfd, form, m, costs):
    """the second piece cheaper everywhere (gapo2 + gape2 < gapo + gape and gape2 < gape), all four costs 0, all four 127"""
    rng = np.random.default_rng(700 + m + sum(costs))
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = _mat(rng, m)
    q, t = u.ragged(rng, 40, m, 1, 260, related=0.7)
    q2, t2 = d.shape_grid(rng, m, (17, 1025), (16, 65))
    _check(lib, q + q2, t + t2, mat, costs, m, capfd, form, msg=(form, m, costs))


@pytest.mark.parametrize("m", [5, 20])
def test_packed_admission_limit(lib, monkeypatch, capfd, m):
    """smax = 127: (min(qlen, tlen) + 1) * smax = 65 532 <= 65 535 at length 515 (packed, best score 65 405), one above it at 516 (int32), and
    a score above 65 535 in int32"""
    rng = np.random.default_rng(800 + m)
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    mat = np.full((m, m), -127, np.int8)
    np.fill_diagonal(mat, 127)
    mat = mat.reshape(-1)
    qs, ts = [], []
    for ln in (515, 515, 516, 600):
        x = rng.integers(0, min(m, 4), ln, dtype=np.uint8)
        y = x.copy()
        if ln == 515 and qs:                 # the second 515: a gap in the middle (the saturating subtractions next to the top of the range)
            y = np.concatenate([x[:300], x[330:], rng.integers(0, min(m, 4), 30, dtype=np.uint8)])
        qs.append(x); ts.append(y)
    exp = d.expected(qs, ts, mat, (100, 20, 127, 5), m)
    assert exp[0]["score"] == 515 * 127 and exp[2]["score"] == 516 * 127 and exp[3]["score"] == 600 * 127 > 65535 and 517 * 127 > 65535 >= 516 * 127
    got, err = _check(lib, qs, ts, mat, (100, 20, 127, 5), m, capfd, exp=exp, msg=m)
    line = re.search(r"lld: pairs=4 pk_tasks=(\d+) int32_tasks=(\d+)", err)
    assert line and (int(line.group(1)), int(line.group(2))) == (1, 2), err      # the two 515s share a packed task; 516 and 600 run in int32


@pytest.mark.parametrize("form", ["1", "2"])
@pytest.mark.parametrize("m", [5, 20])
def test_packed_halves_with_different_cells(lib, monkeypatch, capfd, form, m):
    """same-shape packed partners whose alignments end far apart, a half that scores 0 beside a positive one (the REV pass's bounding
    rectangle), cell (0, 0), full spans, tie-heavy tandem repeats (tests/lla_util.new_ground)"""
    rng = np.random.default_rng(900 + m)
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = _mat(rng, m)
    q, t = la.new_ground(rng, m)
    exp = d.expected(q, t, mat, (4, 2, 7, 1), m)
    assert exp[16]["score"] == 0 and exp[17]["score"] > 0 and (exp[18]["qe"], exp[18]["te"]) == (0, 0)
    _check(lib, q, t, mat, (4, 2, 7, 1), m, capfd, form, exp=exp, msg=(form, m))


@pytest.mark.parametrize("form", ["1", "0"])
def test_golden_file(lib, monkeypatch, form):
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    total = 0
    for name, m, mat, costs, q, t, exp in d.load_golden():
        d.assert_same(lib.lld_align_batch(q, t, mat, *costs, m=m), exp, name)
        a = lf.arena(q, t, lead=1, gap=3)
        d.assert_same(lib.lld_align_batch_flat(*a, mat, *costs, m=m), exp, name)
        total += len(q)
    assert total >= 150


_ragged = {}


def _ragged_case():
    """2 000 pairs of 30-1 500 and their expected records, computed once"""
    if not _ragged:
        rng = np.random.default_rng(1234)
        mat = u.simple_mat(5, 2, 4, -1)
        q, t = u.ragged(rng, 2000, 5, 30, 1500, related=0.3)
        _ragged.update(q=q, t=t, mat=mat, exp=d.expected(q, t, mat, d.CROSS, 5), arena=lf.arena(q, t, rng, lead=5, gap=4))
    return _ragged


@pytest.mark.parametrize("entry", ["batch", "align", "batch_flat", "align_flat"])
def test_ragged_batch(lib, entry):
    c = _ragged_case()
    q, t, mat, exp, a = c["q"], c["t"], c["mat"], c["exp"], c["arena"]
    fwd = np.array([[e["score"], e["qe"], e["te"]] for e in exp], dtype=np.int32)
    if entry == "batch":
        np.testing.assert_array_equal(lib.lld_batch(q, t, mat, *d.CROSS), fwd)
    elif entry == "align":
        d.assert_same(lib.lld_align_batch(q, t, mat, *d.CROSS), exp)
    elif entry == "batch_flat":
        np.testing.assert_array_equal(lib.lld_batch_flat(*a, mat, *d.CROSS), fwd, "host arena")
        with device_arena(lib, a[0]) as p:
            np.testing.assert_array_equal(lib.lld_batch_flat(*a, mat, *d.CROSS, device_base=p), fwd, "device arena")
    else:
        d.assert_same(lib.lld_align_batch_flat(*a, mat, *d.CROSS), exp, "host arena")
        with device_arena(lib, a[0]) as p:
            d.assert_same(lib.lld_align_batch_flat(*a, mat, *d.CROSS, device_base=p), exp, "device arena")


def test_flat_shared_query_and_bad_code(lib, capfd):
    rng = np.random.default_rng(77)
    mat = u.simple_mat(5, 2, 4, -1)
    qq = rng.integers(0, 5, 150, dtype=np.uint8)
    ts = [np.concatenate([rng.integers(0, 5, int(rng.integers(1, 200)), dtype=np.uint8), u.mutate(rng, qq, 5, 0.05, 0.1)]) for _ in range(64)]
    base, qo, ql, to, tl = lf.arena([qq], ts, lead=1, gap=3)
    n = len(ts)
    a = (base, np.repeat(qo, n), np.repeat(ql, n), to, tl)                  # ONE copy of the query in the arena
    exp = d.expected([qq] * n, ts, mat, d.CROSS, 5)
    fwd = np.array([[e["score"], e["qe"], e["te"]] for e in exp], dtype=np.int32)
    for dev in (False, True):
        with device_arena(lib, base) if dev else contextlib.nullcontext() as p:
            kw = dict(device_base=p) if dev else {}
            np.testing.assert_array_equal(lib.lld_batch_flat(*a, mat, *d.CROSS, **kw), fwd)
            d.assert_same(lib.lld_align_batch_flat(*a, mat, *d.CROSS, **kw), exp, dev)
    # a code >= m in pairs 9 and 40: the lowest is named, no alignment kernel runs on the chunk, every entry holds the reset values
    bad = base.copy()
    bad[int(to[40]) + 2] = 5
    bad[int(to[9]) + int(tl[9]) - 1] = 200
    for dev in (False, True):
        with device_arena(lib, bad) if dev else contextlib.nullcontext() as p:
            kw = dict(device_base=p) if dev else {}
            out = np.full((n, 3), 7, np.int32)
            capfd.readouterr()
            with pytest.raises(ka.Ksw2Error, match=r"pair 9: residue code >= m"):
                lib.lld_batch_flat(bad, *a[1:], mat, *d.CROSS, out=out, **kw)
            assert (out == np.array([0, -1, -1])).all()
            aln = (ka.LocalAln * n)()
            with pytest.raises(ka.Ksw2Error, match=r"pair 9: residue code >= m"):
                lib.lld_align_batch_flat(bad, *a[1:], mat, *d.CROSS, aln=aln, **kw)
            assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)
    with pytest.raises(ka.Ksw2Error, match=r"pair 9: residue code >= m"):
        lib.lld_batch([qq] * n, [bad[int(o):int(o) + int(l)] for o, l in zip(to, tl)], mat, *d.CROSS)


def test_flags(lib, capfd):
    """KSW_EZ_SCORE_ONLY, KSW_EZ_RIGHT, KSW_EZ_REV_CIGAR against the project's restatement of the scalar ksw_extd"""
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    costs = (4, 2, 8, 1)
    q, t = u.ragged(rng, 50, 5, 1, 300, related=0.8)
    q += [np.tile(np.array([0, 1], np.uint8), 30)] * 4                       # gaps whose placement RIGHT changes
    t += [np.concatenate([np.tile(np.array([0, 1], np.uint8), 20), [0, 0], np.tile(np.array([0, 1], np.uint8), 20)]).astype(np.uint8)] * 4
    base = d.expected(q, t, mat, costs, 5)
    differs = 0
    for flag in (0, d.RIGHT, d.REV_CIGAR, d.RIGHT | d.REV_CIGAR, d.SCORE_ONLY, d.SCORE_ONLY | d.RIGHT):
        got, _ = _check(lib, q, t, mat, costs, 5, capfd, flag=flag, msg=flag)
        d.check_cigars(got, q, t, mat, 5, costs, flag)
        for g, b in zip(got, base):
            assert all(g[f] == b[f] for f in ("score", "qb", "qe", "tb", "te"))
            assert not (flag & d.SCORE_ONLY) or (g["n_cigar"] == 0 and g["cigar"] == [])
            differs += g["cigar"] != b["cigar"] and not flag & d.SCORE_ONLY
    assert differs > 0
    with pytest.raises(ka.Ksw2Error, match="error -2"):
        lib.lld_align_batch(q[:2], t[:2], mat, *costs, flag=0x40)


@pytest.mark.parametrize("form,m", FORMS)
def test_degenerate_costs_equal_the_single_piece_entries(lib, monkeypatch, form, m):
    """(gapo2, gape2) = (gapo, gape), and gapo2 >= gapo with gape2 >= gape: bit for bit what the ll_* entries return on the device"""
    rng = np.random.default_rng(17 + m)
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    mat = _mat(rng, m)
    q, t = la.new_ground(rng, m, small=True)
    a = lf.arena(q, t, lead=1, gap=1)
    res1, aln1 = lib.ll_batch(q, t, mat, 4, 2, m=m), lib.ll_align_batch(q, t, mat, 4, 2, m=m)
    for go2, ge2 in ((4, 2), (9, 2), (4, 127)):
        costs = (4, 2, go2, ge2)
        np.testing.assert_array_equal(lib.lld_batch(q, t, mat, *costs, m=m), res1)
        np.testing.assert_array_equal(lib.lld_batch_flat(*a, mat, *costs, m=m), res1)
        assert lib.lld_align_batch(q, t, mat, *costs, m=m) == aln1, costs
        assert lib.lld_align_batch_flat(*a, mat, *costs, m=m) == aln1, costs
