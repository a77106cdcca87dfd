"""GPU: ksw2amd_ll_batch_flat / ksw2amd_ll_align_batch_flat on libksw2_amd.so against the scalar oracle and the pointer entries, from a
host arena, a page-locked host arena and a device arena: ragged batches, forced kernel forms, multi-generation tasks with rows = the
query, one query against many targets, bad residue codes (found by k2a_ll_check_kernel before any alignment kernel), chunked calls,
CIGARs with buffer reuse and a C caller built against include/ksw2_amd.h."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ksw2_amd as ka
from tests import ll_util as u
from tests import lla_util as la
from tests import llf_util as f

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("host", "pinned", "device")


@pytest.fixture(scope="module")
def lib():
    L = ka.library()                      # raises if the HIP library is missing: no fallback
    assert L.backend() == "hip:gfx950"
    assert L.device_count() >= 1
    return L


@contextlib.contextmanager
def placed(lib, base, kind):
    """the arena as the call sees it -> keyword arguments for the flat methods"""
    if kind == "host":
        yield dict()
    elif kind == "pinned":
        assert lib.lib.ksw2amd_host_register(ctypes.c_void_p(base.ctypes.data), ctypes.c_size_t(base.nbytes)) == 0, lib.last_error()
        try:
            yield dict()
        finally:
            lib.lib.ksw2amd_host_unregister(ctypes.c_void_p(base.ctypes.data))
    else:
        d = lib.device_copy(base)
        try:
            yield dict(device_base=d)
        finally:
            lib.device_free(d)


@pytest.mark.parametrize("m", [5, 20])
def test_ragged_parity(lib, monkeypatch, m):
    rng = np.random.default_rng(140 + m)
    mat = u.simple_mat(5, 2, 4, -1) if m == 5 else u.random_mat(rng, m)
    q, t = u.ragged(rng, 10000, m, 1, 600, related=0.4)
    q2, t2 = u.ragged(rng, 200, m, 1, 5000, related=0.4)            # lengths 1-5 000 (the oracle is scalar: the long ones are few)
    q, t = q + q2, t + t2
    a = f.arena(q, t, rng, lead=3, gap=5)
    exp = u.oracle_batch(q, t, mat, 4, 2, m)
    for kind in KINDS:
        with placed(lib, a[0], kind) as kw:
            np.testing.assert_array_equal(lib.ll_batch_flat(*a, mat, 4, 2, m=m, **kw), exp, err_msg=kind)


@pytest.mark.parametrize("form,lds", [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")])
def test_forced_forms_and_generations(lib, monkeypatch, form, lds):
    rng = np.random.default_rng(17)
    monkeypatch.setenv("KSW2AMD_LL_FORM", form)
    monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
    mat = u.simple_mat(5, 2, 4, -1)
    q = [rng.integers(0, 5, 256, dtype=np.uint8) for _ in range(512)]
    t = [np.concatenate([rng.integers(0, 5, 300, dtype=np.uint8), u.mutate(rng, x, 5)[:200], rng.integers(0, 5, 1024, dtype=np.uint8)])[:1024]
         for x in q]
    q += [rng.integers(0, 5, 3000, dtype=np.uint8) for _ in range(6)]       # several generations, rows = the query
    t += [rng.integers(0, 5, 2500, dtype=np.uint8) for _ in range(6)]
    a = f.arena(q, t, rng, lead=7, gap=3)
    exp = u.oracle_batch(q, t, mat, 4, 2)
    for kind in KINDS:
        with placed(lib, a[0], kind) as kw:
            np.testing.assert_array_equal(lib.ll_batch_flat(*a, mat, 4, 2, **kw), exp, err_msg=kind)


def test_one_query_many_targets(lib):
    rng = np.random.default_rng(18)
    mat = u.simple_mat(5, 2, 4, -1)
    q = rng.integers(0, 5, 250, dtype=np.uint8)
    ts = [np.concatenate([rng.integers(0, 5, int(rng.integers(0, 500)), dtype=np.uint8), u.mutate(rng, q, 5), rng.integers(0, 5, int(rng.integers(0, 300)), dtype=np.uint8)])
          for _ in range(4096)]
    b, qo, ql, to, tl = f.arena([q], ts, lead=1, gap=0)
    a = (b, np.full(4096, qo[0], np.uint64), np.full(4096, ql[0], np.int32), to, tl)
    exp = lib.ll_batch([q] * 4096, ts, mat, 4, 2)
    assert (exp[:, 0] > 0).all()
    for kind in KINDS:
        with placed(lib, a[0], kind) as kw:
            np.testing.assert_array_equal(lib.ll_batch_flat(*a, mat, 4, 2, **kw), exp, err_msg=kind)


def test_bad_codes_end_in_e_param(lib):
    """every case must come back as KSW2AMD_E_PARAM with reset results: the check runs before any alignment kernel"""
    rng = np.random.default_rng(19)
    m = 5
    mat = u.simple_mat(5, 2, 4, -1)
    qs, ts = u.ragged(rng, 300, m, 70, 400)
    good = f.arena(qs, ts, rng, lead=5, gap=4, fill=0)
    cases = []
    for side, (off, ln) in enumerate(((good[1], good[2]), (good[3], good[4]))):
        for pair in (0, 150, 299):
            o, l = int(off[pair]), int(ln[pair])
            for pos in (o, o + l - 1, o + 1, o + 40, (o + l) // 16 * 16 if (o + l) % 16 else o + l - 1):
                cases.append((pair, pos))
    for k, (pair, pos) in enumerate(cases):
        v = (m, 127, 128, 255)[k % 4]
        kind = KINDS[k % 3]
        a = (good[0].copy(),) + good[1:]
        a[0][pos] = v
        out = np.full((300, 3), 77, np.int32)
        with placed(lib, a[0], kind) as kw:
            with pytest.raises(ka.Ksw2Error, match=r"error -2.*pair %d: residue code >= m" % pair):
                lib.ll_batch_flat(*a, mat, 4, 2, out=out, **kw)
        assert (out == [0, -1, -1]).all(), (pair, pos, v, kind)
    # two pairs at once: the lower one is named; the align entry resets every field
    a = (good[0].copy(),) + good[1:]
    a[0][int(a[1][200]) + 3] = 9
    a[0][int(a[3][31]) + 7] = 200
    aln = (ka.LocalAln * 300)()
    for kind in ("host", "device"):
        with placed(lib, a[0], kind) as kw:
            with pytest.raises(ka.Ksw2Error, match="pair 31: residue code"):
                lib.ll_align_batch_flat(*a, mat, 4, 2, aln=aln, **kw)
        assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)
    # ... and bytes >= m outside the sequences are nobody's business
    a = f.arena(qs, ts, rng, lead=5, gap=4, fill=255)
    exp = lib.ll_batch(qs, ts, mat, 4, 2)
    for kind in KINDS:
        with placed(lib, a[0], kind) as kw:
            np.testing.assert_array_equal(lib.ll_batch_flat(*a, mat, 4, 2, **kw), exp, err_msg=kind)


def test_chunked_call(lib, monkeypatch):
    rng = np.random.default_rng(23)
    mat = u.simple_mat(5, 2, 4, -1)
    qs, ts = u.ragged(rng, 600, 5, 50, 300)
    a = f.arena([x for p in zip(qs, ts) for x in p], [], lead=2, gap=1, fill=0)
    a = (a[0], a[1][0::2].copy(), a[2][0::2].copy(), a[1][1::2].copy(), a[2][1::2].copy())
    exp = lib.ll_batch(qs, ts, mat, 4, 2)
    monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "60000")          # >= 4 chunks
    for kind in ("host", "device"):
        with placed(lib, a[0], kind) as kw:
            np.testing.assert_array_equal(lib.ll_batch_flat(*a, mat, 4, 2, **kw), exp, err_msg=kind)
    a[0][int(a[1][599]) + 1] = 5                                   # the last chunk fails: the first ones' results are in place
    out = np.full((600, 3), 77, np.int32)
    with pytest.raises(ka.Ksw2Error, match="pair 599: residue code"):
        lib.ll_batch_flat(*a, mat, 4, 2, out=out)
    done = int((out[:, 0] > 0).sum())
    assert 100 < done < 600 and (out[:done] == exp[:done]).all() and (out[done:] == [0, -1, -1]).all()


@pytest.mark.parametrize("flag", [0, la.SCORE_ONLY, la.RIGHT, la.REV_CIGAR])
def test_align_equals_pointer_entry(lib, flag):
    rng = np.random.default_rng(24 + flag)
    mat = u.simple_mat(5, 2, 4, -1)
    qs, ts = la.new_ground(rng, 5)
    q2, t2 = u.ragged(rng, 1500, 5, 1, 500, related=0.6)
    qs, ts = qs + q2, ts + t2
    a = f.arena(qs, ts, rng, lead=3, gap=5)
    exp = lib.ll_align_batch(qs, ts, mat, 4, 2, flag=flag)
    for kind in KINDS:
        with placed(lib, a[0], kind) as kw:
            assert lib.ll_align_batch_flat(*a, mat, 4, 2, flag=flag, **kw) == exp, kind


def test_align_reuses_cigar_buffers(lib):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, -1)
    qs, ts = u.ragged(rng, 200, 5, 30, 300, related=1.0)
    a = f.arena(qs, ts, lead=1)
    exp = lib.ll_align_batch(qs, ts, mat, 4, 2)
    aln = (ka.LocalAln * 200)()
    first = lib.ll_align_batch_flat(*a, mat, 4, 2, aln=aln)
    ptrs = [ctypes.cast(aln[i].cigar, ctypes.c_void_p).value for i in range(200)]
    with placed(lib, a[0], "device") as kw:
        again = lib.ll_align_batch_flat(*a, mat, 4, 2, aln=aln, **kw)
    assert first == exp and again == exp
    assert ptrs == [ctypes.cast(aln[i].cigar, ctypes.c_void_p).value for i in range(200)] and any(ptrs)


@pytest.mark.parametrize("kind", KINDS)
def test_c_caller_product_header(lib, tmp_path, kind):
    exe = str(tmp_path / "llf_caller")
    sodir = os.path.dirname(ka.DEFAULT_SO)
    subprocess.run(["gcc", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "dropin", "llf_caller.c"), "-L" + sodir, "-l:libksw2_amd.so", "-Wl,-rpath," + sodir], check=True)
    rng = np.random.default_rng(32)
    mat = u.simple_mat(5, 2, 4, -1)
    q, t = u.ragged(rng, 40, 5, 1, 1500)
    inp = str(tmp_path / "pairs.txt")
    la.write_input(inp, q, t, mat, 5, 4, 2, 0)
    out = subprocess.run([exe, inp, kind], check=True, capture_output=True, text=True, timeout=300).stdout
    lines = out.strip().splitlines()
    k = lines.index("align")
    got = np.array([list(map(int, l.split())) for l in lines[:k]], dtype=np.int32)
    np.testing.assert_array_equal(got, u.oracle_batch(q, t, mat, 4, 2))
    assert lines[-1] == "reused 1"
    aln = [list(map(int, l.split())) for l in lines[k + 1:-1]]
    exp = lib.ll_align_batch(q, t, mat, 4, 2)
    assert [dict(score=v[0], qb=v[1], qe=v[2], tb=v[3], te=v[4], n_cigar=v[5], cigar=v[6:]) for v in aln] == exp
