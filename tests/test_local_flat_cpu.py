"""CPU: ksw2amd_ll_batch_flat / ksw2amd_ll_align_batch_flat on the simulator build of tests/llf_util.py -- the product's host objects
against the lock-step twins of the local-alignment kernels and of k2a_ll_check_kernel.  "Device" memory is host memory there, so
on_device = 1 runs the same code paths as on the GPU (arena used in place, intervals brought back for the CIGAR stage)."""
import ctypes
import os

import numpy as np
import pytest

import ksw2_amd
from tests import ll_util as u
from tests import lla_util as la
from tests import llf_util as f

E_PARAM = "error -2"


@pytest.fixture(scope="module")
def lib():
    return ksw2_amd.Library(f.sim_library())


@pytest.fixture(autouse=True)
def _env():
    keys = ("KSW2AMD_LL_CHUNK_BYTES", "KSW2AMD_LL_FORM", "KSW2AMD_LL_LDS")
    old = {k: os.environ.pop(k, None) for k in keys}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def flat(lib, a, mat, go, ge, m, dev):
    return lib.ll_batch_flat(*a, mat, go, ge, m=m, device_base=a[0].ctypes.data if dev else None)


def check_parity(lib, qs, ts, a, mat, go, ge, m):
    exp = u.oracle_batch(qs, ts, mat, go, ge, m)
    ptr = lib.ll_batch(qs, ts, mat, go, ge, m=m)
    assert (ptr == exp).all()
    for dev in (0, 1):
        got = flat(lib, a, mat, go, ge, m, dev)
        assert (got == exp).all(), (dev, np.nonzero((got != exp).any(axis=1))[0][:5])


@pytest.mark.parametrize("m,form", [(5, 1), (5, 0), (5, 2), (20, 1)])
def test_ragged_parity(lib, m, form):
    rng = np.random.default_rng(100 + m + form)
    os.environ["KSW2AMD_LL_FORM"] = str(form)
    mat = u.simple_mat(5, 2, 4, 0) if m == 5 else u.random_mat(rng, m)
    qs, ts = u.ragged(rng, 120, m, 1, 260)
    q2, t2 = u.ragged(rng, 3, m, 900, 1400)                    # rows above one generation
    qs, ts = qs + q2 + t2[:1], ts + t2 + q2[:1]                # ... also with rows = the query
    a = f.arena(qs, ts, rng, lead=5, gap=7)
    check_parity(lib, qs, ts, a, mat, 4, 2, m)


def test_every_offset_residue_mod_16(lib):
    rng = np.random.default_rng(7)
    mat = u.simple_mat(5, 2, 4, 0)
    for lead in range(16):
        qs, ts = u.ragged(rng, 6, 5, 1, 90)
        a = f.arena(qs, ts, lead=lead, gap=0, align=16)        # every sequence starts at lead mod 16
        assert all(int(o) % 16 == lead for o in list(a[1]) + list(a[3]))
        base = a[0]
        shift = (-base.ctypes.data) % 16                        # ... of a 16-byte aligned address
        buf = np.full(len(base) + 32, 255, np.uint8)
        buf[shift:shift + len(base)] = base
        a = (buf[shift:shift + len(base)],) + a[1:]
        assert a[0].ctypes.data % 16 == 0
        check_parity(lib, qs, ts, a, mat, 4, 2, 5)


def test_overlapping_and_shared_sequences(lib):
    rng = np.random.default_rng(8)
    mat = u.simple_mat(5, 2, 4, 0)
    base = rng.integers(0, 5, 4000, dtype=np.uint8)
    n = 80
    qoff = rng.integers(0, 3000, n).astype(np.uint64)
    toff = rng.integers(0, 3000, n).astype(np.uint64)
    qlen = rng.integers(1, 400, n).astype(np.int32)
    tlen = rng.integers(1, 900, n).astype(np.int32)
    a = (base, qoff, qlen, toff, tlen)
    qs, ts = f.pairs_of(*a)
    check_parity(lib, qs, ts, a, mat, 4, 2, 5)
    # one query shared by all pairs: scanned once by the check
    q = rng.integers(0, 5, 150, dtype=np.uint8)
    ts = [rng.integers(0, 5, int(rng.integers(1, 300)), dtype=np.uint8) for _ in range(64)]
    b, qo, ql, to, tl = f.arena([q], ts, lead=1, gap=3)
    a = (b, np.full(64, qo[0], np.uint64), np.full(64, ql[0], np.int32), to, tl)
    f.reset_counters(lib)
    check_parity(lib, [q] * 64, ts, a, mat, 4, 2, 5)
    blocks = f.counters(lib)[2] / 2                              # two flat calls
    assert blocks <= (len(q) + sum(map(len, ts))) / 16 + 2 * 65, blocks


def test_empty_sequences_and_n0(lib):
    rng = np.random.default_rng(9)
    mat = u.simple_mat(5, 2, 4, 0)
    qs, ts = u.ragged(rng, 12, 5, 1, 60)
    for i in (0, 5):
        qs[i] = np.zeros(0, np.uint8)
    ts[3] = np.zeros(0, np.uint8)
    qs[7] = ts[7] = np.zeros(0, np.uint8)
    a = f.arena(qs, ts, lead=2, gap=1)
    check_parity(lib, qs, ts, a, mat, 4, 2, 5)
    z = np.zeros(0, np.uint8)
    for dev in (0, 1):
        assert lib.ll_batch_flat(z, [], [], [], [], mat, 4, 2, device_base=1234 if dev else None).shape == (0, 3)
        assert lib.ll_align_batch_flat(z, [], [], [], [], mat, 4, 2, device_base=1234 if dev else None) == []
    # every pair empty on one side: no task, the codes are still checked
    a = f.arena([z, z], [ts[0], ts[1]], lead=1)
    assert (flat(lib, a, mat, 4, 2, 5, 0) == [[0, -1, -1]] * 2).all()
    a[0][int(a[3][1])] = 9
    with pytest.raises(ksw2_amd.Ksw2Error, match="pair 1: residue code"):
        flat(lib, a, mat, 4, 2, 5, 0)


def test_argument_checks(lib):
    mat = u.simple_mat(5, 2, 4, 0)
    one = np.array([1, 2, 3], np.uint8)
    a = f.arena([one], [one])
    for m in (0, 128):
        with pytest.raises(ksw2_amd.Ksw2Error, match=E_PARAM):
            lib.ll_batch_flat(*a, mat, 4, 2, m=m)
    assert lib.lib.ksw2amd_ll_batch_flat(5, None, 4, 2, 0, None, None) == -2
    with pytest.raises(ksw2_amd.Ksw2Error, match=E_PARAM):
        lib.ll_batch_flat(*a, mat, 200, 2)
    with pytest.raises(ksw2_amd.Ksw2Error, match="flag accepts"):
        lib.ll_align_batch_flat(*a, mat, 4, 2, flag=0x40)
    fl = ksw2_amd.LocalFlat()
    out = (ksw2_amd.LocalResult * 1)()
    mp = mat.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))
    assert lib.lib.ksw2amd_ll_batch_flat(5, mp, 4, 2, 1, ctypes.byref(fl), out) == -2          # NULL arrays
    assert lib.lib.ksw2amd_ll_batch_flat(5, mp, 4, 2, -1, ctypes.byref(fl), out) == -2
    # the two sequences of one pair more than 4 GiB apart: refused before anything is touched
    far = (a[0], np.array([0], np.uint64), a[2], np.array([1 << 33], np.uint64), a[4])
    with pytest.raises(ksw2_amd.Ksw2Error, match="4 GiB"):
        lib.ll_batch_flat(*far, mat, 4, 2)


@pytest.mark.parametrize("flag", [0, la.SCORE_ONLY, la.RIGHT, la.REV_CIGAR])
def test_align_equals_pointer_entry(lib, flag):
    rng = np.random.default_rng(20 + flag)
    for m in (5, 20):
        mat = u.simple_mat(5, 2, 4, 0) if m == 5 else u.random_mat(rng, m)
        qs, ts = la.new_ground(rng, m, small=True)
        a = f.arena(qs, ts, rng, lead=3, gap=5)
        exp = lib.ll_align_batch(qs, ts, mat, 4, 2, flag=flag, m=m)
        assert any(e["score"] > 0 for e in exp)
        for dev in (0, 1):
            got = lib.ll_align_batch_flat(*a, mat, 4, 2, flag=flag, m=m, device_base=a[0].ctypes.data if dev else None)
            assert got == exp, (m, dev)


def test_align_reuses_cigar_buffers(lib):
    rng = np.random.default_rng(31)
    mat = u.simple_mat(5, 2, 4, 0)
    qs, ts = u.ragged(rng, 20, 5, 30, 200, related=1.0)
    a = f.arena(qs, ts, lead=1)
    aln = (ksw2_amd.LocalAln * 20)()
    first = lib.ll_align_batch_flat(*a, mat, 4, 2, aln=aln)
    ptrs = [ctypes.cast(aln[i].cigar, ctypes.c_void_p).value for i in range(20)]
    caps = [aln[i].m_cigar for i in range(20)]
    again = lib.ll_align_batch_flat(*a, mat, 4, 2, aln=aln, device_base=a[0].ctypes.data)
    assert again == first == lib.ll_align_batch(qs, ts, mat, 4, 2)
    assert ptrs == [ctypes.cast(aln[i].cigar, ctypes.c_void_p).value for i in range(20)] and caps == [aln[i].m_cigar for i in range(20)]
    assert any(p for p in ptrs)


def _expect_bad(lib, a, mat, m, pair, dev=0, align=False):
    """the call fails with E_PARAM naming `pair`, leaves reset results and launches no alignment kernel"""
    n = len(a[1])
    f.reset_counters(lib)
    db = a[0].ctypes.data if dev else None
    if align:
        aln = (ksw2_amd.LocalAln * n)()
        for i in range(n):
            aln[i].score, aln[i].qb, aln[i].te, aln[i].n_cigar = 5, 5, 5, 5
        with pytest.raises(ksw2_amd.Ksw2Error, match=r"%s.*pair %d: residue code >= m" % (E_PARAM, pair)):
            lib.ll_align_batch_flat(*a, mat, 4, 2, m=m, device_base=db, aln=aln)
        assert all((x.score, x.qb, x.qe, x.tb, x.te, x.n_cigar) == (0, -1, -1, -1, -1, 0) for x in aln)
    else:
        out = np.full((n, 3), 77, np.int32)
        with pytest.raises(ksw2_amd.Ksw2Error, match=r"%s.*pair %d: residue code >= m" % (E_PARAM, pair)):
            lib.ll_batch_flat(*a, mat, 4, 2, m=m, device_base=db, out=out)
        assert (out == [0, -1, -1]).all()
    al, ck, _ = f.counters(lib)
    assert al == 0 and ck == 1


@pytest.mark.parametrize("m", [5, 20])
def test_bad_codes(lib, m):
    rng = np.random.default_rng(40 + m)
    mat = u.simple_mat(5, 2, 4, 0) if m == 5 else u.random_mat(rng, m)
    qs, ts = u.ragged(rng, 9, m, 70, 120)
    values = [v for v in (m, 127, 128, 255)]
    for lead in (0, 5):                                   # sequences 16-byte aligned, and with an unaligned head
        good = f.arena(qs, ts, lead=lead, gap=2, fill=0, align=16)
        shift = (-good[0].ctypes.data) % 16
        buf = np.zeros(len(good[0]) + 32, np.uint8)
        for side, (off, ln) in enumerate(((good[1], good[2]), (good[3], good[4]))):
            for pair in (0, 4, 8):
                o, l = int(off[pair]), int(ln[pair])
                head = (16 - (o % 16)) % 16                # bytes before the first aligned block boundary
                places = {"first": o, "last": o + l - 1, "body": o + head + 17, "tail": (o + l) // 16 * 16 if (o + l) % 16 else o + l - 1}
                if head:
                    places["head"] = o + head - 1
                for where, pos in places.items():
                    assert o <= pos < o + l, (where, pos, o, l)
                    for k, v in enumerate(values):
                        buf[shift:shift + len(good[0])] = good[0]
                        a = (buf[shift:shift + len(good[0])],) + good[1:]
                        a[0][pos] = v
                        _expect_bad(lib, a, mat, m, pair, dev=(k + pair + side) % 2, align=(where == "body" and k == 0))
    # two pairs at once: the lower index is named, whichever is found first
    a = f.arena(qs, ts, lead=3, gap=2, fill=0)
    a[0][int(a[1][6]) + 2] = m
    a[0][int(a[3][2]) + int(a[4][2]) - 1] = 255
    _expect_bad(lib, a, mat, m, 2)
    _expect_bad(lib, a, mat, m, 2, dev=1, align=True)
    # a shared sequence names the lowest pair that references it
    b = f.arena(qs, ts, lead=3, gap=2, fill=0)
    b[1][:] = b[1][5]
    b[2][:] = b[2][5]
    b[0][int(b[1][5]) + 1] = m + 1
    _expect_bad(lib, b, mat, m, 0)


def test_bytes_between_sequences_are_not_checked(lib):
    rng = np.random.default_rng(50)
    mat = u.simple_mat(5, 2, 4, 0)
    qs, ts = u.ragged(rng, 30, 5, 1, 100)
    a = f.arena(qs, ts, rng, lead=9, gap=6, fill=255)        # every byte outside a sequence is 255, the one before and after included
    assert (a[0] == 255).sum() > 30
    check_parity(lib, qs, ts, a, mat, 4, 2, 5)
    exp = lib.ll_align_batch(qs, ts, mat, 4, 2)
    assert lib.ll_align_batch_flat(*a, mat, 4, 2) == exp


def test_chunking(lib):
    rng = np.random.default_rng(60)
    mat = u.simple_mat(5, 2, 4, 0)
    qs, ts = u.ragged(rng, 40, 5, 100, 200)
    a = f.arena(qs, ts, lead=4, gap=3, fill=0)
    # the arena holds the queries, then the targets: order the pairs' sequences side by side so that a chunk's span stays short
    a = f.arena([x for p in zip(qs, ts) for x in p], [], lead=4, gap=3, fill=0)
    a = (a[0], a[1][0::2].copy(), a[2][0::2].copy(), a[1][1::2].copy(), a[2][1::2].copy())
    exp = u.oracle_batch(qs, ts, mat, 4, 2, 5)
    exp_aln = lib.ll_align_batch(qs, ts, mat, 4, 2)
    os.environ["KSW2AMD_LL_CHUNK_BYTES"] = "5000"
    for dev in (0, 1):
        f.reset_counters(lib)
        assert (flat(lib, a, mat, 4, 2, 5, dev) == exp).all()
        nchunks = f.counters(lib)[1]
        assert nchunks >= 3, nchunks
        assert lib.ll_align_batch_flat(*a, mat, 4, 2, device_base=a[0].ctypes.data if dev else None) == exp_aln
    # a bad code in the second chunk: the first chunk's results stay, the rest is reset, the pair named is the call's index
    per = 40 // nchunks + 1
    pair = per + 2
    a[0][int(a[3][pair]) + 3] = 5
    out = np.full((40, 3), 77, np.int32)
    f.reset_counters(lib)
    with pytest.raises(ksw2_amd.Ksw2Error, match="pair %d: residue code" % pair):
        lib.ll_batch_flat(*a, mat, 4, 2, out=out)
    al, ck, _ = f.counters(lib)
    assert ck == 2 and al >= 1
    done = int((out[:, 0] > 0).sum())
    assert 0 < done < pair + 1 and (out[:done] == exp[:done]).all() and (out[done:] == [0, -1, -1]).all()
    os.environ.pop("KSW2AMD_LL_CHUNK_BYTES")
    f.reset_counters(lib)
    with pytest.raises(ksw2_amd.Ksw2Error, match="pair %d: residue code" % pair):
        lib.ll_batch_flat(*a, mat, 4, 2, out=out)
    assert f.counters(lib)[:2] == (0, 1) and (out == [0, -1, -1]).all()
