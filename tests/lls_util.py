"""Helpers of the suboptimal-score tests (ksw2amd_ll_sub_batch): the scalar oracle tests/lls_oracle.c compiled with gcc into a temporary
directory, the simulator build with the reduction kernel's twin (tests/llsim/lls_shim_sim.cpp), a pure-Python statement of the
definition on ll_util.brute's matrix, and the edge grid that the CPU tier (simulator) and the GPU tier share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "lls_cases.npz")
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        out = os.path.join(u.build_dir(), "liblls_oracle_%d.so" % os.getpid())
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", out, os.path.join(HERE, "lls_oracle.c")], check=True)
        lib = ctypes.CDLL(out)
        lib.lls_oracle_batch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                                 ctypes.c_int, ctypes.c_void_p]
        _oracle = lib
    return _oracle


def oracle_batch(queries, targets, mat, gapo, gape, excl=-1, m=None):
    """(n, 6) int32 array of score, qe, te, score2, qe2, te2 from the scalar oracle."""
    mat = np.ascontiguousarray(mat, dtype=np.int8)
    m = int(round(len(mat) ** 0.5)) if m is None else m
    n = len(queries)
    seqs = [np.ascontiguousarray(x, dtype=np.uint8) for x in list(queries) + list(targets)]
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    base = np.concatenate(seqs + [np.zeros(1, np.uint8)]).astype(np.uint8)
    qoff, toff = np.ascontiguousarray(offs[:n]), np.ascontiguousarray(offs[n:2 * n])
    qlen, tlen = lens[:n].astype(np.int32), lens[n:].astype(np.int32)
    out = np.zeros((max(n, 1), 6), dtype=np.int32)
    oracle().lls_oracle_batch(n, base.ctypes.data, qoff.ctypes.data, qlen.ctypes.data, toff.ctypes.data, tlen.ctypes.data,
                              m, mat.ctypes.data, gapo, gape, excl, out.ctypes.data)
    return out[:n]


def brute(query, target, mat, gapo, gape, m, excl):
    """The definition in plain Python on the full matrix: (score, qe, te, score2, qe2, te2)."""
    q, t = list(map(int, query)), list(map(int, target))
    NEG = -(1 << 40)
    H = [[0] * (len(q) + 1) for _ in range(len(t) + 1)]
    E = [[NEG] * (len(q) + 1) for _ in range(len(t) + 1)]
    F = [[NEG] * (len(q) + 1) for _ in range(len(t) + 1)]
    for i in range(1, len(t) + 1):
        for j in range(1, len(q) + 1):
            E[i][j] = max(E[i - 1][j] - gape, H[i - 1][j] - gapo - gape)
            F[i][j] = max(F[i][j - 1] - gape, H[i][j - 1] - gapo - gape)
            H[i][j] = max(0, H[i - 1][j - 1] + int(mat[t[i - 1] * m + q[j - 1]]), E[i][j], F[i][j])
    score, qe, te = u.brute(query, target, mat, gapo, gape, m)
    smax = max(int(x) for x in mat)
    if smax <= 0 or not q or not t:
        return 0, -1, -1, 0, -1, -1
    d = excl if excl >= 0 else -(-score // smax)
    rows = [i for i in range(len(t)) if abs(i - te) > d]
    s2 = max([max(H[i + 1][1:]) for i in rows], default=0)
    if s2 <= 0:
        return score, qe, te, 0, -1, -1
    te2 = min(i for i in rows if max(H[i + 1][1:]) == s2)
    qe2 = min(j for j in range(len(q)) if H[te2 + 1][j + 1] == s2)
    return score, qe, te, s2, qe2, te2


def sim_library(path_out=None):
    """The product's host objects -- ksw2_host_ll.c, _lla.c, _llf.c and _lls.c included -- against tests/sim/ksw2_shim_sim.cpp and
    tests/llsim/lls_shim_sim.cpp (every local-alignment twin compiled in).  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="llssim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf", "lls"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "lls_shim_sim.cpp"), "llssim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_llssim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def sub_launches(lib):
    lib.lib.lls_sim_sub_launches.restype = ctypes.c_long
    return int(lib.lib.lls_sim_sub_launches())


def reset_counters(lib):
    lib.lib.lls_sim_reset_counters.restype = None
    lib.lib.lls_sim_reset_counters()


# ---------------------------------------------------------------- the edge grid (both tiers)
M5 = u.simple_mat(5, 2, 4, -1)


def two_copies(rng, qlen, tlen, end1, m=4):
    """A target of tlen holding two mutated copies of a random query of qlen: the first ends near row end1, the second at the end of
    the target, random bases elsewhere (at least one between the copies)."""
    q = rng.integers(0, m, qlen, dtype=np.uint8)
    a, b = u.mutate(rng, q, m, 0.03, 0.01), u.mutate(rng, q, m, 0.06, 0.01)
    t = rng.integers(0, m, tlen, dtype=np.uint8)
    lo = max(0, end1 + 1 - len(a))
    t[lo:lo + len(a)] = a
    assert lo + len(a) + 1 <= tlen - len(b)
    t[tlen - len(b):] = b
    return q, t


def generation_edges(rng):
    """tlen in {1023, 1024, 1025, 2049} and 1500, qlen 200: the first copy ends at row end1, the second at the last row, so te and te2
    fall in different generations where the target has more than one.  The shapes (2049, 1030) and (1500, 1084) put an end 6 and 60
    rows behind row 1024: with d = ceil(score / 2) up to 200 the window straddles row 1024.  d <= qlen < the distance of the ends."""
    qs, ts = [], []
    for tlen, end1 in ((1023, 400), (1024, 500), (1025, 500), (2049, 1000), (2049, 1030), (1500, 1084)):
        for _ in range(2):                       # twice: a packed partner of the same shape
            q, t = two_copies(rng, 200, tlen, end1)
            qs.append(q)
            ts.append(t)
    return qs, ts


def forced_orientation(rng):
    """pairs that ksw2amd_ll_batch runs with rows = query: qlen 3000 x tlen 700, qlen 1500 x tlen 40 (fewer than 64 live rows)"""
    qs, ts = [], []
    for ql, tl in ((3000, 700), (3000, 700), (1500, 40), (1500, 40), (1500, 40)):
        q = rng.integers(0, 4, ql, dtype=np.uint8)
        t = rng.integers(0, 4, tl, dtype=np.uint8)
        k = tl // 3
        q[100:100 + k] = t[:k]                   # two hits at different target rows
        q[ql - 2 * k:ql - k] = u.mutate(rng, t[tl - k:], 4, 0.05, 0.0)[:k]
        qs.append(q)
        ts.append(t)
    return qs, ts


def window_edges(rng):
    """-> list of (queries, targets, excl): windows clipped at row 0 and at row tlen - 1, a window over every row, excl = 0, excl > tlen"""
    x = rng.integers(0, 4, 60, dtype=np.uint8)
    pad = rng.integers(0, 4, 300, dtype=np.uint8)
    head = np.concatenate([x, pad, u.mutate(rng, x, 4, 0.1, 0.0)])        # te = 59: the default window is clipped at row 0
    tail = np.concatenate([u.mutate(rng, x, 4, 0.1, 0.0), pad, x])        # te = tlen - 1
    same = rng.integers(0, 4, 41, dtype=np.uint8)                        # identical: score 82, d = 41 >= tlen: every row excluded
    out = []
    for excl in (-1, 0, 5, 1 << 20):
        out.append(([x, x, same, x], [head, tail, same.copy(), head], excl))
    return out


def differing_halves(rng, m=5):
    """same shapes, different content: every packed task's halves have their own score, te and window"""
    qs, ts = [], []
    for ql, tl in ((150, 1100), (150, 1100), (300, 300), (300, 300), (90, 2100), (90, 2100), (77, 333)):
        q = rng.integers(0, m, ql, dtype=np.uint8)
        t = rng.integers(0, m, tl, dtype=np.uint8)
        k = min(ql, tl) // 2
        p1, p2 = int(rng.integers(0, tl - k + 1)), int(rng.integers(0, tl - k + 1))
        t[p1:p1 + k] = q[:k]
        t[p2:p2 + k // 2] = q[ql - k // 2:]
        qs.append(q)
        ts.append(t)
    return qs, ts


def tandem_repeats(rng):
    """tandem-repeat pairs: many rows share the best and the second-best maximum (smallest te2, then smallest qe2)"""
    qs, ts = [], []
    for unit, nq, nt in ((3, 4, 40), (5, 3, 30), (2, 6, 50), (7, 2, 400), (4, 5, 300)):
        r = rng.integers(0, 4, unit, dtype=np.uint8)
        qs.append(np.tile(r, nq))
        ts.append(np.tile(r, nt))
    return qs, ts


RAGGED = [(m, go, ge) for m in (5, 20) for go, ge in ((4, 2), (0, 1), (6, 1))]


def ragged_set(k):
    """set k of RAGGED: 2 000 pairs of lengths 1-600 plus 50 of lengths up to 5 000 -> (queries, targets, mat, m, gapo, gape)"""
    m, go, ge = RAGGED[k]
    rng = np.random.default_rng(310 + k)
    q, t = u.ragged(rng, 2000, m, 1, 600)
    q2, t2 = u.ragged(rng, 50, m, 600, 5000)
    return q + q2, t + t2, M5 if m == 5 else u.random_mat(rng, 20), m, go, ge


def wide_score(rng):
    """a near-identical pair of 700 with match 120: score and score2 above 65 535 through the int32 profile words (ll_pk_admit rejects
    the pair: 701 * 120 > 65 535); excl = 60 leaves rows outside the window -> (queries, targets, mat, excl)"""
    q = rng.integers(0, 4, 700, dtype=np.uint8)
    t = q.copy()
    t[rng.integers(0, 700, 6)] = 4                       # wildcard columns: -1 each
    return [q, q[:650]], [t, t[:650]], u.simple_mat(5, 120, 90, -1), 60


# ---------------------------------------------------------------- the checks of the grid: lib is the simulator build or the GPU library
def check(lib, q, t, mat, go, ge, excl=-1, m=None, positive=False):
    """ll_sub_batch against the scalar oracle; res bit-identical to ll_batch; -> the expected (n, 6) array"""
    exp = oracle_batch(q, t, mat, go, ge, excl, m)
    res, sub = lib.ll_sub_batch(q, t, mat, go, ge, excl=excl, m=m)
    np.testing.assert_array_equal(res, exp[:, :3])
    np.testing.assert_array_equal(sub, exp[:, 3:])
    np.testing.assert_array_equal(res, lib.ll_batch(q, t, mat, go, ge, m=m))
    if positive:
        assert (exp[:, 3] > 0).all(), exp
    return exp


def forms(monkeypatch):
    """every (form, lookup) combination of the switches"""
    for form in ("0", "1", "2"):
        for lds in ("0", "1"):
            monkeypatch.setenv("KSW2AMD_LL_FORM", form)
            monkeypatch.setenv("KSW2AMD_LL_LDS", lds)
            yield form, lds


def check_generation_edges(lib, monkeypatch):
    q, t = generation_edges(np.random.default_rng(301))
    for _ in forms(monkeypatch):
        exp = check(lib, q, t, M5, 4, 2, positive=True)
    gen = lambda r: r // 1024
    assert sum(gen(e[2]) != gen(e[5]) for e in exp) >= 4                    # te and te2 in different generations
    assert any(abs(int(e[2]) - 1024) <= -(-int(e[0]) // 2) and e[2] != 1024 for e in exp)      # a window straddling row 1024


def check_forced_orientation(lib, monkeypatch):
    q, t = forced_orientation(np.random.default_rng(302))
    for _ in forms(monkeypatch):
        check(lib, q, t, M5, 4, 2, positive=True)


def check_window_edges(lib, monkeypatch):
    for q, t, excl in window_edges(np.random.default_rng(303)):
        for _ in forms(monkeypatch):
            exp = check(lib, q, t, M5, 4, 2, excl=excl)
        assert exp[2, 0] == 82
        if excl == -1:
            assert exp[0, 2] == 59 and exp[1, 2] == len(t[1]) - 1 and exp[0, 3] > 0 and exp[1, 3] > 0      # clipped at row 0 / at the last row
            assert exp[2, 3:].tolist() == [0, -1, -1]                         # tlen 41 <= 2 d + 1: every row excluded
        if excl == 0:
            assert (exp[:, 3] > 0).all() and (np.abs(exp[:, 5] - exp[:, 2]) >= 1).all()
        if excl > 1000:
            assert (exp[:, 3:] == [0, -1, -1]).all()


def check_differing_halves(lib, monkeypatch, capfd):
    rng = np.random.default_rng(304)
    q, t = differing_halves(rng)
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form, lds in forms(monkeypatch):
        capfd.readouterr()
        exp = check(lib, q, t, M5, 4, 2)
        err = capfd.readouterr().err
        line = [l for l in err.splitlines() if "ll-sub:" in l][0]
        pk, i32 = int(line.split("pk_tasks=")[1].split()[0]), int(line.split("int32_tasks=")[1].split()[0])
        assert (pk, i32) == {"0": (0, 7), "1": (3, 1), "2": (4, 0)}[form], line
        assert ("profile=lds" in line) == (lds == "1") and "excl=-1" in line
    assert len(set(map(tuple, exp[:6, [0, 2]].tolist()))) == 6               # the halves differ in score and te
    m20 = u.random_mat(rng, 20)
    q, t = differing_halves(rng, 20)
    for form in ("0", "1", "2"):
        monkeypatch.setenv("KSW2AMD_LL_FORM", form)
        check(lib, q, t, m20, 6, 1, m=20)


def check_ties(lib, monkeypatch):
    q, t = tandem_repeats(np.random.default_rng(305))
    for _ in forms(monkeypatch):
        exp = check(lib, q, t, M5, 4, 2, positive=True)
    assert (exp[:, 3] == exp[:, 0]).all()                                    # the repeat reaches the best score again outside the window
    for e, qq, tt in zip(exp, q, t):
        assert brute(qq, tt, M5, 4, 2, 5, -1) == tuple(int(x) for x in e)    # smallest te2, then smallest qe2


def check_wide_query(lib, monkeypatch, capfd):
    """qlen = 65 536 against a short target: the column index does not fit 16 bits, the pair takes the int32 form"""
    rng = np.random.default_rng(306)
    t = rng.integers(0, 4, 70, dtype=np.uint8)
    q = rng.integers(0, 4, 65536, dtype=np.uint8)
    q[65536 - 30:] = t[40:]
    q[100:130] = t[:30]
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    monkeypatch.setenv("KSW2AMD_LL_FORM", "2")
    capfd.readouterr()
    exp = check(lib, [q, q[:65535]], [t, t], M5, 4, 2, excl=3, positive=True)
    err = capfd.readouterr().err
    assert "ll-sub: pk_tasks=1 int32_tasks=1 " in err, err                    # 65 535 is admitted (forced self-pairing), 65 536 is not
    assert exp[0, 4] > 65000 or exp[0, 1] > 65000


def check_wide_score(lib, monkeypatch, capfd):
    q, t, mat, excl = wide_score(np.random.default_rng(312))
    monkeypatch.setenv("KSW2AMD_TRACE", "1")
    for form, lds in forms(monkeypatch):
        capfd.readouterr()
        exp = check(lib, q, t, mat, 30, 10, excl=excl)
        assert "ll-sub: pk_tasks=0 int32_tasks=2 " in capfd.readouterr().err
    assert (exp[:, 0] > 65535).all() and (exp[:, 3] > 65535).all() and (np.abs(exp[:, 5] - exp[:, 2]) > excl).all(), exp


def check_flat(lib, placed, kinds, monkeypatch):
    """flat entries against the pointer entry: every arena kind, one query shared by all pairs, a multi-chunk call, a bad code"""
    from tests import llf_util as f
    rng = np.random.default_rng(307)
    q, t = differing_halves(rng)
    q2, t2 = u.ragged(rng, 60, 5, 1, 400)
    q, t = q + q2, t + t2
    a = f.arena(q, t, rng, lead=3, gap=5)
    res0, sub0 = lib.ll_sub_batch(q, t, M5, 4, 2)
    np.testing.assert_array_equal(np.hstack([res0, sub0]), oracle_batch(q, t, M5, 4, 2))
    for kind in kinds:
        with placed(lib, a[0], kind) as kw:
            res, sub = lib.ll_sub_batch_flat(*a, M5, 4, 2, **kw)
            np.testing.assert_array_equal(res, res0)
            np.testing.assert_array_equal(sub, sub0)
    monkeypatch.setenv("KSW2AMD_LL_CHUNK_BYTES", "20000")                    # several chunks
    res, sub = lib.ll_sub_batch_flat(*a, M5, 4, 2)
    np.testing.assert_array_equal(np.hstack([res, sub]), np.hstack([res0, sub0]))
    # a bad code in the last third: the chunks before it are done, res[] and sub[] hold the reset values from the failing chunk on
    base = a[0].copy()
    bad = len(q) - 10
    base[int(a[3][bad])] = 9
    out, so = np.full((len(q), 3), 7, np.int32), np.full((len(q), 3), 7, np.int32)
    try:
        lib.ll_sub_batch_flat(base, *a[1:], M5, 4, 2, out=out, sub=so)
        raise AssertionError("a residue code >= m was accepted")
    except Exception as e:
        assert "error -2" in str(e) and "pair %d" % bad in lib.last_error(), (e, lib.last_error())
    first = next(i for i in range(len(q)) if (out[i] == [0, -1, -1]).all() and (out[i:, 0] == 0).all())
    assert 0 < first <= bad
    np.testing.assert_array_equal(out[:first], res0[:first])
    np.testing.assert_array_equal(so[:first], sub0[:first])
    assert (out[first:] == [0, -1, -1]).all() and (so[first:] == [0, -1, -1]).all()
    monkeypatch.delenv("KSW2AMD_LL_CHUNK_BYTES")
    # one query shared by all pairs
    qq = rng.integers(0, 4, 120, dtype=np.uint8)
    ts = [np.concatenate([u.mutate(rng, qq, 4), rng.integers(0, 4, 50, dtype=np.uint8), u.mutate(rng, qq, 4, 0.1)]) for _ in range(20)]
    b = f.arena([qq], ts)
    qoff, qlen = np.repeat(b[1], 20), np.repeat(b[2], 20)
    res, sub = lib.ll_sub_batch_flat(b[0], qoff, qlen, b[3], b[4], M5, 4, 2)
    np.testing.assert_array_equal(np.hstack([res, sub]), oracle_batch([qq] * 20, ts, M5, 4, 2))
    assert (sub[:, 0] > 0).all()


def check_bad_arguments(lib, Ksw2Error, launches=None):
    """launches: () -> the launches a simulator build has counted; every rejected or empty call must leave it at zero"""
    one = [np.array([0, 1, 2, 3, 0, 1], np.uint8)]
    for args, kw in (((one, [np.array([0, 5], np.uint8)], M5, 4, 2), {}), ((one, one, M5, -1, 2), {}), ((one, one, M5, 4, 128), {}),
                     ((one, one, M5, 4, 2), dict(excl=0x40000000)), ((one, one, M5[:16], 4, 2), dict(m=0))):
        try:
            lib.ll_sub_batch(*args, **kw)
            raise AssertionError("accepted: %r" % (kw,))
        except Ksw2Error as e:
            assert "error -2" in str(e), e
    res, sub = lib.ll_sub_batch([], [], M5, 4, 2)
    assert res.shape == (0, 3) and sub.shape == (0, 3)
    res, sub = lib.ll_sub_batch(one, one, -np.abs(M5), 4, 2)                  # no positive entry: nothing launched
    assert res.tolist() == [[0, -1, -1]] and sub.tolist() == [[0, -1, -1]]
    res, sub = lib.ll_sub_batch(one + [np.zeros(0, np.uint8)], [np.zeros(0, np.uint8)] + one, M5, 4, 2)
    assert res.tolist() == [[0, -1, -1]] * 2 and sub.tolist() == [[0, -1, -1]] * 2
    before = lib.error_count()                                              # the single-pair call reports a bad argument like ksw_ll_i16
    assert lib.ll_sub(one[0], one[0], M5, 4, 2, excl=0x40000000) == ((0, -1, -1), (0, -1, -1))
    assert lib.error_count() == before + 1 and "excl" in lib.last_error()
    assert launches is None or launches() == 0, launches()                 # nothing above reached a launch
    rng = np.random.default_rng(308)
    q, t = generation_edges(rng)
    exp = oracle_batch(q[:3], t[:3], M5, 4, 2, 7)
    for i in range(3):                                                      # the single-pair call
        r, s = lib.ll_sub(q[i], t[i], M5, 4, 2, excl=7)
        assert list(r) + list(s) == exp[i].tolist()
    assert lib.ll_sub(np.zeros(0, np.uint8), t[0], M5, 4, 2) == ((0, -1, -1), (0, -1, -1))


def check_c_caller(so_dir, libname, tmp_path):
    """tests/dropin/lls_caller.c built against include/ksw2_amd.h: the batch call and the single calls print the oracle's numbers"""
    exe = str(tmp_path / "lls_caller")
    subprocess.run(["gcc", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(HERE, "dropin", "lls_caller.c"),
                    "-L" + so_dir, "-l" + libname, "-Wl,-rpath," + so_dir], check=True)
    rng = np.random.default_rng(309)
    q, t = u.ragged(rng, 12, 5, 1, 500)
    q2, t2 = generation_edges(rng)
    q, t = q + q2[:2], t + t2[:2]
    inp = str(tmp_path / "pairs.txt")
    with open(inp, "w") as f:
        f.write("5 4 2 -1\n%s\n%d\n" % (" ".join(str(int(x)) for x in M5), len(q)))
        for a, b in zip(q, t):
            f.write("%d %s\n%d %s\n" % (len(a), " ".join(map(str, a.tolist())), len(b), " ".join(map(str, b.tolist()))))
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True).stdout
    got = np.array([list(map(int, l.split())) for l in out.strip().splitlines()], dtype=np.int32)
    exp = oracle_batch(q, t, M5, 4, 2)
    np.testing.assert_array_equal(got, np.vstack([exp, exp]))


def load_golden():
    """-> list of (queries, targets, mat, m, gapo, gape, excl, expected (n, 6)) from tests/golden/lls_cases.npz"""
    z = np.load(GOLDEN)
    out = []
    for k in range(int(z["nsets"])):
        m, go, ge, excl = map(int, z["s%d_par" % k])
        ql, tl = z["s%d_qlen" % k], z["s%d_tlen" % k]
        qo, to = np.concatenate([[0], np.cumsum(ql)]), np.concatenate([[0], np.cumsum(tl)])
        q = [z["s%d_q" % k][qo[i]:qo[i + 1]] for i in range(len(ql))]
        t = [z["s%d_t" % k][to[i]:to[i + 1]] for i in range(len(tl))]
        out.append((q, t, z["s%d_mat" % k], m, go, ge, excl, z["s%d_res" % k]))
    return out
