#!/usr/bin/env python3
"""Local-alignment throughput (ksw2amd_ll_batch): cells = qlen x tlen summed over the batch.

  python tools/scripts/ll_bench.py --workload A [--reps 3] [--out profiles/ll_bench_A.json]

Workloads: A 65 536 x (256 x 1 024) (packed form), B 4 096 x 5 000^2, C 16 384 ragged pairs of 100-5 000, D 1 024 x 20 000^2 (int32 form:
KSW2AMD_LL_FORM=0, its scores would fit the packed form).  Reports end-to-end GCUPS (Python pair setup, staging, upload, kernels,
download; best of --reps after one warm-up) and, when --kstats points at a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a run
of the same workload with --kbatches ll_batch calls (1 + that run's --reps), resident GCUPS from the k2a_ll_kernel time per batch.
The record names the kernel forms the batch took (the library's KSW2AMD_TRACE line).
A parity sample (the scalar test oracle, tests/ll_oracle.c) is checked outside the clock.

  python tools/scripts/ll_bench.py --workload C --align cigar [--baseline] [--pairs N] [--out profiles/lla_bench_C.json]

--align coords | cigar: ksw2amd_ll_align_batch (start cell, KSW_EZ_SCORE_ONLY; or with the CIGAR) instead of ksw2amd_ll_batch.
--baseline: what a caller had to do before that entry existed, through the public API only -- ksw2amd_ll_batch, host reversal of the
prefixes, a second ksw2amd_ll_batch, and for `cigar` ksw2amd_extz_batch on the intervals; timed the same way, and compared with the
new entry's results outside the clock.  Rates stay in forward cells (qlen x tlen); rev_cells = sum of (qe + 1) x (te + 1) is recorded
for the start-cell pass (its kernel: k2a_ll_rev_kernel in --kstats).  --pairs N: the first N pairs of the workload.

  python tools/scripts/ll_bench.py --workload A --flat all [--align coords] [--out profiles/llf_bench_A.json]

--flat host | host-pinned | device | all: ksw2amd_ll_batch_flat (with --align coords: ksw2amd_ll_align_batch_flat, KSW_EZ_SCORE_ONLY)
from one arena, against the unchanged pointer entry on the same pairs.  On both sides the clock covers ONLY the library call: the
ksw2amd_lpair_t array, the arena, the offset arrays, page-locking and the device copy are made before it.  --no-compare skips the
pointer entry (a profiled run then holds 1 + reps batches of one path); --kstats adds k2a_ll_check_kernel next to k2a_ll_kernel.

  python tools/scripts/ll_bench.py --workload A --sub [--excl -1] [--ktrace kernel_trace.csv] [--out profiles/lls_bench_A.json]

--sub: ksw2amd_ll_sub_batch (suboptimal score) beside ksw2amd_ll_batch on the same prebuilt pair array, the
library call alone in the clock on both sides; pairs/s and GCUPS of both and their ratio, the forms both took, how many pairs change
orientation (qlen > tlen: ll_batch runs them with rows = query), res equality and a parity sample against tests/lls_oracle.c.
--ktrace: the kernel_trace.csv of a `rocprofv3 --kernel-trace` run of the same command -- per batch the time of k2a_ll_kernel, of
k2a_ll_fsub_kernel and of k2a_ll_sub_kernel, their ratio, and the batch-to-batch spread of k2a_ll_kernel over its timed batches.

  python tools/scripts/ll_bench.py --workload A --dual [--align coords|cigar] [--ktrace kernel_trace.csv] [--out profiles/lld_bench_A.json]

--dual: ksw2amd_lld_batch under the two-piece costs (4, 2, 24, 1) beside ksw2amd_ll_batch under (4, 2) on the
same prebuilt pair array -- with --align the two align entries (coords: KSW_EZ_SCORE_ONLY) -- the library call alone in the clock on
both sides, a warm-up plus --reps batches of each in one process; pairs/s and GCUPS of both, their ratio, the spread of the single-piece
batches, the forms both took, how many scores the second piece changes and a parity sample against tests/lld_oracle.c.  --ktrace: the
kernel_trace.csv of a `rocprofv3 --kernel-trace` run of the same command -- per batch the time of k2a_ll_kernel (+ k2a_ll_rev_kernel)
and of k2a_lld_kernel (+ k2a_lld_rev_kernel), their ratio and the batch-to-batch spread of the single-piece kernels.

  python tools/scripts/ll_bench.py --workload A --dual --sub [--excl -1] [--ktrace kernel_trace.csv] [--out profiles/llds_bench_A.json]

--dual --sub: ksw2amd_lld_sub_batch beside ksw2amd_lld_batch, both under (4, 2, 24, 1), on the same prebuilt pair
array, the library call alone in the clock on both sides; pairs/s and GCUPS of both and their ratio, the forms both took, res equality and
a parity sample against tests/llds_oracle.c.  --ktrace: per batch the time of k2a_lld_kernel, of k2a_lld_fsub_kernel and of
k2a_ll_sub_kernel, the ratio (k2a_lld_fsub_kernel + k2a_ll_sub_kernel) / k2a_lld_kernel and the batch-to-batch spread of k2a_lld_kernel.

  python tools/scripts/ll_bench.py --workload A --sg [--ktrace kernel_trace.csv] [--out profiles/sg_bench_A.json]

--sg: ksw2amd_sg_batch (semi-global) beside ksw2amd_ll_batch on the same prebuilt pair array, every pair oriented so
that its target is the longer sequence (both entries then run it with rows = target), the library call alone in the clock on both sides
and the two entries ALTERNATING batch by batch in one process; pairs/s and GCUPS (qlen x tlen cells) of both, their ratio, the spread of
the ll_batch batches, the forms both took and a parity sample against tests/sg_oracle.c.  --ktrace: per batch the time of k2a_ll_kernel
and of k2a_sg_kernel, their ratio and the batch-to-batch spread of k2a_ll_kernel.

  python tools/scripts/ll_bench.py --workload A --sg-align [--ktrace kernel_trace.csv] [--out profiles/sga_bench_A.json]

--sg-align: ksw2amd_sg_align_batch on the pair array of --sg: ksw2amd_sg_batch, ksw2amd_sg_align_batch with
KSW_EZ_SCORE_ONLY, ksw2amd_sg_align_batch with CIGARs, and the by-hand pattern they replace (sg_batch, host reversal, ksw2amd_extz_batch for
mqe_t, ksw2amd_extz_batch for the CIGAR) alternate batch by batch, a warm-up plus --reps batches each, library calls only in the clock (the
by-hand pattern's host work is reported beside it).  --ktrace: per batch the time of k2a_sg_kernel and of k2a_sg_rev_kernel.

  python tools/scripts/ll_bench.py --workload A --sgd [--ktrace kernel_trace.csv] [--out profiles/sgd_bench_A.json]
  python tools/scripts/ll_bench.py --workload A --sgd-align [--ktrace kernel_trace.csv] [--out profiles/sgda_bench_A.json]

--sgd: ksw2amd_sgd_batch under (4, 2, 24, 1) beside ksw2amd_lld_batch under the same costs and ksw2amd_sg_batch
under (4, 2), on the pair array of --sg, the three ALTERNATING batch by batch in one process, library calls only in the clock; a parity
sample against tests/sgd_oracle.c.  --sgd-align: ksw2amd_lld_batch, ksw2amd_sgd_align_batch with KSW_EZ_SCORE_ONLY and with CIGARs, the same
way.  --ktrace: per batch the time of k2a_lld_kernel, k2a_sg_kernel, k2a_sgd_kernel and k2a_sgd_rev_kernel, the ratios sgd / lld and
sgd_rev / sgd, and the batch-to-batch spread of k2a_lld_kernel.

  python tools/scripts/ll_bench.py --workload A --ov [--ktrace kernel_trace.csv] [--out profiles/ov_bench_A.json]

--ov: ksw2amd_ov_batch with both query ends free (overlap alignment) beside ksw2amd_ll_batch and ksw2amd_sg_batch on
the pair array of --sg, the three ALTERNATING batch by batch in one process, library calls only in the clock; a parity sample against
tests/ov_oracle.c.  --ktrace: per batch the time of k2a_ll_kernel, k2a_sg_kernel and k2a_ov_kernel, the ratios ov / ll and ov / sg, and the
batch-to-batch spread of k2a_ll_kernel, which the gap between ov and ll is held against.

  python tools/scripts/ll_bench.py --workload A --ov-align [--ktrace kernel_trace.csv] [--out profiles/ova_bench_A.json]

--ov-align: ksw2amd_ov_align_batch / ksw2amd_ovd_align_batch with both query ends free on the pair array of --sg:
ksw2amd_sg_align_batch and ksw2amd_sgd_align_batch with KSW_EZ_SCORE_ONLY (the start passes the new ones are held against, on the same pairs),
ksw2amd_ov_align_batch and ksw2amd_ovd_align_batch with KSW_EZ_SCORE_ONLY, ksw2amd_ov_align_batch with CIGARs, and the by-hand pattern it
replaces (ksw2amd_ov_batch, host reversal of both prefixes, ksw2amd_extz_batch for mqe / mte, the corner constants, ksw2amd_extz_batch for the
CIGAR) alternate batch by batch, a warm-up plus --reps batches each, library calls only in the clock (the by-hand pattern's host work is
reported beside it).  --ktrace: per batch the time of the four forward and the four start-pass kernels, the ratios ov_rev / sg_rev and
ovd_rev / sgd_rev, and the batch-to-batch spread of each."""
import argparse
import ctypes
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import ksw2_amd  # noqa: E402
from tests import ll_util as u  # noqa: E402


def workload(name, rng):
    if name == "A":
        q = [rng.integers(0, 4, 256, dtype=np.uint8) for _ in range(65536)]
        t = [rng.integers(0, 4, 1024, dtype=np.uint8) for _ in range(65536)]
        for i in range(0, 65536, 2):                       # a related window in every other pair
            w = u.mutate(rng, q[i], 4, 0.05, 0.0)[:256]
            t[i][300:300 + len(w)] = w
    elif name == "B":
        q = [rng.integers(0, 4, 5000, dtype=np.uint8) for _ in range(4096)]
        t = [u.mutate(rng, x, 4, 0.05, 0.01)[:5000] for x in q]
        t = [np.concatenate([x, rng.integers(0, 4, 5000 - len(x), dtype=np.uint8)]) if len(x) < 5000 else x for x in t]
    elif name == "C":
        q, t = u.ragged(rng, 16384, 4, 100, 5000, related=0.5)
    elif name == "D":
        q = [rng.integers(0, 4, 20000, dtype=np.uint8) for _ in range(1024)]
        t = [u.mutate(rng, x, 4, 0.01, 0.002)[:20000] for x in q]
        t = [np.concatenate([x, rng.integers(0, 4, 20000 - len(x), dtype=np.uint8)]) if len(x) < 20000 else x for x in t]
    else:
        raise SystemExit("unknown workload " + name)
    return q, t


def kernel_ms(path, batches, name="k2a_ll_kernel"):
    """total time of the kernels whose name contains `name` in a kernel_stats.csv, per batch"""
    tot = 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            if name in row.get("Name", ""):
                tot += float(row["TotalDurationNs"]) * 1e-6
    return tot / batches


GENERIC_SC, SCORE_ONLY = 0x04, 0x01


def align_new(lib, q, t, mat, gapo, gape, cigar):
    r = lib.ll_align_batch(q, t, mat, gapo, gape, flag=0 if cigar else SCORE_ONLY)
    return [(d["score"], d["qb"], d["qe"], d["tb"], d["te"], d["cigar"]) for d in r]


def align_baseline(lib, q, t, mat, gapo, gape, cigar):
    """the three-call pattern of a minimap2 / BWA style caller on the public API"""
    f = lib.ll_batch(q, t, mat, gapo, gape)
    pos = [i for i in range(len(q)) if f[i][0] > 0]
    rq = [np.ascontiguousarray(q[i][:f[i][1] + 1][::-1]) for i in pos]
    rt = [np.ascontiguousarray(t[i][:f[i][2] + 1][::-1]) for i in pos]
    r = lib.ll_batch(rq, rt, mat, gapo, gape)
    out = [(0, -1, -1, -1, -1, [])] * len(q)
    cells = []
    for k, i in enumerate(pos):
        s, qe, te = map(int, f[i])
        cells.append((i, s, qe - int(r[k][1]), qe, te - int(r[k][2]), te))
    cig = [[]] * len(cells)
    if cigar and cells:
        ez = lib.extz_batch([q[i][qb:qe + 1] for i, s, qb, qe, tb, te in cells], [t[i][tb:te + 1] for i, s, qb, qe, tb, te in cells],
                            mat, gapo, gape, w=-1, zdrop=-1, flag=GENERIC_SC)
        cig = [z["cigar"] for z in ez]
    for k, (i, s, qb, qe, tb, te) in enumerate(cells):
        out[i] = (s, qb, qe, tb, te, cig[k])
    return out


def main_flat(a, lib, q, t, mat, gapo, gape, cells, form):
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    align = a.align == "coords"
    if a.align == "cigar":
        raise SystemExit("--flat measures ll_batch and --align coords")
    # everything the calls take, outside the clock
    pairs, keep = lib.local_pairs(q, t)
    lens = np.array([len(x) for x in q + t], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    base = np.concatenate(q + t).astype(np.uint8)
    qoff, toff = np.ascontiguousarray(offs[:n]), np.ascontiguousarray(offs[n:])
    qlen, tlen = np.ascontiguousarray(lens[:n].astype(np.int32)), np.ascontiguousarray(lens[n:].astype(np.int32))
    res = np.zeros((n, 3), dtype=np.int32)
    aln = (ksw2_amd.LocalAln * n)()
    rp = res.ctypes.data_as(ctypes.POINTER(ksw2_amd.LocalResult))

    def timed(fn):
        rc = fn()                                              # warm-up
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        out = np.array([(x.score, x.qb, x.qe, x.tb, x.te) for x in aln], dtype=np.int32) if align else res.copy()
        return times, out

    def pointer():
        if align:
            return L.ksw2amd_ll_align_batch(None, 5, mp.ctypes.data_as(i8p), gapo, gape, SCORE_ONLY, n, pairs, aln)
        return L.ksw2amd_ll_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp)

    rec = dict(workload=a.workload, mode="flat-align-coords" if align else "flat", pairs=n, cells=cells, arena_bytes=int(base.nbytes), ll_form=form,
               clock="library call only: pair array, arena, offsets, page-locking and device copy are built before it")
    ref = None
    if not a.no_compare:
        times, ref = timed(pointer)
        rec["pointer"] = dict(e2e_s=min(times), e2e_gcups=cells / min(times) / 1e9, e2e_all_s=times)
    ok = True
    for kind in (("host", "host-pinned", "device") if a.flat == "all" else (a.flat,)):
        f = ksw2_amd.LocalFlat()
        f.qoff, f.toff, f.qlen, f.tlen = qoff.ctypes.data, toff.ctypes.data, qlen.ctypes.data, tlen.ctypes.data
        f.base, f.on_device = base.ctypes.data, 0
        dev = None
        if kind == "host-pinned":
            lib._check(L.ksw2amd_host_register(base.ctypes.data, base.nbytes))
        elif kind == "device":
            dev = lib.device_copy(base)
            f.base, f.on_device = dev, 1

        def flat():
            if align:
                return L.ksw2amd_ll_align_batch_flat(None, 5, mp.ctypes.data_as(i8p), gapo, gape, SCORE_ONLY, n, ctypes.byref(f), aln)
            return L.ksw2amd_ll_batch_flat(5, mp.ctypes.data_as(i8p), gapo, gape, n, ctypes.byref(f), rp)
        times, got = timed(flat)
        if kind == "host-pinned":
            L.ksw2amd_host_unregister(base.ctypes.data)
        if dev is not None:
            lib.device_free(dev)
        same = None if ref is None else bool((got == ref).all())
        ok = ok and same is not False
        rec[kind] = dict(e2e_s=min(times), e2e_gcups=cells / min(times) / 1e9, e2e_all_s=times, equals_pointer_entry=same)
        if ref is not None:
            rec[kind]["speedup_over_pointer"] = rec["pointer"]["e2e_s"] / min(times)
    if not align:
        idx = np.linspace(0, n - 1, a.parity).astype(int)
        exp = u.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, gapo, gape)
        rec["parity_ok"] = bool((got[idx] == exp).all())
        ok = ok and rec["parity_ok"]
    if a.kstats:
        fwd, chk = kernel_ms(a.kstats, a.kbatches, "k2a_ll_kernel"), kernel_ms(a.kstats, a.kbatches, "k2a_ll_check_kernel")
        rec.update(fwd_kernel_ms=fwd, check_kernel_ms=chk, check_over_fwd=chk / fwd if fwd else None)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if ok else 1


def trace_batches(path, name, launches_per_batch):
    """per-batch kernel time (ms) of the dispatches whose name contains `name` in a rocprofv3 kernel_trace.csv, in dispatch order"""
    d = []
    with open(path) as f:
        for row in csv.DictReader(f):
            if name in row.get("Kernel_Name", ""):
                d.append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6))
    d = [x[1] for x in sorted(d)]
    k = max(1, launches_per_batch)
    return [sum(d[i:i + k]) for i in range(0, len(d) - k + 1, k)]


def main_sub(a, lib, q, t, mat, gapo, gape, cells, form):
    from tests import lls_util as ls
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res, res2, sub = (np.zeros((n, 3), dtype=np.int32) for _ in range(3))
    rp = lambda x, ty: x.ctypes.data_as(ctypes.POINTER(ty))

    def plain():
        return L.ksw2amd_ll_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp(res, ksw2_amd.LocalResult))

    def withsub():
        return L.ksw2amd_ll_sub_batch(5, mp.ctypes.data_as(i8p), gapo, gape, a.excl, n, pairs, rp(res2, ksw2_amd.LocalResult), rp(sub, ksw2_amd.LocalSub))

    def timed(fn, tag):
        os.environ["KSW2AMD_TRACE"] = "1"                      # the warm-up's form lines
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            lines = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tag in l]
        os.environ.pop("KSW2AMD_TRACE")                        # (the binding re-reads the environment in front of every call)
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return dict(e2e_s=min(times), e2e_all_s=times, pairs_per_s=n / min(times), e2e_gcups=cells / min(times) / 1e9, forms=lines)

    rec = dict(workload=a.workload, mode="sub", pairs=n, cells=cells, excl=a.excl, ll_form=form,
               pairs_changing_orientation=int(sum(len(x) > len(y) for x, y in zip(q, t))),
               clock="library call only: the pair array is built before it")
    rec["ll_batch"] = timed(plain, "ll: pairs")
    rec["ll_sub_batch"] = timed(withsub, "ll-sub:")
    rec["sub_over_plain_e2e"] = rec["ll_sub_batch"]["e2e_s"] / rec["ll_batch"]["e2e_s"]
    rec["res_equal"] = bool((res == res2).all())
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = ls.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, gapo, gape, a.excl)
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = bool((np.hstack([res2, sub])[idx] == exp).all())
    rec["score2_positive"] = int((sub[:, 0] > 0).sum())
    if a.ktrace:
        # launches per batch: one per kernel form that had tasks (packed, int32), as the form lines say
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        kp = trace_batches(a.ktrace, "k2a_ll_kernel", nl(rec["ll_batch"]["forms"][0]))[1:]        # [0]: the warm-up
        kf = trace_batches(a.ktrace, "k2a_ll_fsub_kernel", nl(rec["ll_sub_batch"]["forms"][0]))[1:]
        kr = trace_batches(a.ktrace, "k2a_ll_sub_kernel", nl(rec["ll_sub_batch"]["forms"][0]))[1:]
        ks = [x + y for x, y in zip(kf, kr)]
        rec["kernel"] = dict(ll_kernel_ms=kp, fsub_kernel_ms=kf, sub_kernel_ms=kr,
                             ll_kernel_spread=(max(kp) - min(kp)) / min(kp) if kp else None,
                             sub_over_plain=(sum(ks) / len(ks)) / (sum(kp) / len(kp)) if kp and ks else None,
                             note="k2a_ll_kernel of this build, same session (its code and register counts are the parent commit's)")
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["res_equal"] and rec["parity_ok"] else 1


def main_sg(a, lib, q, t, mat, gapo, gape, cells, form):
    from tests import sg_util as sg
    swap = [len(x) > len(y) for x, y in zip(q, t)]
    q, t = [y if w else x for x, y, w in zip(q, t, swap)], [x if w else y for x, y, w in zip(q, t, swap)]      # target >= query
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res, res2 = (np.zeros((n, 3), dtype=np.int32) for _ in range(2))
    rp = lambda x, ty: x.ctypes.data_as(ctypes.POINTER(ty))
    fns = dict(ll_batch=lambda: L.ksw2amd_ll_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp(res, ksw2_amd.LocalResult)),
               sg_batch=lambda: L.ksw2amd_sg_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp(res2, ksw2_amd.LocalResult)))
    tags = dict(ll_batch="ll: pairs", sg_batch="sg: pairs")
    forms = {}
    os.environ["KSW2AMD_TRACE"] = "1"                          # the warm-ups' form lines
    for name, fn in fns.items():
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            forms[name] = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tags[name] in l]
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
    os.environ.pop("KSW2AMD_TRACE")                            # (the binding re-reads the environment in front of every call)
    times = dict(ll_batch=[], sg_batch=[])
    for _ in range(a.reps):                                    # alternating: ll, sg, ll, sg, ...
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    rec = dict(workload=a.workload, mode="sg", pairs=n, cells=cells, ll_form=form, pairs_turned_round=int(sum(swap)),
               clock="library call only: the pair array is built before it; the two entries alternate batch by batch")
    for name in fns:
        ts = times[name]
        rec[name] = dict(e2e_s=min(ts), e2e_all_s=ts, pairs_per_s=n / min(ts), e2e_gcups=cells / min(ts) / 1e9, forms=forms[name])
    rec["sg_over_ll_e2e"] = rec["sg_batch"]["e2e_s"] / rec["ll_batch"]["e2e_s"]
    rec["ll_e2e_spread"] = (max(times["ll_batch"]) - min(times["ll_batch"])) / min(times["ll_batch"])
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = sg.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, gapo, gape, 5)
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = bool((res2[idx] == exp).all())
    rec["negative_scores"] = int((res2[:, 0] < 0).sum())
    if a.ktrace:
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        kl = trace_batches(a.ktrace, "k2a_ll_kernel", nl(forms["ll_batch"][0]))[1:]        # [0]: the warm-up
        ks = trace_batches(a.ktrace, "k2a_sg_kernel", nl(forms["sg_batch"][0]))[1:]
        rec["kernel"] = dict(ll_kernel_ms=kl, sg_kernel_ms=ks,
                             ll_kernel_spread=(max(kl) - min(kl)) / min(kl) if kl else None,
                             sg_over_ll=(sum(ks) / len(ks)) / (sum(kl) / len(kl)) if kl and ks else None,
                             ll_resident_gcups=cells / (sum(kl) / len(kl) * 1e-3) / 1e9 if kl else None,
                             sg_resident_gcups=cells / (sum(ks) / len(ks) * 1e-3) / 1e9 if ks else None)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["parity_ok"] else 1


def main_ov(a, lib, q, t, mat, gapo, gape, cells, form):
    """--ov: ksw2amd_ll_batch, ksw2amd_sg_batch and ksw2amd_ov_batch(ends = 3), alternating"""
    from tests import ov_util as ov
    ends = ksw2_amd.KSW2AMD_OV_QBEG | ksw2_amd.KSW2AMD_OV_QEND
    swap = [len(x) > len(y) for x, y in zip(q, t)]
    q, t = [y if w else x for x, y, w in zip(q, t, swap)], [x if w else y for x, y, w in zip(q, t, swap)]      # target >= query, as --sg
    n = len(q)
    L = lib.lib
    mpp = np.ascontiguousarray(mat, dtype=np.int8).ctypes.data_as(ctypes.POINTER(ctypes.c_int8))
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res = {k: np.zeros((n, 3), dtype=np.int32) for k in ("ll_batch", "sg_batch", "ov_batch")}
    rp = lambda x: x.ctypes.data_as(ctypes.POINTER(ksw2_amd.LocalResult))
    fns = dict(ll_batch=lambda: L.ksw2amd_ll_batch(5, mpp, gapo, gape, n, pairs, rp(res["ll_batch"])),
               sg_batch=lambda: L.ksw2amd_sg_batch(5, mpp, gapo, gape, n, pairs, rp(res["sg_batch"])),
               ov_batch=lambda: L.ksw2amd_ov_batch(5, mpp, gapo, gape, ends, n, pairs, rp(res["ov_batch"])))
    tags = dict(ll_batch="ll: pairs", sg_batch="sg: pairs", ov_batch="ov: pairs")
    forms = {}
    os.environ["KSW2AMD_TRACE"] = "1"                          # the warm-ups' form lines
    for name, fn in fns.items():
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            forms[name] = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tags[name] in l]
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
    os.environ.pop("KSW2AMD_TRACE")                            # (the binding re-reads the environment in front of every call)
    times = {k: [] for k in fns}
    for _ in range(a.reps):                                    # alternating: ll, sg, ov, ll, sg, ov, ...
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    rec = dict(workload=a.workload, mode="ov", ends=ends, pairs=n, cells=cells, ll_form=form, pairs_turned_round=int(sum(swap)),
               clock="library call only: the pair array is built before it; the three entries alternate batch by batch")
    for name in fns:
        ts = times[name]
        rec[name] = dict(e2e_s=min(ts), e2e_all_s=ts, pairs_per_s=n / min(ts), e2e_gcups=cells / min(ts) / 1e9, forms=forms[name])
    rec["ov_over_ll_e2e"] = rec["ov_batch"]["e2e_s"] / rec["ll_batch"]["e2e_s"]
    rec["ov_over_sg_e2e"] = rec["ov_batch"]["e2e_s"] / rec["sg_batch"]["e2e_s"]
    rec["ll_e2e_spread"] = (max(times["ll_batch"]) - min(times["ll_batch"])) / min(times["ll_batch"])
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = ov.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, (gapo, gape), ends, 5)
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = bool((res["ov_batch"][idx] == exp).all())
    rec["ends_in_last_row_off_the_corner"] = int((res["ov_batch"][:, 1] < np.array([len(x) - 1 for x in q])).sum())
    rec["scores_differing_from_sg"] = int((res["ov_batch"][:, 0] != res["sg_batch"][:, 0]).sum())
    if a.ktrace:
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        mean = lambda v: sum(v) / len(v)
        kl = trace_batches(a.ktrace, "k2a_ll_kernel", nl(forms["ll_batch"][0]))[1:]        # [0]: the warm-up
        ks = trace_batches(a.ktrace, "k2a_sg_kernel", nl(forms["sg_batch"][0]))[1:]
        ko = trace_batches(a.ktrace, "k2a_ov_kernel", nl(forms["ov_batch"][0]))[1:]
        rec["kernel"] = dict(ll_kernel_ms=kl, sg_kernel_ms=ks, ov_kernel_ms=ko,
                             ll_kernel_spread=(max(kl) - min(kl)) / min(kl) if kl else None,
                             ov_over_ll=mean(ko) / mean(kl) if kl and ko else None,
                             ov_over_sg=mean(ko) / mean(ks) if ks and ko else None,
                             ov_below_ll_by_more_than_the_spread=bool(max(ko) < min(kl) and (mean(kl) - mean(ko)) > (max(kl) - min(kl))) if kl and ko else None,
                             ov_resident_gcups=cells / (mean(ko) * 1e-3) / 1e9 if ko else None)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["parity_ok"] else 1


def main_sg_align(a, lib, q, t, mat, gapo, gape, cells, form):
    """--sg-align: ksw2amd_sg_batch, ksw2amd_sg_align_batch (SCORE_ONLY, and with CIGARs) and the by-hand pattern they replace, alternating"""
    from tests import sga_util as sga
    swap = [len(x) > len(y) for x, y in zip(q, t)]
    q, t = [y if w else x for x, y, w in zip(q, t, swap)], [x if w else y for x, y, w in zip(q, t, swap)]      # target >= query, as --sg
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res = np.zeros((n, 3), dtype=np.int32)
    alns = dict(sga_coords=(ksw2_amd.LocalAln * n)(), sga_cigar=(ksw2_amd.LocalAln * n)())      # CIGAR buffers are reused from batch to batch
    rp = lambda x, ty: x.ctypes.data_as(ctypes.POINTER(ty))
    hand = {}

    def sg_batch():
        return L.ksw2amd_sg_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp(res, ksw2_amd.LocalResult))

    def by_hand():
        """sg_batch, host reversal, ksw2amd_extz_batch for mqe_t, ksw2amd_extz_batch for the CIGAR; the time inside the three library calls
        and the host work between them are kept apart"""
        c = dict(lib=0.0, host=0.0)
        r = np.zeros((n, 3), dtype=np.int32)
        t0 = time.perf_counter()
        rc = L.ksw2amd_sg_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp(r, ksw2_amd.LocalResult))
        t1 = time.perf_counter()
        b1 = lib.make_batch([np.ascontiguousarray(x[::-1]) for x in q], [np.ascontiguousarray(y[te::-1]) for y, te in zip(t, r[:, 2])],
                            mat, gapo, gape, w=-1, zdrop=-1, flag=SCORE_ONLY)
        ez1 = (ksw2_amd.KswExtz * n)()
        t2 = time.perf_counter()
        rc |= L.ksw2amd_extz_batch(None, ctypes.byref(b1.sc), n, b1.pairs, ez1)
        t3 = time.perf_counter()
        tb = [int(te) - ez1[i].mqe_t if ez1[i].mqe > -(gapo + len(q[i]) * gape) else int(te) + 1 for i, te in enumerate(r[:, 2])]
        live = [i for i in range(n) if tb[i] <= r[i, 2]]
        b2 = lib.make_batch([q[i] for i in live], [t[i][tb[i]:r[i, 2] + 1] for i in live], mat, gapo, gape, w=-1, zdrop=-1, flag=GENERIC_SC)
        ez2 = (ksw2_amd.KswExtz * max(len(live), 1))()
        t4 = time.perf_counter()
        rc |= L.ksw2amd_extz_batch(None, ctypes.byref(b2.sc), len(live), b2.pairs, ez2)
        t5 = time.perf_counter()
        c["lib"], c["host"] = (t1 - t0) + (t3 - t2) + (t5 - t4), (t2 - t1) + (t4 - t3)
        hand.update(tb=tb, live=live, cigar={i: [int(ez2[k].cigar[j]) for j in range(ez2[k].n_cigar)] for k, i in enumerate(live) if k % 97 == 0},
                    lib_s=hand.get("lib_s", []) + [c["lib"]], host_s=hand.get("host_s", []) + [c["host"]])
        for k in range(len(live)):
            ksw2_amd._libc.free(ctypes.cast(ez2[k].cigar, ctypes.c_void_p))
        return rc

    fns = dict(sg_batch=sg_batch,
               sga_coords=lambda: L.ksw2amd_sg_align_batch(None, 5, mp.ctypes.data_as(i8p), gapo, gape, SCORE_ONLY, n, pairs, alns["sga_coords"]),
               sga_cigar=lambda: L.ksw2amd_sg_align_batch(None, 5, mp.ctypes.data_as(i8p), gapo, gape, 0, n, pairs, alns["sga_cigar"]),
               by_hand=by_hand)
    tags = dict(sg_batch="sg: pairs", sga_coords="sga", sga_cigar="sga", by_hand="sg: pairs")
    forms = {}
    os.environ["KSW2AMD_TRACE"] = "1"                          # the warm-ups' form lines
    for name, fn in fns.items():
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            forms[name] = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tags[name] in l]
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
    os.environ.pop("KSW2AMD_TRACE")
    hand["lib_s"], hand["host_s"] = [], []                     # (the warm-up's)
    times = {k: [] for k in fns}
    for _ in range(a.reps):                                    # alternating: sg, coords, cigar, by hand, sg, ...
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    times["by_hand"] = hand["lib_s"]                           # the three library calls only, like the others
    rec = dict(workload=a.workload, mode="sg-align", pairs=n, cells=cells, ll_form=form, pairs_turned_round=int(sum(swap)),
               clock="library calls only: pair and result arrays are built before them; the four alternate batch by batch; by_hand = the sum of "
                     "its three library calls, the host reversal and the pair arrays between them in by_hand_host_s")
    for name in fns:
        ts = times[name]
        rec[name] = dict(e2e_s=min(ts), e2e_all_s=ts, pairs_per_s=n / min(ts), e2e_gcups=cells / min(ts) / 1e9, forms=forms[name][:4])
    rec["by_hand_host_s"] = hand["host_s"]
    rec["sg_e2e_spread"] = (max(times["sg_batch"]) - min(times["sg_batch"])) / min(times["sg_batch"])
    al = alns["sga_cigar"]
    rec["empty_intervals"] = int(sum(al[i].tb > al[i].te for i in range(n)))
    rec["mean_interval"] = float(np.mean([al[i].te - al[i].tb + 1 for i in range(n)]))
    rec["by_hand_agrees"] = bool(all(hand["tb"][i] == al[i].tb and res[i, 2] == al[i].te and res[i, 0] == al[i].score for i in range(n))
                                 and all([int(al[i].cigar[j]) for j in range(al[i].n_cigar)] == c for i, c in hand["cigar"].items()))
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = sga.oracle_cells([q[i] for i in idx], [t[i] for i in idx], mat, gapo, gape, 5)
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = bool(all(tuple(exp[k]) == (al[i].score, al[i].qb, al[i].qe, al[i].tb, al[i].te) for k, i in enumerate(idx))
                            and all(tuple(exp[k]) == tuple(getattr(alns["sga_coords"][i], f) for f in ("score", "qb", "qe", "tb", "te")) for k, i in enumerate(idx)))
    if a.ktrace:
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        per = nl(forms["sg_batch"][0])
        kf = trace_batches(a.ktrace, "k2a_sg_kernel", per)     # in dispatch order: warm-ups sg, coords, cigar, by hand, then reps x the same four
        kr = trace_batches(a.ktrace, "k2a_sg_rev_kernel", per)
        fwd_sg = [kf[4 + 4 * r] for r in range(a.reps) if 4 + 4 * r < len(kf)]                 # the forward kernel of the sg_batch batches
        fwd_all = kf[4:]
        rev = kr[2:]                                                                         # coords, cigar alternating
        rec["kernel"] = dict(sg_kernel_ms_of_sg_batch=fwd_sg, sg_kernel_ms_all=fwd_all, sg_rev_kernel_ms=rev,
                             sg_kernel_spread=(max(fwd_all) - min(fwd_all)) / min(fwd_all) if fwd_all else None,
                             rev_over_fwd=(sum(rev) / len(rev)) / (sum(fwd_all) / len(fwd_all)) if rev and fwd_all else None)
    for x in alns["sga_cigar"]:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["parity_ok"] and rec["by_hand_agrees"] else 1


def main_ov_align(a, lib, q, t, mat, gapo, gape, cells, form):
    """--ov-align: the sg / sgd / ov / ovd align entries with SCORE_ONLY, ov_align with CIGARs and the by-hand pattern, alternating"""
    from tests import ova_util as ova
    swap = [len(x) > len(y) for x, y in zip(q, t)]
    q, t = [y if w else x for x, y, w in zip(q, t, swap)], [x if w else y for x, y, w in zip(q, t, swap)]      # target >= query, as --sg
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    mpp = mp.ctypes.data_as(i8p)
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    go2, ge2, ends = 24, 1, 3
    names = ("sga_coords", "sgda_coords", "ova_coords", "ovda_coords", "ova_cigar")
    alns = {k: (ksw2_amd.LocalAln * n)() for k in names}       # CIGAR buffers are reused from batch to batch
    rp = lambda x, ty: x.ctypes.data_as(ctypes.POINTER(ty))
    cost = lambda l: gapo + l * gape
    hand = {}

    def by_hand():
        """ov_batch, host reversal of both prefixes, ksw2amd_extz_batch for mqe / mte, the two corner constants, ksw2amd_extz_batch for the
        CIGAR; the time inside the three library calls and the host work between them are kept apart"""
        r = np.zeros((n, 3), dtype=np.int32)
        t0 = time.perf_counter()
        rc = L.ksw2amd_ov_batch(5, mpp, gapo, gape, ends, n, pairs, rp(r, ksw2_amd.LocalResult))
        t1 = time.perf_counter()
        b1 = lib.make_batch([np.ascontiguousarray(x[qe::-1]) for x, qe in zip(q, r[:, 1])], [np.ascontiguousarray(y[te::-1]) for y, te in zip(t, r[:, 2])],
                            mat, gapo, gape, w=-1, zdrop=-1, flag=SCORE_ONLY)
        ez1 = (ksw2_amd.KswExtz * n)()
        t2 = time.perf_counter()
        rc |= L.ksw2amd_extz_batch(None, ctypes.byref(b1.sc), n, b1.pairs, ez1)
        t3 = time.perf_counter()
        st, sc = [], []
        for i in range(n):                                     # (tb, qb): a start some caller would take -- its ties are not the entry's
            qe, te = int(r[i, 1]), int(r[i, 2])
            c = [(-cost(qe + 1), te + 1, 0), (ez1[i].mqe, te - ez1[i].mqe_t, 0), (-cost(te + 1), 0, qe + 1), (ez1[i].mte, 0, qe - ez1[i].mte_q)]
            best = max(c, key=lambda x: x[0])
            sc.append(best[0]); st.append(best[1:])
        live = [i for i in range(n) if st[i][0] <= r[i, 2] and st[i][1] <= r[i, 1]]
        b2 = lib.make_batch([q[i][st[i][1]:r[i, 1] + 1] for i in live], [t[i][st[i][0]:r[i, 2] + 1] for i in live], mat, gapo, gape, w=-1, zdrop=-1, flag=GENERIC_SC)
        ez2 = (ksw2_amd.KswExtz * max(len(live), 1))()
        t4 = time.perf_counter()
        rc |= L.ksw2amd_extz_batch(None, ctypes.byref(b2.sc), len(live), b2.pairs, ez2)
        t5 = time.perf_counter()
        hand.update(score=sc, fwd=r, global_ok=all(ez2[k].score == sc[i] for k, i in enumerate(live)),
                    lib_s=hand.get("lib_s", []) + [(t1 - t0) + (t3 - t2) + (t5 - t4)], host_s=hand.get("host_s", []) + [(t2 - t1) + (t4 - t3)])
        for k in range(len(live)):
            ksw2_amd._libc.free(ctypes.cast(ez2[k].cigar, ctypes.c_void_p))
        return rc

    fns = dict(sga_coords=lambda: L.ksw2amd_sg_align_batch(None, 5, mpp, gapo, gape, SCORE_ONLY, n, pairs, alns["sga_coords"]),
               sgda_coords=lambda: L.ksw2amd_sgd_align_batch(None, 5, mpp, gapo, gape, go2, ge2, SCORE_ONLY, n, pairs, alns["sgda_coords"]),
               ova_coords=lambda: L.ksw2amd_ov_align_batch(None, 5, mpp, gapo, gape, ends, SCORE_ONLY, n, pairs, alns["ova_coords"]),
               ovda_coords=lambda: L.ksw2amd_ovd_align_batch(None, 5, mpp, gapo, gape, go2, ge2, ends, SCORE_ONLY, n, pairs, alns["ovda_coords"]),
               ova_cigar=lambda: L.ksw2amd_ov_align_batch(None, 5, mpp, gapo, gape, ends, 0, n, pairs, alns["ova_cigar"]),
               by_hand=by_hand)
    tags = dict(sga_coords="sga", sgda_coords="sgda", ova_coords="ova", ovda_coords="ovda", ova_cigar="ova", by_hand="ov: pairs")
    forms = {}
    os.environ["KSW2AMD_TRACE"] = "1"                          # the warm-ups' form lines
    for name, fn in fns.items():
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            forms[name] = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if "] " + tags[name] in l]
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
    os.environ.pop("KSW2AMD_TRACE")
    hand["lib_s"], hand["host_s"] = [], []                     # (the warm-up's)
    times = {k: [] for k in fns}
    for _ in range(a.reps):                                    # alternating
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    times["by_hand"] = hand["lib_s"]                           # the three library calls only, like the others
    rec = dict(workload=a.workload, mode="ov-align", pairs=n, cells=cells, ll_form=form, ends=ends, costs2=[go2, ge2], pairs_turned_round=int(sum(swap)),
               clock="library calls only: pair and result arrays are built before them; the six alternate batch by batch; by_hand = the sum of "
                     "its three library calls, the host reversal and the pair arrays between them in by_hand_host_s")
    for name in fns:
        ts = times[name]
        rec[name] = dict(e2e_s=min(ts), e2e_all_s=ts, e2e_spread=(max(ts) - min(ts)) / min(ts), pairs_per_s=n / min(ts), e2e_gcups=cells / min(ts) / 1e9,
                         forms=forms[name][:4])
    rec["by_hand_host_s"] = hand["host_s"]
    al = alns["ova_cigar"]
    rec["empty_target_intervals"] = int(sum(al[i].tb > al[i].te for i in range(n)))
    rec["empty_query_intervals"] = int(sum(al[i].qb > al[i].qe for i in range(n)))
    rec["starts_in_row_0"] = int(sum(al[i].qb > 0 for i in range(n)))
    rec["mean_target_interval"] = float(np.mean([al[i].te - al[i].tb + 1 for i in range(n)]))
    rec["mean_rectangle_cells"] = float(np.mean([(al[i].te + 1) * (al[i].qe + 1) for i in range(n)]))
    rec["by_hand_agrees"] = bool(hand["global_ok"] and all(hand["score"][i] == al[i].score and hand["fwd"][i, 1] == al[i].qe and hand["fwd"][i, 2] == al[i].te
                                                          for i in range(n)))
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    F = ("score", "qb", "qe", "tb", "te")
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = True
    for key, costs in (("ova_coords", (gapo, gape)), ("ova_cigar", (gapo, gape)), ("ovda_coords", (gapo, gape, go2, ge2))):
        exp = ova.oracle_cells([q[i] for i in idx], [t[i] for i in idx], mat, costs, ends, 5)
        rec["parity_ok"] = bool(rec["parity_ok"] and all(tuple(exp[k]) == tuple(getattr(alns[key][i], f) for f in F) for k, i in enumerate(idx)))
    if a.ktrace:
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        per = nl(forms["ova_coords"][0])
        k = {name: trace_batches(a.ktrace, "k2a_%s_kernel" % name, per) for name in ("sg", "sg_rev", "sgd", "sgd_rev", "ov", "ov_rev", "ovd", "ovd_rev")}
        skip = dict(sg_rev=1, sgd_rev=1, ov_rev=2, ovd_rev=1)  # the warm-ups
        kr = {name: k[name][skip[name]:] for name in skip}
        spread = lambda x: (max(x) - min(x)) / min(x) if x else None
        mean = lambda x: sum(x) / len(x) if x else None
        rec["kernel"] = dict({name + "_kernel_ms": v for name, v in kr.items()}, **{name + "_spread": spread(v) for name, v in kr.items()})
        rec["kernel"].update(sg_kernel_ms=k["sg"][1:], sgd_kernel_ms=k["sgd"][1:], ov_kernel_ms=k["ov"][3:], ovd_kernel_ms=k["ovd"][1:],
                             ov_rev_over_sg_rev=mean(kr["ov_rev"]) / mean(kr["sg_rev"]) if kr["ov_rev"] and kr["sg_rev"] else None,
                             ovd_rev_over_sgd_rev=mean(kr["ovd_rev"]) / mean(kr["sgd_rev"]) if kr["ovd_rev"] and kr["sgd_rev"] else None,
                             ov_rev_over_ov=mean(kr["ov_rev"]) / mean(k["ov"][3:]) if kr["ov_rev"] and k["ov"][3:] else None)
    for x in alns["ova_cigar"]:
        ksw2_amd._libc.free(ctypes.cast(x.cigar, ctypes.c_void_p))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["parity_ok"] and rec["by_hand_agrees"] else 1


def main_sgd(a, lib, q, t, mat, gapo, gape, cells, form):
    """--sgd / --sgd-align: the two-piece semi-global entries beside ksw2amd_lld_batch (and ksw2amd_sg_batch), alternating"""
    from tests import sgd_util as sd
    swap = [len(x) > len(y) for x, y in zip(q, t)]
    q, t = [y if w else x for x, y, w in zip(q, t, swap)], [x if w else y for x, y, w in zip(q, t, swap)]      # target >= query, as --sg
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    mpp = mp.ctypes.data_as(i8p)
    gapo2, gape2 = 24, 1
    costs = (gapo, gape, gapo2, gape2)
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res = {k: np.zeros((n, 3), dtype=np.int32) for k in ("lld_batch", "sg_batch", "sgd_batch")}
    alns = {k: (ksw2_amd.LocalAln * n)() for k in ("sgda_coords", "sgda_cigar")} if a.sgd_align else {}
    rp = lambda x: x.ctypes.data_as(ctypes.POINTER(ksw2_amd.LocalResult))
    fns = dict(lld_batch=lambda: L.ksw2amd_lld_batch(5, mpp, gapo, gape, gapo2, gape2, n, pairs, rp(res["lld_batch"])))
    tags = dict(lld_batch="lld: pairs")
    if a.sgd_align:
        fns.update(sgda_coords=lambda: L.ksw2amd_sgd_align_batch(None, 5, mpp, gapo, gape, gapo2, gape2, SCORE_ONLY, n, pairs, alns["sgda_coords"]),
                   sgda_cigar=lambda: L.ksw2amd_sgd_align_batch(None, 5, mpp, gapo, gape, gapo2, gape2, 0, n, pairs, alns["sgda_cigar"]))
        tags.update(sgda_coords="sgda: pairs", sgda_cigar="sgda: pairs")
    else:
        fns.update(sg_batch=lambda: L.ksw2amd_sg_batch(5, mpp, gapo, gape, n, pairs, rp(res["sg_batch"])),
                   sgd_batch=lambda: L.ksw2amd_sgd_batch(5, mpp, gapo, gape, gapo2, gape2, n, pairs, rp(res["sgd_batch"])))
        tags.update(sg_batch="sg: pairs", sgd_batch="sgd: pairs")
    forms = {}
    os.environ["KSW2AMD_TRACE"] = "1"                          # the warm-ups' form lines
    for name, fn in fns.items():
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            forms[name] = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tags[name] in l]
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
    os.environ.pop("KSW2AMD_TRACE")                            # (the binding re-reads the environment in front of every call)
    times = {name: [] for name in fns}
    for _ in range(a.reps):                                    # alternating batch by batch
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    rec = dict(workload=a.workload, mode="sgd-align" if a.sgd_align else "sgd", pairs=n, cells=cells, ll_form=form, costs=list(costs),
               pairs_turned_round=int(sum(swap)), clock="library call only: the pair array is built before it; the entries alternate batch by batch")
    for name in fns:
        ts = times[name]
        rec[name] = dict(e2e_s=min(ts), e2e_all_s=ts, pairs_per_s=n / min(ts), e2e_gcups=cells / min(ts) / 1e9, forms=forms[name])
    rec["lld_e2e_spread"] = (max(times["lld_batch"]) - min(times["lld_batch"])) / min(times["lld_batch"])
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = sd.oracle_cells([q[i] for i in idx], [t[i] for i in idx], mat, costs, 5)
    rec["parity_sample"] = int(len(idx))
    if a.sgd_align:
        got = [[[x.score, x.qb, x.qe, x.tb, x.te] for x in (alns[k][int(i)] for i in idx)] for k in ("sgda_coords", "sgda_cigar")]
        rec["parity_ok"] = bool(got[0] == exp.tolist() and got[1] == exp.tolist())
        rec["empty_intervals"] = int(sum(x.tb > x.te for x in alns["sgda_coords"]))
    else:
        rec["parity_ok"] = bool((res["sgd_batch"][idx] == exp[:, [0, 2, 4]]).all())
        rec["scores_differing_from_sg"] = int((res["sgd_batch"][:, 0] != res["sg_batch"][:, 0]).sum())
    if a.ktrace:
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        first = "sgda_coords" if a.sgd_align else "sgd_batch"
        kl = trace_batches(a.ktrace, "k2a_lld_kernel", nl(forms["lld_batch"][0]))[1:]        # [0]: the warm-up
        kd = trace_batches(a.ktrace, "k2a_sgd_kernel", nl(forms[first][0]))
        kr = trace_batches(a.ktrace, "k2a_sgd_rev_kernel", nl(forms[first][0]))
        kd, kr = kd[(2 if a.sgd_align else 1):], kr[2:]       # the warm-ups: one per entry that launches the kernel
        ks = trace_batches(a.ktrace, "k2a_sg_kernel", nl(forms["sg_batch"][0]))[1:] if not a.sgd_align else []
        mean = lambda x: sum(x) / len(x) if x else None
        rec["kernel"] = dict(lld_kernel_ms=kl, sg_kernel_ms=ks, sgd_kernel_ms=kd, sgd_rev_kernel_ms=kr,
                             lld_kernel_spread=(max(kl) - min(kl)) / min(kl) if kl else None,
                             sgd_over_lld=mean(kd) / mean(kl) if kl and kd else None,
                             sgd_over_sg=mean(kd) / mean(ks) if ks and kd else None,
                             sgd_rev_over_sgd=mean(kr) / mean(kd) if kr and kd else None)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["parity_ok"] else 1


def main_dual(a, lib, q, t, mat, gapo, gape, cells, form):
    from tests import lld_util as ld
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    gapo2, gape2 = 24, 1
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res, res2 = (np.zeros((n, 3), dtype=np.int32) for _ in range(2))
    aln, aln2 = ((ksw2_amd.LocalAln * n)() for _ in range(2))   # CIGAR buffers are reused from batch to batch
    flag = SCORE_ONLY if a.align == "coords" else 0
    rp = lambda x: x.ctypes.data_as(ctypes.POINTER(ksw2_amd.LocalResult))

    def single():
        if a.align:
            return L.ksw2amd_ll_align_batch(None, 5, mp.ctypes.data_as(i8p), gapo, gape, flag, n, pairs, aln)
        return L.ksw2amd_ll_batch(5, mp.ctypes.data_as(i8p), gapo, gape, n, pairs, rp(res))

    def dual():
        if a.align:
            return L.ksw2amd_lld_align_batch(None, 5, mp.ctypes.data_as(i8p), gapo, gape, gapo2, gape2, flag, n, pairs, aln2)
        return L.ksw2amd_lld_batch(5, mp.ctypes.data_as(i8p), gapo, gape, gapo2, gape2, n, pairs, rp(res2))

    def timed(fn, tag):
        os.environ["KSW2AMD_TRACE"] = "1"                      # the warm-up's form lines
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            lines = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tag in l]
        os.environ.pop("KSW2AMD_TRACE")
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return dict(e2e_s=min(times), e2e_all_s=times, e2e_spread=(max(times) - min(times)) / min(times), pairs_per_s=n / min(times),
                    e2e_gcups=cells / min(times) / 1e9, forms=lines)

    rec = dict(workload=a.workload, mode="dual" + ("-align-" + a.align if a.align else ""), pairs=n, cells=cells, costs=[gapo, gape, gapo2, gape2],
               ll_form=form, clock="library call only: the pair array is built before it")
    one, two = ("ll_align_batch", "lld_align_batch") if a.align else ("ll_batch", "lld_batch")
    rec[one] = timed(single, "ll: pairs")
    rec[two] = timed(dual, "lld: pairs")
    rec["dual_over_single_e2e"] = rec[two]["e2e_s"] / rec[one]["e2e_s"]
    if a.align:
        res = np.array([(x.score, x.qe, x.te) for x in aln], dtype=np.int32)
        res2 = np.array([(x.score, x.qe, x.te) for x in aln2], dtype=np.int32)
    rec["scores_changed_by_second_piece"] = int((res[:, 0] != res2[:, 0]).sum())
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = ld.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, (gapo, gape, gapo2, gape2))
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = bool((res2[idx] == exp).all())
    if a.ktrace:
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        k1 = trace_batches(a.ktrace, "k2a_ll_kernel", nl(rec[one]["forms"][0]))[1:]            # [0]: the warm-up
        k2 = trace_batches(a.ktrace, "k2a_lld_kernel", nl(rec[two]["forms"][0]))[1:]
        kern = dict(ll_kernel_ms=k1, lld_kernel_ms=k2)
        if a.align:
            r1 = trace_batches(a.ktrace, "k2a_ll_rev_kernel", nl(rec[one]["forms"][0]))[1:]
            r2 = trace_batches(a.ktrace, "k2a_lld_rev_kernel", nl(rec[two]["forms"][0]))[1:]
            kern.update(ll_rev_kernel_ms=r1, lld_rev_kernel_ms=r2, rev_dual_over_single=(sum(r2) / len(r2)) / (sum(r1) / len(r1)) if r1 and r2 else None)
        kern.update(ll_kernel_spread=(max(k1) - min(k1)) / min(k1) if k1 else None,
                    dual_over_single=(sum(k2) / len(k2)) / (sum(k1) / len(k1)) if k1 and k2 else None,
                    note="k2a_ll_kernel of this build, same session (its code and register counts are the parent commit's)")
        rec["kernel"] = kern
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["parity_ok"] else 1


def main_dual_sub(a, lib, q, t, mat, gapo, gape, cells, form):
    from tests import llds_util as lx
    n = len(q)
    L = lib.lib
    i8p = ctypes.POINTER(ctypes.c_int8)
    mp = np.ascontiguousarray(mat, dtype=np.int8)
    gapo2, gape2 = 24, 1
    pairs, keep = lib.local_pairs(q, t)                        # outside the clock
    res, res2, sub = (np.zeros((n, 3), dtype=np.int32) for _ in range(3))
    rp = lambda x, ty: x.ctypes.data_as(ctypes.POINTER(ty))

    def plain():
        return L.ksw2amd_lld_batch(5, mp.ctypes.data_as(i8p), gapo, gape, gapo2, gape2, n, pairs, rp(res, ksw2_amd.LocalResult))

    def withsub():
        return L.ksw2amd_lld_sub_batch(5, mp.ctypes.data_as(i8p), gapo, gape, gapo2, gape2, a.excl, n, pairs, rp(res2, ksw2_amd.LocalResult),
                                       rp(sub, ksw2_amd.LocalSub))

    def timed(fn, tag):
        os.environ["KSW2AMD_TRACE"] = "1"                      # the warm-up's form lines
        err_fd = os.dup(2)
        with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
            os.dup2(tr.fileno(), 2)
            try:
                rc = fn()
            finally:
                os.dup2(err_fd, 2)
                os.close(err_fd)
            tr.seek(0)
            lines = [re.sub(r"^\[ksw2_amd\] ", "", l.strip()) for l in tr.read().splitlines() if tag in l]
        os.environ.pop("KSW2AMD_TRACE")                        # (the binding re-reads the environment in front of every call)
        if rc != 0:
            raise SystemExit("library error %d: %s" % (rc, lib.last_error()))
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
        return dict(e2e_s=min(times), e2e_all_s=times, e2e_spread=(max(times) - min(times)) / min(times), pairs_per_s=n / min(times),
                    e2e_gcups=cells / min(times) / 1e9, forms=lines)

    rec = dict(workload=a.workload, mode="dual-sub", pairs=n, cells=cells, costs=[gapo, gape, gapo2, gape2], excl=a.excl, ll_form=form,
               pairs_changing_orientation=int(sum(len(x) > len(y) for x, y in zip(q, t))),
               clock="library call only: the pair array is built before it")
    rec["lld_batch"] = timed(plain, "lld: pairs")
    rec["lld_sub_batch"] = timed(withsub, "lld-sub:")
    rec["sub_over_plain_e2e"] = rec["lld_sub_batch"]["e2e_s"] / rec["lld_batch"]["e2e_s"]
    rec["res_equal"] = bool((res == res2).all())
    idx = np.linspace(0, n - 1, a.parity).astype(int)
    exp = lx.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, (gapo, gape, gapo2, gape2), a.excl)
    rec["parity_sample"] = int(len(idx))
    rec["parity_ok"] = bool((np.hstack([res2, sub])[idx] == exp).all())
    rec["score2_positive"] = int((sub[:, 0] > 0).sum())
    if a.ktrace:
        # launches per batch: one per kernel form that had tasks (packed, int32), as the form lines say
        def nl(line):
            return sum(int(x) > 0 for x in re.findall(r"(?:pk|int32)_tasks=(\d+)", line))
        kp = trace_batches(a.ktrace, "k2a_lld_kernel", nl(rec["lld_batch"]["forms"][0]))[1:]          # [0]: the warm-up
        kf = trace_batches(a.ktrace, "k2a_lld_fsub_kernel", nl(rec["lld_sub_batch"]["forms"][0]))[1:]
        kr = trace_batches(a.ktrace, "k2a_ll_sub_kernel", nl(rec["lld_sub_batch"]["forms"][0]))[1:]
        ks = [x + y for x, y in zip(kf, kr)]
        rec["kernel"] = dict(lld_kernel_ms=kp, lld_fsub_kernel_ms=kf, sub_kernel_ms=kr,
                             lld_kernel_spread=(max(kp) - min(kp)) / min(kp) if kp else None,
                             sub_over_plain=(sum(ks) / len(ks)) / (sum(kp) / len(kp)) if kp and ks else None,
                             fsub_over_plain=(sum(kf) / len(kf)) / (sum(kp) / len(kp)) if kp and kf else None,
                             note="k2a_lld_kernel of this build, same session (its code and register counts are the parent commit's)")
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
    return 0 if rec["res_equal"] and rec["parity_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parity", type=int, default=4)
    ap.add_argument("--kstats", default=None)
    ap.add_argument("--kbatches", type=int, default=2)
    ap.add_argument("--form", default=None, help="KSW2AMD_LL_FORM (default: 0 for D, the library's default otherwise)")
    ap.add_argument("--align", choices=("coords", "cigar"), default=None, help="ksw2amd_ll_align_batch: start cells only, or with CIGARs")
    ap.add_argument("--baseline", action="store_true", help="with --align: the three-call pattern on the public API instead")
    ap.add_argument("--no-compare", action="store_true", help="with --align: skip the other path (a profiled run then holds 1 + reps batches of one path only)")
    ap.add_argument("--flat", choices=("host", "host-pinned", "device", "all"), default=None,
                    help="ksw2amd_ll_batch_flat / _align_batch_flat from one arena against the pointer entry, library calls only in the clock")
    ap.add_argument("--sub", action="store_true", help="ksw2amd_ll_sub_batch beside ksw2amd_ll_batch on the same pair array, library calls only in the clock")
    ap.add_argument("--dual", action="store_true", help="ksw2amd_lld_batch under (4, 2, 24, 1) beside ksw2amd_ll_batch under (4, 2); with --align the align entries; with --sub ksw2amd_lld_sub_batch beside ksw2amd_lld_batch")
    ap.add_argument("--sg", action="store_true", help="ksw2amd_sg_batch beside ksw2amd_ll_batch on the same pair array (target >= query), alternating, library calls only in the clock")
    ap.add_argument("--sg-align", action="store_true", help="ksw2amd_sg_batch, ksw2amd_sg_align_batch (SCORE_ONLY and with CIGARs) and the by-hand pattern (sg_batch, host reversal, two ksw2amd_extz_batch calls) on the same pair array, alternating")
    ap.add_argument("--sgd", action="store_true", help="ksw2amd_sgd_batch under (4, 2, 24, 1) beside ksw2amd_lld_batch and ksw2amd_sg_batch on the pair array of --sg, alternating, library calls only in the clock")
    ap.add_argument("--sgd-align", action="store_true", help="ksw2amd_lld_batch and ksw2amd_sgd_align_batch (SCORE_ONLY and with CIGARs) on the same pair array, alternating")
    ap.add_argument("--ov", action="store_true", help="ksw2amd_ov_batch with both query ends free beside ksw2amd_ll_batch and ksw2amd_sg_batch on the pair array of --sg, alternating, library calls only in the clock")
    ap.add_argument("--ov-align", action="store_true", help="ksw2amd_sg_align_batch / sgd / ov / ovd with SCORE_ONLY, ksw2amd_ov_align_batch with CIGARs and the by-hand pattern (ov_batch, host reversal, two ksw2amd_extz_batch calls) on the pair array of --sg, alternating")
    ap.add_argument("--excl", type=int, default=-1, help="with --sub: the excluded rows on either side of te (-1: ceil(score / smax))")
    ap.add_argument("--ktrace", default=None, help="with --sub: kernel_trace.csv of a rocprofv3 --kernel-trace run of the same command")
    ap.add_argument("--pairs", type=int, default=0, help="only the first N pairs of the workload")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    q, t = workload(a.workload, rng)
    if a.pairs > 0:
        q, t = q[:a.pairs], t[:a.pairs]
    mat = u.simple_mat(5, 2, 4, -1)
    gapo, gape = 4, 2
    cells = float(sum(len(x) * len(y) for x, y in zip(q, t)))
    form = a.form if a.form is not None else ("0" if a.workload == "D" else None)
    if form is not None:
        os.environ["KSW2AMD_LL_FORM"] = form
    lib = ksw2_amd.library()
    if a.ov_align:
        return main_ov_align(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.ov:
        return main_ov(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.sgd or a.sgd_align:
        return main_sgd(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.sg_align:
        return main_sg_align(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.sg:
        return main_sg(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.dual and a.sub:
        return main_dual_sub(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.dual:
        return main_dual(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.sub:
        return main_sub(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.flat:
        return main_flat(a, lib, q, t, mat, gapo, gape, cells, form)
    if a.align:
        return main_align(a, lib, q, t, mat, gapo, gape, cells, form)
    os.environ["KSW2AMD_TRACE"] = "1"                      # the form line on stderr (pk_tasks / int32_tasks)
    err_fd = os.dup(2)
    with open(os.devnull if a.out is None else a.out + ".trace", "w+") as tr:
        os.dup2(tr.fileno(), 2)
        try:
            res = lib.ll_batch(q, t, mat, gapo, gape)    # warm-up
        finally:
            os.dup2(err_fd, 2)
            os.close(err_fd)
        tr.seek(0)
        trace = [l.strip() for l in tr.read().splitlines() if "ll: pairs" in l]
    os.environ.pop("KSW2AMD_TRACE")
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = lib.ll_batch(q, t, mat, gapo, gape)
        times.append(time.perf_counter() - t0)
    idx = np.linspace(0, len(q) - 1, a.parity).astype(int)
    exp = u.oracle_batch([q[i] for i in idx], [t[i] for i in idx], mat, gapo, gape)
    ok = bool((res[idx] == exp).all())
    rec = dict(workload=a.workload, pairs=len(q), cells=cells, e2e_s=min(times), e2e_gcups=cells / min(times) / 1e9,
               e2e_all_s=times, parity_sample=int(len(idx)), parity_ok=ok, max_score=int(res[:, 0].max()),
               forms=[re.sub(r"^\[ksw2_amd\] ll: ", "", l) for l in trace], ll_form=form)
    if a.kstats:
        ms = kernel_ms(a.kstats, a.kbatches)
        rec.update(kernel_ms=ms, resident_gcups=cells / (ms * 1e-3) / 1e9)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if ok else 1


def main_align(a, lib, q, t, mat, gapo, gape, cells, form):
    cigar = a.align == "cigar"
    fn = align_baseline if a.baseline else align_new
    res = fn(lib, q, t, mat, gapo, gape, cigar)                                  # warm-up
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = fn(lib, q, t, mat, gapo, gape, cigar)
        times.append(time.perf_counter() - t0)
    ok = None
    if not a.no_compare:                                                           # outside the clock: both ways agree
        ok = res == (align_new if a.baseline else align_baseline)(lib, q, t, mat, gapo, gape, cigar)
    rev_cells = float(sum((r[2] + 1) * (r[4] + 1) for r in res if r[0] > 0))
    rec = dict(workload=a.workload, mode="align-" + a.align, path="baseline" if a.baseline else "ll_align_batch", pairs=len(q), cells=cells,
               rev_cells=rev_cells, e2e_s=min(times), e2e_gcups=cells / min(times) / 1e9, e2e_all_s=times, agrees_with_other_path=ok,
               cigar_ops=int(sum(len(r[5]) for r in res)), ll_form=form)
    if a.kstats:
        fwd, rev = kernel_ms(a.kstats, a.kbatches, "k2a_ll_kernel"), kernel_ms(a.kstats, a.kbatches, "k2a_ll_rev_kernel")
        allk = kernel_ms(a.kstats, a.kbatches, "")
        rec.update(fwd_kernel_ms=fwd, rev_kernel_ms=rev, rev_over_fwd=rev / fwd if fwd else None, cigar_stage_kernel_ms=allk - fwd - rev,
                   cigar_stage_share_of_e2e=(allk - fwd - rev) * 1e-3 / min(times),
                   fwd_resident_gcups=cells / (fwd * 1e-3) / 1e9 if fwd else None, rev_resident_gcups=rev_cells / (rev * 1e-3) / 1e9 if rev else None)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if ok is not False else 1


if __name__ == "__main__":
    sys.exit(main())
