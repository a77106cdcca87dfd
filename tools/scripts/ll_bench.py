#!/usr/bin/env python3
"""Local-alignment throughput (ksw2amd_ll_batch): cells = qlen x tlen summed over the batch.

  python tools/scripts/ll_bench.py --workload A [--reps 3] [--out profiles/ll_bench_A.json]

Workloads: A 65 536 x (256 x 1 024) (packed form), B 4 096 x 5 000^2, C 16 384 ragged pairs of 100-5 000, D 1 024 x 20 000^2 (int32 form:
KSW2AMD_LL_FORM=0, its scores would fit the packed form).  Reports end-to-end GCUPS (Python pair setup, staging, upload, kernels,
download; best of --reps after one warm-up) and, when --kstats points at a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a run
of the same workload with --kbatches ll_batch calls (1 + that run's --reps), resident GCUPS from the k2a_ll_kernel time per batch.
The record names the kernel forms the batch took (the library's KSW2AMD_TRACE line).
A parity sample (the scalar test oracle, tests/ll_oracle.c) is checked outside the clock."""
import argparse
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


def kernel_ms(path, batches):
    """total k2a_ll_kernel time in a kernel_stats.csv, per batch"""
    tot = 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            if "k2a_ll_kernel" in row.get("Name", ""):
                tot += float(row["TotalDurationNs"]) * 1e-6
    return tot / batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parity", type=int, default=4)
    ap.add_argument("--kstats", default=None)
    ap.add_argument("--kbatches", type=int, default=2)
    ap.add_argument("--form", default=None, help="KSW2AMD_LL_FORM (default: 0 for D, the library's default otherwise)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    q, t = workload(a.workload, rng)
    mat = u.simple_mat(5, 2, 4, -1)
    gapo, gape = 4, 2
    cells = float(sum(len(x) * len(y) for x, y in zip(q, t)))
    form = a.form if a.form is not None else ("0" if a.workload == "D" else None)
    if form is not None:
        os.environ["KSW2AMD_LL_FORM"] = form
    lib = ksw2_amd.library()
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


if __name__ == "__main__":
    sys.exit(main())
