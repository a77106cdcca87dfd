"""Helpers of the tests of the flat local-alignment batches (ksw2amd_ll_batch_flat / ksw2amd_ll_align_batch_flat): the simulator build
with the check kernel's twin and counted launches (tests/llsim/llf_shim_sim.cpp), and arena builders."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

from tests import ll_util as u

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def sim_library(path_out=None):
    """The product's host objects -- ksw2_host_ll.c, ksw2_host_lla.c and ksw2_host_llf.c included -- against tests/sim/ksw2_shim_sim.cpp
    and tests/llsim/llf_shim_sim.cpp (which compiles the two local-alignment twins in).  Returns the path of the .so."""
    d = tempfile.mkdtemp(prefix="llfsim_", dir=u.build_dir())
    csrc = os.path.join(ROOT, "ksw2_amd", "csrc")
    objs = []
    for h in ("plan", "pool", "single", "ext", "ll", "lla", "llf"):
        o = os.path.join(d, "host_%s.o" % h)
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-fPIC", "-c", os.path.join(csrc, "ksw2_host_%s.c" % h), "-o", o], check=True)
        objs.append(o)
    for src, o in ((os.path.join(HERE, "sim", "ksw2_shim_sim.cpp"), "sim.o"), (os.path.join(HERE, "llsim", "llf_shim_sim.cpp"), "llfsim.o")):
        o = os.path.join(d, o)
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-w", "-c", src, "-o", o], check=True)
        objs.append(o)
    out = path_out or os.path.join(d, "libksw2_amd_llfsim.so")
    subprocess.run(["g++", "-shared", "-o", out] + objs + ["-ldl", "-lpthread"], check=True)
    return out


def counters(lib):
    """(alignment launches, check launches, blocks checked) of a simulator build since reset_counters"""
    L = lib.lib
    for f in (L.llf_sim_align_launches, L.llf_sim_check_launches, L.llf_sim_check_blocks):
        f.restype = ctypes.c_long
    return int(L.llf_sim_align_launches()), int(L.llf_sim_check_launches()), int(L.llf_sim_check_blocks())


def reset_counters(lib):
    lib.lib.llf_sim_reset_counters.restype = None
    lib.lib.llf_sim_reset_counters()


def arena(queries, targets, rng=None, lead=0, gap=0, fill=255, align=1):
    """One uint8 arena holding every query and target once -> (base, qoff, qlen, toff, tlen).  lead: bytes before the first sequence;
    gap: up to that many bytes (exactly that many without rng) between sequences; the bytes outside the sequences hold `fill` (a code
    that no matrix admits: the check must not look at them); align: every sequence starts at a multiple of it plus lead."""
    seqs = [np.ascontiguousarray(x, dtype=np.uint8) for x in list(queries) + list(targets)]
    offs, pos = [], lead
    for s in seqs:
        pos = lead + (pos - lead + align - 1) // align * align
        offs.append(pos)
        pos += len(s) + (int(rng.integers(0, gap + 1)) if rng is not None and gap else gap)
    base = np.full(pos + 1, fill, dtype=np.uint8)
    for o, s in zip(offs, seqs):
        base[o:o + len(s)] = s
    n = len(queries)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    offs = np.array(offs, dtype=np.uint64)
    return base, offs[:n].copy(), lens[:n].copy(), offs[n:].copy(), lens[n:].copy()


def pairs_of(base, qoff, qlen, toff, tlen):
    """The (queries, targets) lists that an arena's offsets describe (copies)."""
    qs = [base[int(o):int(o) + int(l)].copy() for o, l in zip(qoff, qlen)]
    ts = [base[int(o):int(o) + int(l)].copy() for o, l in zip(toff, tlen)]
    return qs, ts
