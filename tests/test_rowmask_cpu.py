"""CPU: the wavefront-uniform row masks of the packed fill (ksw2_amd/csrc/ksw2_lane_rowmask.h) against the per-lane band test of
K2aLanePk::step, on the host: tests/rowmask/rowmask_check.cpp compiled with the address and undefined-behaviour sanitizers into a
stand-alone program (the sanitizer runtimes linked in) and run as one; nothing is loaded into this process.  The program walks 64 lanes in lock step through the fill
body's loop with both row predicates and compares the masks bit for bit and the lane state after every step, on the grid of
(w, tlen, qlen) around every boundary of the strip schedule for each packed geometry plus random shapes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rowmask_checker(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/rowmask/rowmask_check.cpp")
    exe = str(tmp_path / "rowmask_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread",
                        "-I", os.path.join(ROOT, "ksw2_amd", "csrc"), os.path.join(ROOT, "tests", "rowmask", "rowmask_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("(")]
    geoms = {tuple(int(x) for x in re.match(r"\((\d+),(\d+)\)", l).groups()) for l in lines}
    assert geoms == {(64, 16), (8, 18), (16, 8), (64, 8)}, r.stdout
    for l in lines:
        grid, uni = int(re.search(r"(\d+) grid shapes", l).group(1)), int(re.search(r"(\d+) on shifted masks alone", l).group(1))
        assert grid >= 400 and uni > 0, l
    assert r.stdout.rstrip().endswith("rowmask check ok"), r.stdout[-500:]
