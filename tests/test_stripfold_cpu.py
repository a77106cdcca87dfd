"""CPU: the deferred fills' strip-end fold (ksw2_lane_pkfold.h: k2a_pkfold_task) against K2aLanePk::do_fin_seq, strip by strip.

tests/stripfold/stripfold_check.cpp compiled with the address and undefined-behaviour sanitizers into a stand-alone program (the
sanitizer runtimes linked in) and run as such; nothing is loaded into this process.  The program runs the fold's own text with its 64
lanes as loops on synthetic records, C = 8 and C = 16, from buffers of exactly the task's size and from buffers with winning stale
records behind, and compares every book field; its directed cases check on the reference's book that they are what they are named
after."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stripfold_checker(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/stripfold/stripfold_check.cpp")
    exe = str(tmp_path / "stripfold_check")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "ksw2_amd", "csrc"), os.path.join(ROOT, "tests", "stripfold", "stripfold_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    for c in (8, 16):
        m = re.search(r"C=%d: (\d+) directed, (\d+) random cases" % c, r.stdout)
        assert m and int(m.group(1)) >= 30 and int(m.group(2)) >= 1000, r.stdout
    assert r.stdout.rstrip().endswith("stripfold check ok"), r.stdout[-500:]
