"""CPU: the deferred fills' pair-maximum form (K2aLanePk PM, ksw2_lane_pk.h; k2a_pkfold_task_pm, ksw2_lane_pkfold.h) against the per-row
form and a plain int32 recurrence.

tests/stripmax/stripmax_check.cpp compiled with the address and undefined-behaviour sanitizers into a stand-alone program (the
sanitizer runtimes linked in) and run as such; nothing is loaded into this process.  The program runs 64 lanes of both forms in lock
step over whole alignments, C = 8 and C = 16, plain and re-based, and checks the pairs' maxima, the bound on adjacent rows' maxima that
the fold's freeze test rests on, and the fold's books against K2aLanePk::do_fin_seq -- equal where neither freezes, the exact book in
front of an earlier row where the new fold freezes, never unfrozen where the per-row form froze."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stripmax_checker(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/stripmax/stripmax_check.cpp")
    exe = str(tmp_path / "stripmax_check")
    b = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-I", os.path.join(ROOT, "ksw2_amd", "csrc"), os.path.join(ROOT, "tests", "stripmax", "stripmax_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    for c in (8, 16):
        m = re.search(r"C=%d: (\d+) cases" % c, r.stdout)
        assert m and int(m.group(1)) >= 60, r.stdout
    m = re.search(r"best cells: (\d+) at column 0, (\d+) on the left band edge, (\d+) on the right", r.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), r.stdout
    m = re.search(r"(\d+) books: the pair fold froze (\d+) \((\d+) of them before", r.stdout)
    assert m and int(m.group(1)) >= 2000 and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout
    assert r.stdout.rstrip().endswith("stripmax check ok"), r.stdout[-500:]
