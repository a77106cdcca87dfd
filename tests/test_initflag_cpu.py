"""CPU: K2aLanePk::do_init behind the wavefront-uniform "some new strip has column-0 rows" flag (what the packed fill passes with
K2A_INIT_COL0_UNIFORM) against the plain do_init, on the host: tests/stripev/initflag_check.cpp compiled with the address and
undefined-behaviour sanitizers into a stand-alone program (the sanitizer runtimes linked in) and run as one; nothing is loaded into
this process.  The program walks 64 lanes of the headline fill's lane type in lock step through the fill body's loop with both forms,
re-based and not, and compares the lane state after every step and the two books after every strip."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_initflag_checker(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/stripev/initflag_check.cpp")
    exe = str(tmp_path / "initflag_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread",
                        "-I", os.path.join(ROOT, "ksw2_amd", "csrc"), os.path.join(ROOT, "tests", "stripev", "initflag_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    runs = [l for l in r.stdout.splitlines() if l.startswith("RB ")]
    assert sorted(re.match(r"RB (\d):", l).group(1) for l in runs) == ["0", "1"], r.stdout
    for l in runs:
        cases, frozen = int(re.search(r"(\d+) cases", l).group(1)), int(re.search(r"(\d+) frozen books", l).group(1))
        off, on = int(re.search(r"(\d+) with the flag off", l).group(1)), int(re.search(r"(\d+) on;", l).group(1))
        assert cases >= 400 and frozen > 0 and off > 0 and on > 0, l
    assert r.stdout.rstrip().endswith("initflag check ok"), r.stdout[-500:]
