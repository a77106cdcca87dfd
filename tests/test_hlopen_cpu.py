"""CPU: the packed lanes' row registers hold H - q and the column profiles q + e + s (K2A_HL_OPEN, ksw2_lane_pk.h "Open form").

test_hlopen_checker: tests/hlopen/hlopen_check.cpp compiled with the address and undefined-behaviour sanitizers into stand-alone
programs (one per geometry, built side by side; the sanitizer runtimes linked in) and run as such; nothing is loaded into this
process.  The program drives K2aLanePk lanes through whole small alignments and compares them with a plain int32 recurrence of its own.

test_hlopen_sim_*: the simulator build against the oracle under the scorings of tests/hlopen_util.py -- the ones that sit on the
boundaries of a profile byte -- through every packed form: score only with the deferred arg-max and without, KSW_EZ_APPROX_MAX, CIGAR
left- and right-aligned, two-piece gaps, solo (an odd pair out), generation-serial.  Every case asserts that every pair is packed;
each was checked to be packed under the form before this one too (the table's form does not decide what is packed)."""
import os
import re
import shutil
import subprocess

import pytest

import ksw2_amd as ka
from oracle import pyoracle as po
from tests import hlopen_util as hu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "sim")


def test_hlopen_checker(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/hlopen/hlopen_check.cpp")
    geoms = {0: "(8,18)", 1: "(16,8)", 2: "(64,16)"}
    builds = {g: subprocess.Popen([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                                   "-static-libubsan", "-pthread", "-DHLOPEN_GEOM=%d" % g, "-I", os.path.join(ROOT, "ksw2_amd", "csrc"),
                                   os.path.join(ROOT, "tests", "hlopen", "hlopen_check.cpp"), "-o", str(tmp_path / ("hlopen_check%d" % g))],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for g in geoms}
    for g, b in builds.items():
        _, err = b.communicate()
        assert b.returncode == 0, err[-4000:]
    for g, name in geoms.items():
        r = subprocess.run([str(tmp_path / ("hlopen_check%d" % g))], capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        forms = [l for l in r.stdout.splitlines() if l.startswith(name)]
        # plain and re-based x single and two-piece x score only and left-aligned, each with cases
        assert len(forms) == 8 and all(int(re.search(r"(\d+) cases", l).group(1)) >= 12 for l in forms), r.stdout
        assert re.search(r"K2A_HL_OPEN 1: \d+ cases", r.stdout), r.stdout
        assert r.stdout.rstrip().endswith("hlopen check ok"), r.stdout[-500:]


@pytest.fixture(scope="module")
def sim():
    subprocess.run(["make", "-C", SIM_DIR], check=True, capture_output=True)
    L = ka.Library(os.path.join(SIM_DIR, "libksw2_amd_sim.so"))
    assert L.backend() == "sim"
    return L


def _pk(form=None, **kv):
    return lambda d: all(c["kernel"] == "pk" and (form is None or c["form"] == form) and all(c[k] == v for k, v in kv.items()) for c in d)


# (name, env, two-piece, flag, pairs, qlen, tlen, w, zdrop, check of the plan's description)
FORMS = [
    ("defer", {"KSW2AMD_DEFER": 1, "KSW2AMD_SOLO": 0}, False, po.SCORE_ONLY, 8, 300, 310, 40, 100, _pk("defer", mode="score")),
    ("nodefer", {"KSW2AMD_DEFER": 0, "KSW2AMD_SOLO": 0}, False, po.SCORE_ONLY, 8, 300, 310, 40, 100, lambda d: _pk(mode="score")(d) and all(c["form"] != "defer" for c in d)),
    ("approx", {"KSW2AMD_SOLO": 0}, False, po.SCORE_ONLY | po.APPROX_MAX, 8, 300, 310, 40, -1, _pk(nomax=1)),
    ("cigar-left", {"KSW2AMD_SOLO": 0}, False, 0, 8, 200, 190, 30, 100, _pk(mode="left")),
    ("cigar-right", {"KSW2AMD_SOLO": 0}, False, po.RIGHT, 8, 200, 190, 30, 100, _pk(mode="right")),
    ("two-piece", {"KSW2AMD_SOLO": 0}, True, 0, 8, 200, 190, 30, 100, _pk(gaps=2, mode="left")),
    ("two-piece-score", {"KSW2AMD_SOLO": 0}, True, po.SCORE_ONLY, 8, 300, 310, 40, 100, _pk(gaps=2, mode="score")),
    ("solo", {"KSW2AMD_SOLO": "all"}, False, 0, 3, 300, 290, 64, 100, lambda d: all(c["kernel"] == "solo" for c in d)),
    ("solo-score", {"KSW2AMD_SOLO": "all"}, True, po.SCORE_ONLY, 3, 300, 290, 64, 100, lambda d: all(c["kernel"] == "solo" for c in d)),
    ("serial", {}, False, po.SCORE_ONLY, 2, 2300, 2337, -1, -1, lambda d: all(c["kernel"] == "pkmp" for c in d)),
    ("serial-cigar", {}, True, 0, 2, 2300, 2337, -1, 300, lambda d: all(c["kernel"] == "pkmp" for c in d)),
]
# gap costs of 155 and more: short pairs on a plain window; neither the solo nor the generation-serial class admits them
SHORT_FORMS = [(name, env, dual, flag, n, 40, 44, 10, zd if zd < 0 else 400, want) for name, env, dual, flag, n, _, _, _, zd, want in FORMS[:7]]


def _cases():
    out = []
    for s in hu.SCORINGS:
        for f in (SHORT_FORMS if s in hu.SHORT else FORMS):
            if s == "deep" and f[0].startswith("serial"):      # a row maximum may drift too far between two re-bases under this scoring (pk_slide_ok): int32 before and now
                continue
            out.append(pytest.param(s, f, id="%s-%s" % (s, f[0])))
    return out


@pytest.mark.parametrize("scoring,form", _cases())
def test_hlopen_sim_forms(sim, monkeypatch, scoring, form):
    name, env, dual, flag, n, ql, tl, w, zd, want = form
    m, wild = hu.SCORINGS[scoring][1], hu.SCORINGS[scoring][9]
    qs, ts = hu.pairs(5100 + len(name) + 7 * ql, n, ql, tl, m, wild, zd)
    d = hu.run_case(sim, monkeypatch.setenv, monkeypatch.delenv, scoring, env, dual, flag, qs, ts, w, zd, want)
    if scoring in hu.SHORT:
        assert all(c["rebased"] == 0 for c in d), d
