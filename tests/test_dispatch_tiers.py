"""csrc/tiers.hpp on CPU (a g++ build of tests/native/tiers_driver.cpp): which tier of a model family a launch gets.  The header is
what muse_kernels.hip's dispatch compiles -- the families' tier lists and the one tier rule -- instantiated here over stand-in types
that carry MAXB alone.  The expected table is written out below from the dispatch's specification, not computed from the header:

    family                                  tier for ntheta (small tiers)
    funnel                                  1 -> 1, 2 -> 2, 3-4 -> 4, 5-8 -> 8
    every stencil and response variant      1-2 -> 2, 3-4 -> 4, 5-8 -> 8
    user elementwise                        1 -> 1, 2-8 -> 8
    pair family                             2 -> 2, 3-4 -> 4, 5-8 -> 8   (1, which the engine never forms: the first tier that holds it)
    noise                                   its one type

`big` set (it can be for 2 .. 8 components as well as above 8): the tier with MAXB > 8, refused where the family has none -- noise and
the pair family.  Without `big` nothing holds more than 8 components: refused.  The per-simulation operators' policy: the widest small
tier for every ntheta <= 8."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "native", "tiers_driver.cpp")
BIG = 64
HAS_BIG = {"funnel": True, "stencil": True, "elementwise": True, "pair": False, "noise": False}
FIRST_FIT = {
    "funnel": {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8},
    "stencil": {1: 2, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8},      # (a response header's family is this list over its own type)
    "elementwise": {1: 1, 2: 8, 3: 8, 4: 8, 5: 8, 6: 8, 7: 8, 8: 8},
    "pair": {1: 2, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8},
    "noise": {1: 1},
}
WIDEST = {"funnel": 8, "stencil": 8, "elementwise": 8, "pair": 8, "noise": 1}


def expected_lines():
    out = {}
    for fam, small in FIRST_FIT.items():
        big_row = [str(BIG) if HAS_BIG[fam] else "-"] * BIG
        out[f"{fam} first big=0"] = [str(small[nt]) if nt in small else "-" for nt in range(1, BIG + 1)]
        out[f"{fam} widest big=0"] = [str(WIDEST[fam]) if nt <= WIDEST[fam] else "-" for nt in range(1, BIG + 1)]
        out[f"{fam} first big=1"] = big_row
        out[f"{fam} widest big=1"] = big_row
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tier_rule_equals_the_written_table(tmp_path, sanitize):
    exe = str(tmp_path / "tiers_driver")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, DRIVER], capture_output=True, text=True)
    # (skipped only where the linker does not find the sanitizers' runtime libraries; every other failure of the compile is a failure)
    if r.returncode != 0 and sanitize and any(lib in r.stderr for lib in ("libasan", "libubsan", "-lasan", "-lubsan")):
        pytest.skip(f"sanitizer runtime not available for this build: {r.stderr[-400:]}")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    for marker in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert marker not in out, out[-3000:]
    lines = r.stdout.splitlines()
    assert lines[0] == f"kMaxTheta 8 kBigTheta {BIG}"
    got = {k: v.split() for k, v in (l.split(":") for l in lines if ":" in l)}
    want = expected_lines()
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the policy is decided at compile time: a visitor is compiled for the tiers its policy can pick and no other -- all five of the
    # funnel's under first-fit, <8> and <64> under the per-simulation operators' (a kernel launched from the visitor is instantiated
    # for every tier the visitor is compiled for, launched or not)
    assert "compiled funnel first 5 widest 2" in lines
    assert lines[-1] == "tiers driver ok"
