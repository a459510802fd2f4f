"""muse_exp (csrc/step.hpp) on the CPU -- a g++ build of tests/native/exp_driver.cpp, without floating-point contraction --
against numpy.longdouble's exp (x87 extended, 64-bit significand: its own error is below 2^-10 ulp of a double)."""
import os
import subprocess

import numpy as np
import pytest

import hp_reference as R

pytestmark = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
HI_CUT, LO_CUT = 7.09782712893383973096e+02, -7.45133219101941108420e+02     # the source's cut-offs
LN2 = np.log(LD(2))
TINY, SUB = 2.0 ** -1022, 2.0 ** -1074                                      # smallest normal, subnormal spacing


def _neighbours(v, n=2):
    out = [np.asarray(v, np.float64)]
    for d in (-np.inf, np.inf):
        w = out[0]
        for _ in range(n):
            w = np.nextafter(w, d)
            out.append(w)
    return np.concatenate([np.atleast_1d(o) for o in out])


def _run(exe, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    text = "\n".join(f"{b:016x}" for b in x.view(np.uint64).tolist()) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    y = np.array([int(t, 16) for t in r.stdout.split()], dtype=np.uint64).view(np.float64)
    assert y.size == x.size
    return y


def _ulp(v):
    """The spacing of doubles at |v| (v a longdouble array of normal-range magnitudes): 2^(floor(log2 |v|) - 52)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(LD(1), e - 53)


def test_muse_exp_against_longdouble_exp(tmp_path):
    """Below 1 ulp wherever the result is normal (the source's own claim); below one ulp of the unscaled y plus half a subnormal
    spacing where it is subnormal (the two-step scaling rounds a second time); the exact values at the special arguments.

    Recorded (not the tolerance): over the 130 079 arguments of this test the largest error among normal results is 0.8994 ulp,
    at x = 597.8394432329529; among subnormal results the largest error is within 1e-8 of its bound (the arguments beside the
    lower cut-off, whose result is half a subnormal spacing: correct rounding all but attains the bound there)."""
    exe = str(tmp_path / "exp_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           "-o", exe, os.path.join(HERE, "native", "exp_driver.cpp")])
    rng = np.random.default_rng(20240)
    m = np.arange(-1076, 1026)
    edges = np.concatenate([((m + s) * LN2).astype(np.float64) for s in (LD(0.5), LD(-0.5))])     # where k changes
    xs = np.concatenate([
        rng.uniform(-745.2, 709.8, 50_000), rng.uniform(-2.0, 2.0, 30_000), rng.normal(0.0, 1e-3, 10_000),
        rng.uniform(-1.0, 1.0, 5_000) * 2.0 ** rng.integers(-1074, -10, 5_000).astype(np.float64),       # dense around 0, down to subnormals
        _neighbours(edges), _neighbours([HI_CUT, LO_CUT], 3),
        rng.uniform(-745.2, -708.3, 10_000),                                                             # subnormal results
        rng.uniform(709.44, HI_CUT, 2_000), _neighbours([709.5, 709.7]),                                 # k = 1024
        rng.uniform(-708.75, -708.05, 2_000), _neighbours([-708.4]),                                     # k = -1022
        _neighbours([0.0, -0.0, 1.0, -1.0, 0.5 * float(LN2), -0.5 * float(LN2)])])
    y = _run(exe, xs)
    k = np.floor(xs.astype(LD) / LN2 + LD(0.5))
    assert (k == 1024).sum() > 1000 and (k == -1022).sum() > 1000
    want = np.exp(xs.astype(LD))
    over, under = xs > HI_CUT, xs < LO_CUT
    assert over.any() and under.any()
    assert np.all(np.isposinf(y[over])) and np.all(y[under] == 0.0) and not np.signbit(y[under]).any()
    mid = ~(over | under)
    assert np.all(np.isfinite(y[mid])) and np.all(y[mid] > 0.0)
    err = np.abs(y.astype(LD) - want)
    normal = mid & (want >= LD(TINY))
    sub = mid & (want < LD(TINY))
    assert normal.sum() > 100_000 and sub.sum() > 10_000
    e_n = (err[normal] / _ulp(want[normal])).astype(np.float64)
    i = int(np.argmax(e_n))
    print(f"muse_exp: {xs.size} arguments; normal results: max {e_n[i]:.4f} ulp at x = {xs[normal][i]!r}")
    assert e_n.max() < 1.0, (e_n.max(), xs[normal][i])
    # a subnormal result is y 2^(k + 1000) (exact: a normal number) rounded once more onto the subnormal grid by the product with
    # 2^-1000: y within one of ITS ulps of exp(r) -- relative to the result at most 2^-52, y >= 1/2 ... -- plus half a spacing
    b_s = want[sub] * LD(2.0 ** -52) + LD(0.5) * LD(SUB)
    e_s = (err[sub] / b_s).astype(np.float64)
    print(f"muse_exp: subnormal results: max {e_s.max():.8f} of the bound")
    assert e_s.max() < 1.0, e_s.max()
    # the special arguments: exact values
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, HI_CUT, LO_CUT, np.nextafter(HI_CUT, np.inf), np.nextafter(LO_CUT, -np.inf)])
    ys = _run(exe, sp)
    assert ys[0] == 1.0 and ys[1] == 1.0                     # muse_exp(+-0) == 1 exactly
    assert np.isposinf(ys[2]) and ys[3] == 0.0 and not np.signbit(ys[3]) and np.isnan(ys[4])
    assert np.isfinite(ys[5]) and abs(LD(ys[5]) - np.exp(LD(HI_CUT))) < _ulp(np.exp(LD(HI_CUT)))   # the last finite result
    assert ys[6] in (0.0, SUB)                               # exp(LO_CUT) = 0.5000000000002 SUB ... either neighbour is within the bound
    assert np.isposinf(ys[7]) and ys[8] == 0.0
