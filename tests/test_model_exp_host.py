"""muse::model_exp (csrc/model_math.hpp: what muse_model_exp resolves to in the per-element functions of device code) evaluated
on the CPU -- a g++ build of tests/native/model_exp_driver.cpp, without floating-point contraction -- against muse::muse_exp: the
same BITS for every argument, whatever the reciprocal's seed the refinement starts from (the host stands in for v_rcp_f64 with
1 / d cut down to 20 or 12 bits, rounded down and up), and the quotient itself against the IEEE division.  The device's own
sequence is compared on the GPU (tests/test_gpu_model_exp.py)."""
import os
import subprocess

import numpy as np
import pytest

import model_exp_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp_path, name, *defs):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *defs,
                           "-o", exe, os.path.join(HERE, "native", "model_exp_driver.cpp")])
    return exe


def _run(exe, cols, *args):
    text = "\n".join(" ".join(f"{b:016x}" for b in row) for row in zip(*[np.ascontiguousarray(c, np.float64).view(np.uint64).tolist() for c in cols])) + "\n"
    r = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = np.array([int(t, 16) for t in r.stdout.split()], dtype=np.uint64).view(np.float64).reshape(-1, 2)
    assert out.shape[0] == len(cols[0])
    return out[:, 0], out[:, 1]


@pytest.mark.parametrize("defs", [("-DSEED_BITS=20",), ("-DSEED_BITS=20", "-DSEED_UP"), ("-DSEED_BITS=12",), ("-DSEED_BITS=12", "-DSEED_UP")])
def test_model_exp_has_the_bits_of_muse_exp(tmp_path, defs):
    exe = _build(tmp_path, "model_exp_driver", *defs)
    xs = K.arguments()
    want, got = _run(exe, [xs])
    bad = ~K.same_bits(want, got)
    assert not bad.any(), (int(bad.sum()), xs[bad][:5], want[bad][:5], got[bad][:5])
    # the argument set reaches what it is meant to: overflow, flush to zero, subnormal results, NaN, and both scaling bands
    assert np.isposinf(want).sum() > 3 and (want == 0.0).sum() > 3 and np.isnan(want).sum() == 1
    assert ((want > 0) & (want < 2.0 ** -1022)).sum() > 10_000 and (want > 2.0 ** 1023).sum() > 1000


def test_the_unscaled_division_is_the_correctly_rounded_quotient(tmp_path):
    """model_div_unscaled(n, d) == n / d bit for bit over the operands the exponential forms -- d = 2 - c in [1.2, 2.8], n = r c with
    |r| <= ln2 / 2 -- and, wider, d in [1, 4) and |n| in [2^-900, 1]; from the coarsest seed (12 bits, rounded up)."""
    exe = _build(tmp_path, "model_div_driver", "-DSEED_BITS=12", "-DSEED_UP")
    rng = np.random.default_rng(7)
    r = rng.uniform(-0.3466, 0.3466, 400_000)
    c = r - r * r * (1.0 / 6.0)
    n = np.concatenate([r * c, rng.uniform(-1.0, 1.0, 200_000) * 2.0 ** rng.integers(-900, 1, 200_000).astype(np.float64)])
    d = np.concatenate([2.0 - c, rng.uniform(1.0, 4.0, 200_000)])
    want, got = _run(exe, [n, d], "-q")
    bad = ~K.same_bits(want, got)
    assert not bad.any(), (int(bad.sum()), n[bad][:5], d[bad][:5])
