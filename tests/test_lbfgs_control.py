"""The scalar machine of libmuse_lbfgs.so on the CPU, the library's exports and its kernels' resources (no GPU).

tests/native/lbfgs_driver.cpp is a g++ build of museinference.jl_amd/lbfgs/lbfgs_control.hpp + lbfgs_advance.hpp -- the headers the
advance kernel compiles -- over naive host loops: its counts and statuses must EQUAL optim.lbfgs's on the same functions in torch, and
the minimisers agree to 1e-12 (n <= 2: the sums have the same order).  Built a second time with -fsanitize=address,undefined."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from museinference_jl_amd import _capi, optim
from museinference_jl_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T = lambda v: torch.tensor(v, dtype=torch.float64)


def _torch_cases():
    rosen = lambda z: ((1 - z[0]) ** 2 + 100 * (z[1] - z[0] ** 2) ** 2,
                       torch.stack([-2 * (1 - z[0]) - 400 * z[0] * (z[1] - z[0] ** 2), 200 * (z[1] - z[0] ** 2)]))
    bowl = lambda z: (0.5 * (z[0] * z[0] + z[1] * z[1]), z.clone())
    nan_f = lambda z: (T(math.nan), z.clone())
    barrier = lambda z: (0.5 * ((z[0] - 3) * (z[0] - 3)) - torch.log(2.5 - z[0]), ((z[0] - 3) + 1 / (2.5 - z[0])).reshape(1))

    def quartic(z):
        u = z[0] - 1
        return (u * u) * (u * u) + 0.5 * (z[0] * z[0]), (4 * (u * u * u) + z[0]).reshape(1)
    return {"rosenbrock_origin": (rosen, [0.0, 0.0]), "rosenbrock_classic": (rosen, [-1.2, 1.0]), "converged_at_start": (bowl, [0.0, 0.0]),
            "nan_objective": (nan_f, [1.0]), "nonfinite_first_trial": (barrier, [0.0]), "quartic": (quartic, [3.0])}


def _run_driver(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(HERE, "native", "lbfgs_driver.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "lbfgs driver ok" in r.stdout, r.stdout
    out = {}
    for line in r.stdout.splitlines()[:-1]:
        w = line.split()
        assert len(w) >= 7, line
        out[w[0]] = (int(w[1]), int(w[2]), int(w[3]), float(w[4]), float(w[5]), np.array([float(v) for v in w[6:]]))
    return out


@pytest.fixture(scope="module")
def reference():
    return {k: optim.lbfgs(fg, T(x0), 1e-8) for k, (fg, x0) in _torch_cases().items()}


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["O2", "asan_ubsan"])
def test_control_header_equals_optim_lbfgs(tmp_path, reference, flags):
    got = _run_driver(tmp_path, flags, "lbfgs_driver")
    assert set(got) == set(reference)
    for k, (x, info) in reference.items():
        it, fc, st, fmin, gn, xd = got[k]
        assert (it, fc, st) == (info["iterations"], info["f_calls"], info["status"]), (k, got[k], info)
        np.testing.assert_allclose(xd, x.numpy(), rtol=0, atol=1e-12, err_msg=k)
        if math.isfinite(info["f_min"]):
            np.testing.assert_allclose(fmin, info["f_min"], rtol=1e-12, atol=1e-300, err_msg=k)
            np.testing.assert_allclose(gn, info["gnorm"], rtol=0, atol=1e-12, err_msg=k)
    # the pins themselves: Optim's documented run, a start at the minimum, a NaN objective, and the psi3 shrink really taken
    assert got["rosenbrock_origin"][:3] == (24, 67, optim.STATUS_G_CONVERGED)
    assert got["converged_at_start"][:3] == (0, 1, optim.STATUS_G_CONVERGED)
    assert got["nan_objective"][:3] == (0, 1, optim.STATUS_NONFINITE)
    assert got["nonfinite_first_trial"][2] == optim.STATUS_G_CONVERGED and got["nonfinite_first_trial"][5][0] < 2.5


def test_nonfinite_first_trial_takes_the_shrink_branch():
    """(the case is what it says: optim.lbfgs's first trial point of that function is not finite)"""
    fg, x0 = _torch_cases()["nonfinite_first_trial"]
    f0, g0 = fg(T(x0))
    f1, _ = fg(T(x0) - g0)
    assert math.isfinite(float(f0)) and not math.isfinite(float(f1))


def test_lbfgs_library_exports_equal_header_equal_ctypes_table():
    path = B.build_lbfgs_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    assert exported == B.lbfgs_declared_symbols() == sorted(_capi.LBFGS_SIGNATURES)
    # ... and the product library's are what they were: its own header, its own table
    assert not any(n.startswith("muse_lbfgs") for n in _capi.SIGNATURES)
    assert not any(n.startswith("muse_lbfgs") for n in B.declared_symbols())
    lib = _capi.load_lbfgs_library()
    assert lib.muse_lbfgs_workspace_bytes(3, 7, 10) > 3 * 23 * 7 * 8
    assert lib.muse_lbfgs_workspace_bytes(3, 7, 9) < 0          # m = 10 only
    assert lib.muse_lbfgs_workgroup_size(4096) == 256 and lib.muse_lbfgs_workgroup_size(4097) == 1024


def test_lbfgs_sources_are_not_under_csrc():
    """bench.csrc_fingerprint() and the model libraries are defined by csrc/: the new sources live beside it."""
    assert not [f for f in os.listdir(B.CSRC) if "lbfgs" in f]
    assert os.path.dirname(B._LBFGS_SOURCE) != B.CSRC


def test_advance_kernel_has_no_scratch_and_no_spill():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regs
    rows = regs.library_report(B.build_lbfgs_library())
    adv = [r for r in rows if "advance_kernel" in r[0]]
    assert len(adv) == 2, rows                       # the two workgroup sizes
    for name, vgpr, vspill, sspill, scratch, dyn in rows:
        assert vspill == 0 and scratch == 0 and not dyn, (name, vgpr, vspill, scratch, dyn)
    assert all(r[1] <= 128 for r in adv), adv        # (1024 threads = 4 wavefronts per SIMD: at most 128 registers each)
