"""The lock-step conjugate gradients of libmuse_lbfgs.so on the CPU, the library's new exports and its kernels' resources (no GPU).

tests/native/cg_driver.cpp is a g++ build of museinference.jl_amd/lbfgs/cg_control.hpp + cg_advance.hpp -- the headers the CG step
kernel compiles -- over naive host loops: its counts must EQUAL simple._cg's on the same operators and right-hand sides in torch
(reltol sqrt(eps), maxiter 100), and its true residual |b - M y| is at most the larger of the tolerance and twice _cg's own.  Built a
second time with -fsanitize=address,undefined."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from museinference_jl_amd import _capi, simple
from museinference_jl_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RELTOL = math.sqrt(np.finfo(np.float64).eps)
NS, KS = (1, 5, 255, 257, 4097), (1, 2, 3, 5)


# The right-hand sides: the first n of one standard-normal vector (numpy's legacy generator, seed 1: a fixed stream), handed to the
# driver as a file -- the same bits on both sides.  How many iterations the periodic operator takes at n = 257 depends on b (17 / 20 /
# 37 is what a normal b typically gives, and what this one gives under numpy in plain, permuted and pairwise summation; a smoother b
# takes fewer); the diagonal cases take one iteration per DISTINCT value, min(k, n) -- 1 at n = 1 -- for any b with a component in each.
MASTER = np.random.RandomState(1).randn(4097)


def rhs(n):
    return torch.as_tensor(MASTER[:n].copy())


def diag_op(n, k):
    d = torch.as_tensor(1.0 + 0.75 * (np.arange(n) % k).astype(np.float64))
    return lambda p: d * p


def periodic_op(s):
    return lambda p: (2.0 + s) * p - torch.roll(p, 1) - torch.roll(p, -1)


def operator_cases():
    """name -> (operator, n, the count the case is expected to take)"""
    cases = {f"diag_n{n}_k{k}": (diag_op(n, k), n, min(k, n)) for n in NS for k in KS}
    cases["periodic_n33_s1"] = (periodic_op(1.0), 33, 17)
    cases["periodic_n257_s1"] = (periodic_op(1.0), 257, 20)
    cases["periodic_n257_s025"] = (periodic_op(0.25), 257, 37)
    return cases


def _run_driver(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(HERE, "native", "cg_driver.cpp")])
    vec = str(tmp_path / "rhs.f64")
    MASTER.tofile(vec)
    r = subprocess.run([exe, vec], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cg driver ok" in r.stdout, r.stdout
    out = {}
    for line in r.stdout.splitlines()[:-1]:
        w = line.split()
        assert len(w) == 7, line
        out[w[0]] = dict(count=int(w[1]), rounds=int(w[2]), resnorm=float(w[3]), true_res=float(w[4]), bnorm=float(w[5]), ymax=float(w[6]))
    return out


@pytest.fixture(scope="module")
def reference():
    ref = {}
    for name, (op, n, _) in operator_cases().items():
        b = rhs(n)
        y, k = simple._cg(op, b, 100, RELTOL)
        ref[name] = (k, float(torch.linalg.norm(b - op(y))), float(torch.linalg.norm(b)))
    return ref


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["O2", "asan_ubsan"])
def test_cg_headers_equal_simple_cg(tmp_path, reference, flags):
    got = _run_driver(tmp_path, flags, "cg_driver")
    cases = operator_cases()
    assert set(cases) <= set(got)
    for name, (op, n, expected) in cases.items():
        k, res, bnorm = reference[name]
        g = got[name]
        print(name, "count", g["count"], "_cg", k, "true residual", g["true_res"], "_cg", res, "tol", RELTOL * bnorm)
        assert g["count"] == k == expected, (name, g, k, expected)
        assert g["rounds"] == g["count"]
        assert g["bnorm"] == pytest.approx(bnorm, rel=1e-14)
        assert g["true_res"] <= max(RELTOL * bnorm, 2.0 * res), (name, g, res)
        assert g["resnorm"] <= RELTOL * bnorm
    # a zero right-hand side, maxiter = 0 and maxiter = 3
    assert got["zero_rhs"]["count"] == 0 and got["zero_rhs"]["rounds"] == 0 and got["zero_rhs"]["ymax"] == 0.0
    assert got["maxiter0"]["count"] == 0 and got["maxiter0"]["rounds"] == 0 and got["maxiter0"]["ymax"] == 0.0
    assert got["maxiter3"]["count"] == 3 and got["maxiter3"]["rounds"] == 3
    # abstol (1e-4) above reltol |b| stops earlier than reltol alone, at a residual within it
    a = got["abstol"]
    assert 1e-4 > RELTOL * a["bnorm"] and 0 < a["count"] < got["periodic_n257_s025"]["count"] and a["resnorm"] <= 1e-4
    # M = diag(1, -1), b = (1, 2): p.Mp = -3 in the first round -- the guard: count -1 - 0, y as it was
    assert got["indefinite"]["count"] == -1 and got["indefinite"]["rounds"] == 1 and got["indefinite"]["ymax"] == 0.0
    assert got["nan_operator"]["count"] < 0 and got["nan_operator"]["ymax"] == 0.0


def test_cg_entry_points_are_exported_and_refuse_bad_arguments():
    path = B.build_lbfgs_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    names = {"muse_lbfgs_cg_workspace_bytes", "muse_lbfgs_cg_begin", "muse_lbfgs_cg_advance", "muse_lbfgs_cg_result"}
    assert names <= exported and names <= set(B.lbfgs_declared_symbols()) and names <= set(_capi.LBFGS_SIGNATURES)
    for f in ("cg_control.hpp", "cg_advance.hpp", "cg_kernels.hpp"):
        assert os.path.join(B.LBFGS_DIR, f) in B._LBFGS_DEPS
    lib = _capi.load_lbfgs_library()
    # one record per row (256-byte aligned) and two vectors, y and r: p lives in the caller's row
    assert lib.muse_lbfgs_cg_workspace_bytes(3, 7) == 256 + 3 * 2 * 7 * 8
    assert lib.muse_lbfgs_cg_workspace_bytes(0, 7) == -1 and lib.muse_lbfgs_cg_workspace_bytes(3, 0) == -1
    # bad arguments are answered before anything touches a device (a non-null pointer is never followed)
    buf = np.zeros(64)
    p = buf.ctypes.data
    assert lib.muse_lbfgs_cg_begin(None, 1, 4, p, RELTOL, 0.0, 100, p, p, None) == -1
    assert lib.muse_lbfgs_cg_begin(p, 1, 4, None, RELTOL, 0.0, 100, p, p, None) == -1
    assert lib.muse_lbfgs_cg_begin(p, 1, 4, p, RELTOL, 0.0, 100, None, p, None) == -1
    assert lib.muse_lbfgs_cg_begin(p, 1, 4, p, RELTOL, 0.0, 100, p, None, None) == -1
    assert lib.muse_lbfgs_cg_begin(p, 0, 4, p, RELTOL, 0.0, 100, p, p, None) == -1
    assert lib.muse_lbfgs_cg_begin(p, 1, 0, p, RELTOL, 0.0, 100, p, p, None) == -1
    assert lib.muse_lbfgs_cg_advance(None, 1, 4, p, p, p, None) == -1
    assert lib.muse_lbfgs_cg_advance(p, 1, 4, None, p, p, None) == -1
    assert lib.muse_lbfgs_cg_advance(p, 1, 4, p, None, p, None) == -1
    assert lib.muse_lbfgs_cg_advance(p, 1, 4, p, p, None, None) == -1
    assert lib.muse_lbfgs_cg_advance(p, 0, 4, p, p, p, None) == -1 and lib.muse_lbfgs_cg_advance(p, 1, 0, p, p, p, None) == -1
    assert lib.muse_lbfgs_cg_result(None, 1, 4, p, p, p, None) == -1
    assert lib.muse_lbfgs_cg_result(p, 1, 4, None, p, p, None) == -1
    assert lib.muse_lbfgs_cg_result(p, 1, 4, p, None, p, None) == -1
    assert lib.muse_lbfgs_cg_result(p, 1, 4, p, p, None, None) == -1
    assert lib.muse_lbfgs_cg_result(p, 0, 4, p, p, p, None) == -1 and lib.muse_lbfgs_cg_result(p, 1, 0, p, p, p, None) == -1


def test_cg_kernels_resources():
    """No kernel of the library spills or uses scratch; the CG step kernel at 1024 threads (4 wavefronts per SIMD) fits 128 registers;
    no new kernel's name holds `advance_kernel` (the L-BFGS resource test counts exactly two of those)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regs
    rows = regs.library_report(B.build_lbfgs_library())
    for name, vgpr, vspill, sspill, scratch, dyn in rows:
        assert vspill == 0 and scratch == 0 and not dyn, (name, vgpr, vspill, scratch, dyn)
    cg = [r for r in rows if "cg_" in r[0]]
    assert not [r for r in cg if "advance_kernel" in r[0]]
    step = [r for r in cg if "cg_step_kernel" in r[0]]
    assert len(step) == 2 and len([r for r in cg if "cg_begin_kernel" in r[0]]) == 2, rows
    assert len([r for r in cg if "cg_result_kernel" in r[0]]) == 2 and len([r for r in cg if "cg_count_kernel" in r[0]]) == 1, rows
    assert all(r[1] <= 128 for r in step), step
