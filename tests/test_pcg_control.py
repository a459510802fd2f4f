"""The diagonally preconditioned lock-step conjugate gradients of libmuse_lbfgs.so on the CPU, the library's new exports and its
kernels' resources (no GPU).

tests/native/pcg_driver.cpp is a g++ build of museinference.jl_amd/lbfgs/pcg_control.hpp + pcg_advance.hpp -- the headers the
preconditioned round kernel compiles -- over naive host loops: its counts must EQUAL simple._pcg's in torch and those of the longdouble
restatement tests/pcg_reference.py on the same operators, diagonals and right-hand sides (reltol sqrt(eps), maxiter 100), and its true
residual |b - M y| is at most the larger of the tolerance and twice the reference's own.  Built a second time with
-fsanitize=address,undefined (a stand-alone program: nothing is preloaded)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pcg_reference as R
from museinference_jl_amd import _capi, simple
from museinference_jl_amd import build as B
from test_cg_control import KS, MASTER, NS, RELTOL, diag_op, periodic_op, rhs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble

# The scaled periodic family: M = W T W with T p = 3 p - roll(p, 1) - roll(p, -1) and W_i = exp(2 sin(1.7 i + 0.3)): the spectrum of T
# lies in [1, 5], the weights span e^-2 .. e^2, so cond(M) reaches ~5 e^8 ~ 1.5e4 and plain CG does not get to sqrt(eps) in 100
# iterations; with d = diag(M) = 3 W^2 the preconditioned operator is similar to T / 3 and the count is T's own.  The weights are
# handed to the driver as a file: the same bits on both sides.
SCALED_NS = (5, 33, 255, 257, 4097)
WEIGHTS = np.exp(2.0 * np.sin(1.7 * np.arange(4097, dtype=np.float64) + 0.3))
SCALED_COUNTS = {5: 3, 33: 17, 255: 22, 257: 22, 4097: 22}


def scaled_op(n):
    w = torch.as_tensor(WEIGHTS[:n].copy())

    def M(p):
        q = w * p
        return w * (3.0 * q - torch.roll(q, 1) - torch.roll(q, -1))
    return M


def scaled_diag(n):
    w = torch.as_tensor(WEIGHTS[:n].copy())
    return 3.0 * (w * w)


def diag_of(n, k):
    return torch.as_tensor(1.0 + 0.75 * (np.arange(n) % k).astype(np.float64))


def scaled_ld(n):
    w = WEIGHTS[:n].astype(LD)

    def M(p):
        q = w * p
        return w * (LD(3) * q - np.roll(q, 1) - np.roll(q, -1))
    return M, LD(3) * (w * w)


def diag_ld(n, k):
    d = (LD(1) + LD(0.75) * (np.arange(n) % k).astype(LD))
    return (lambda p: d * p), d


def periodic_ld(s):
    return lambda p: LD(2.0 + s) * p - np.roll(p, 1) - np.roll(p, -1)


def operator_cases():
    """name -> (torch operator, torch diagonal, longdouble operator, n, the count the case is expected to take, or None: _cg's)"""
    cases = {}
    for n in NS:
        for k in KS:
            Mld, dld = diag_ld(n, k)
            cases[f"diag_n{n}_k{k}"] = (diag_op(n, k), diag_of(n, k), Mld, n, 1)
            cases[f"unit_diag_n{n}_k{k}"] = (diag_op(n, k), torch.ones(n, dtype=torch.float64), Mld, n, None)
    for name, s, n in (("unit_periodic_n33_s1", 1.0, 33), ("unit_periodic_n257_s1", 1.0, 257), ("unit_periodic_n257_s025", 0.25, 257)):
        cases[name] = (periodic_op(s), torch.ones(n, dtype=torch.float64), periodic_ld(s), n, None)
    for n in SCALED_NS:
        cases[f"scaled_n{n}"] = (scaled_op(n), scaled_diag(n), scaled_ld(n)[0], n, SCALED_COUNTS[n])
    return cases


def _run_driver(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(HERE, "native", "pcg_driver.cpp")])
    vec, wts = str(tmp_path / "rhs.f64"), str(tmp_path / "weights.f64")
    MASTER.tofile(vec)
    WEIGHTS.tofile(wts)
    r = subprocess.run([exe, vec, wts], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pcg driver ok" in r.stdout, r.stdout
    out = {}
    for line in r.stdout.splitlines()[:-1]:
        w = line.split()
        assert len(w) == 7, line
        out[w[0]] = dict(count=int(w[1]), rounds=int(w[2]), resnorm=float(w[3]), true_res=float(w[4]), bnorm=float(w[5]), ymax=float(w[6]))
    return out


@pytest.fixture(scope="module")
def reference():
    """name -> (simple._pcg's count, its true residual, |b|, the longdouble count, the longdouble history)"""
    ref = {}
    for name, (op, d, Mld, n, _) in operator_cases().items():
        b = rhs(n)
        y, k = simple._pcg(op, b, d, 100, RELTOL)
        _, kld, hist = R.solve(Mld, MASTER[:n], d.numpy(), maxiter=100, reltol=RELTOL)
        ref[name] = (k, float(torch.linalg.norm(b - op(y))), float(torch.linalg.norm(b)), kld, hist)
    return ref


def test_the_scaled_family_is_what_the_issue_says(reference):
    """Preconditioned counts 3 / 17 / 22; for n >= 255 no count hangs on a rounding (sqrt(rr) / tol is >= 1.70 before the last iteration and
    <= 0.38 after it, in longdouble); plain CG on the same systems stops at maxiter 100."""
    for n in SCALED_NS:
        k, _, _, kld, hist = reference[f"scaled_n{n}"]
        print("scaled", n, "count", k, "longdouble", kld, "sqrt(rr)/tol before / after the last iteration", hist[-2], hist[-1])
        assert k == kld == SCALED_COUNTS[n]
        if n >= 255:
            assert hist[-2] >= 1.70 and hist[-1] <= 0.38
            _, kplain = simple._cg(scaled_op(n), rhs(n), 100, RELTOL)
            assert kplain == 100


def test_unit_diagonal_gives_the_counts_of_plain_cg(reference):
    for name, (op, d, _, n, expected) in operator_cases().items():
        if expected is None:
            _, kplain = simple._cg(op, rhs(n), 100, RELTOL)
            assert reference[name][0] == reference[name][3] == kplain, name


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["O2", "asan_ubsan"])
def test_pcg_headers_equal_simple_pcg_and_the_longdouble_reference(tmp_path, reference, flags):
    got = _run_driver(tmp_path, flags, "pcg_driver")
    cases = operator_cases()
    assert set(cases) <= set(got)
    for name, (op, d, _, n, expected) in cases.items():
        k, res, bnorm, kld, hist = reference[name]
        g = got[name]
        print(name, "count", g["count"], "_pcg", k, "longdouble", kld, "true residual", g["true_res"], "_pcg", res, "tol", RELTOL * bnorm)
        assert g["count"] == k == kld, (name, g, k, kld)
        if expected is not None:
            assert g["count"] == expected, (name, g, expected)
        assert g["rounds"] == g["count"]
        assert g["bnorm"] == pytest.approx(bnorm, rel=1e-14)
        assert g["true_res"] <= max(RELTOL * bnorm, 2.0 * res), (name, g, res)
        assert g["resnorm"] <= RELTOL * bnorm
    for n in (255, 257, 4097):
        assert got[f"scaled_n{n}"]["resnorm"] <= 0.38 * RELTOL * got[f"scaled_n{n}"]["bnorm"] * (1 + 1e-6)
    # a zero right-hand side, maxiter = 0 and maxiter = 3
    assert got["zero_rhs"]["count"] == 0 and got["zero_rhs"]["rounds"] == 0 and got["zero_rhs"]["ymax"] == 0.0
    assert got["maxiter0"]["count"] == 0 and got["maxiter0"]["rounds"] == 0 and got["maxiter0"]["ymax"] == 0.0
    assert got["maxiter3"]["count"] == 3 and got["maxiter3"]["rounds"] == 3
    # abstol (1e-4) above reltol |b| stops earlier than reltol alone, at a residual within it
    a = got["abstol"]
    assert 1e-4 > RELTOL * a["bnorm"] and 0 < a["count"] < got["scaled_n257"]["count"] and a["resnorm"] <= 1e-4
    # M = diag(1, -1), b = (1, 2), d = 1: p.Mp = -3 in the first round -- the guard: count -1 - 0, y as it was
    assert got["indefinite"]["count"] == -1 and got["indefinite"]["rounds"] == 1 and got["indefinite"]["ymax"] == 0.0
    assert got["nan_operator"]["count"] < 0 and got["nan_operator"]["ymax"] == 0.0
    # a diagonal with a zero, a negative, an infinite, a NaN entry: stopped in begin, the operator never applied
    for kind in ("zero", "negative", "infinite", "nan"):
        g = got["bad_diag_" + kind]
        assert g["count"] == -1 and g["rounds"] == 0 and g["ymax"] == 0.0, (kind, g)
    assert got["zero_rhs_bad_diag"]["count"] == 0 and got["zero_rhs_bad_diag"]["ymax"] == 0.0


def test_simple_pcg_edge_cases():
    """simple._pcg and the longdouble reference take the same decisions as the headers at the edges."""
    n = 33
    op, d, (Mld, dld), b = scaled_op(n), scaled_diag(n), scaled_ld(n), rhs(n)
    for kw, expect in ((dict(maxiter=0), 0), (dict(maxiter=3), 3)):
        y, k = simple._pcg(op, b, d, kw["maxiter"], RELTOL)
        assert k == expect == R.solve(Mld, MASTER[:n], d.numpy(), maxiter=kw["maxiter"], reltol=RELTOL)[1]
    y, k = simple._pcg(op, torch.zeros(n, dtype=torch.float64), d, 100, RELTOL)
    assert k == 0 and float(y.abs().max()) == 0.0
    y, k = simple._pcg(op, b, d, 100, RELTOL, 1e-4)
    assert 0 < k < 17 and k == R.solve(Mld, MASTER[:n], d.numpy(), maxiter=100, reltol=RELTOL, abstol=1e-4)[1]
    ind = lambda p: torch.tensor([1.0, -1.0], dtype=torch.float64) * p
    y, k = simple._pcg(ind, torch.tensor([1.0, 2.0], dtype=torch.float64), torch.ones(2, dtype=torch.float64), 100, RELTOL)
    assert k == -1 and float(y.abs().max()) == 0.0
    assert R.solve(lambda p: np.array([1, -1], dtype=LD) * p, [1.0, 2.0], [1.0, 1.0])[1] == -1
    y, k = simple._pcg(lambda p: p * float("nan"), b, d, 100, RELTOL)
    assert k == -1 and float(y.abs().max()) == 0.0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        dd = d.clone()
        dd[7] = bad
        y, k = simple._pcg(op, b, dd, 100, RELTOL)
        assert k == -1 and float(y.abs().max()) == 0.0, bad
        assert R.solve(Mld, MASTER[:n], dd.numpy())[1] == -1


def test_pcg_entry_points_are_exported_and_refuse_bad_arguments():
    path = B.build_lbfgs_library()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    names = {"muse_lbfgs_pcg_begin", "muse_lbfgs_pcg_advance"}
    assert names <= exported and names <= set(B.lbfgs_declared_symbols()) and names <= set(_capi.LBFGS_SIGNATURES)
    assert exported == set(B.lbfgs_declared_symbols()) == set(_capi.LBFGS_SIGNATURES)
    for f in ("pcg_control.hpp", "pcg_advance.hpp", "pcg_kernels.hpp"):
        assert os.path.join(B.LBFGS_DIR, f) in B._LBFGS_DEPS
    lib = _capi.load_lbfgs_library()
    # the workspace is the plain solver's: one record per row (256-byte aligned) and two vectors, y and r
    assert lib.muse_lbfgs_cg_workspace_bytes(3, 7) == 256 + 3 * 2 * 7 * 8
    # bad arguments are answered before anything touches a device (a non-null pointer is never followed)
    buf = np.zeros(64)
    p = buf.ctypes.data
    begin = lambda ws, nrows, n, b, d, k, pe, act: lib.muse_lbfgs_pcg_begin(ws, nrows, n, b, d, k, RELTOL, 0.0, 100, pe, act, None)
    assert begin(None, 1, 4, p, p, 1, p, p) == -1
    assert begin(p, 1, 4, None, p, 1, p, p) == -1
    assert begin(p, 1, 4, p, None, 1, p, p) == -1
    assert begin(p, 1, 4, p, p, 1, None, p) == -1
    assert begin(p, 1, 4, p, p, 1, p, None) == -1
    assert begin(p, 0, 4, p, p, 1, p, p) == -1 and begin(p, 1, 0, p, p, 1, p, p) == -1
    assert begin(p, 3, 4, p, p, 0, p, p) == -1 and begin(p, 3, 4, p, p, -1, p, p) == -1
    assert begin(p, 4, 4, p, p, 3, p, p) == -1 and begin(p, 1, 4, p, p, 3, p, p) == -1        # nrows is no multiple of rows_per_diag
    adv = lambda ws, nrows, n, Mp, d, k, pe, act: lib.muse_lbfgs_pcg_advance(ws, nrows, n, Mp, d, k, pe, act, None)
    assert adv(None, 1, 4, p, p, 1, p, p) == -1
    assert adv(p, 1, 4, None, p, 1, p, p) == -1
    assert adv(p, 1, 4, p, None, 1, p, p) == -1
    assert adv(p, 1, 4, p, p, 1, None, p) == -1
    assert adv(p, 1, 4, p, p, 1, p, None) == -1
    assert adv(p, 0, 4, p, p, 1, p, p) == -1 and adv(p, 1, 0, p, p, 1, p, p) == -1
    assert adv(p, 3, 4, p, p, 0, p, p) == -1 and adv(p, 4, 4, p, p, 3, p, p) == -1


def test_pcg_kernels_resources():
    """No kernel of the library spills or uses scratch; the preconditioned round kernel at 1024 threads (4 wavefronts per SIMD) fits 128
    registers, as the plain step kernel; the new kernels' names leave the plain kernels' counts as they were."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regs
    rows = regs.library_report(B.build_lbfgs_library())
    for name, vgpr, vspill, sspill, scratch, dyn in rows:
        assert vspill == 0 and scratch == 0 and not dyn, (name, vgpr, vspill, scratch, dyn)
    start = [r for r in rows if "precond_start_kernel" in r[0]]
    rnd = [r for r in rows if "precond_round_kernel" in r[0]]
    assert len(start) == 2 and len(rnd) == 2, rows
    assert all(r[1] <= 128 for r in rnd + start), (rnd, start)
    cg = [r for r in rows if "cg_" in r[0]]
    assert not [r for r in cg if "advance_kernel" in r[0]]
    step = [r for r in cg if "cg_step_kernel" in r[0]]
    assert len(step) == 2 and len([r for r in cg if "cg_begin_kernel" in r[0]]) == 2, rows
    assert len([r for r in cg if "cg_result_kernel" in r[0]]) == 2 and len([r for r in cg if "cg_count_kernel" in r[0]]) == 1, rows
    assert all(r[1] <= 128 for r in step), step
    assert len([r for r in rows if "advance_kernel" in r[0]]) == 2
