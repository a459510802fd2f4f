"""CPU checks of the stencil model with run-time weights (muse_set_stencil): the longdouble reference against hp_reference and
against closed forms, the boundary (header, exports, ctypes, Julia shim), and the new kernels' registers from the built library's
own code object.  No GPU, no oracle."""
import importlib.util
import os
import re

import numpy as np
import pytest

import hp_reference as R
import stencil_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)

PAIRS = [(0.7, 0.15), (0.6, -0.2), (0.0, 0.5), (1.0, 0.0), (0.5, 0.25)]


# ------------------------------------------------------------------------------------------------ 1. the built-in pair
@needs_ld
@pytest.mark.parametrize("N,theta", [(5, [0.3]), (64, [1.0, -0.5]), (601, [1.0, 2.0, 3.0, 0.5]), (1000, list(np.linspace(-1, 1.5, 12)))])
def test_reference_at_the_builtin_weights_is_hp_reference(N, theta):
    """(1/2, 1/4) are powers of two: every product by a weight is exact, so the two restatements agree to longdouble rounding."""
    xs, zs, _ = S.sample_x_z(N, 7, 3, theta, S.BUILTIN)
    xr, zr = R.sample_x_z("smooth", N, 7, 3, theta)
    assert np.array_equal(zs, zr)
    tiny = 2.0 ** -60
    assert np.abs(xs - xr).max() <= tiny * np.abs(xr).max()
    x, z = xr.astype(np.float64), (0.7 * zr + 0.1).astype(np.float64)
    fs, gs, cfs, cgs = S.objective(x, z, theta, S.BUILTIN)
    fr, gr, cfr, cgr = R.objective("smooth", x, z, theta)
    assert abs(fs - fr) <= tiny * abs(fr) and np.abs(gs - gr).max() <= tiny * np.abs(cgr).max()
    assert abs(cfs - cfr) <= tiny * cfr and np.abs(cgs - cgr).max() <= tiny * cgr.max()
    s1, c1 = S.score(x, z, theta)
    s2, c2 = R.score("smooth", x, z, theta)
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2)
    if N <= 400:
        zm = S.exact_map(x, theta, S.BUILTIN)
        assert np.abs(zm - R.exact_map("smooth", x, theta)).max() <= 2.0 ** -50 * np.abs(zm).max()
        Hs, Hr = S.implicit_H(N, 17, 1, theta, S.BUILTIN), R.implicit_H("smooth", N, 17, 1, theta)
        assert np.abs(Hs - Hr).max() <= 2.0 ** -45 * np.abs(Hr).max()


# ------------------------------------------------------------------------------------------------ 2. closed forms, per pair
@needs_ld
@pytest.mark.parametrize("w", PAIRS)
@pytest.mark.parametrize("N,theta", [(5, [0.4]), (97, [1.0, -0.5, 0.2]), (400, [1.5])])
def test_dense_map_zeroes_the_gradient_and_the_two_marginals_agree(w, N, theta):
    x = S.sample_x_z(N, 11, 0, theta, w)[0].astype(np.float64)
    zs = S.exact_map(x, theta, w)
    # the gradient at the longdouble MAP, evaluated in longdouble: below 2^-55 of its own condition sum
    _, g, _, cg = S.objective(x, zs.astype(np.float64), theta, w)        # (objective rounds z to fp64: allow that rounding)
    lam_max = float((abs(w[0]) + 2 * abs(w[1])) ** 2 + np.exp(-np.min(theta)))
    assert np.abs(g).max() <= 2.0 ** -53 * lam_max * np.abs(zs).max() * 2 + 2.0 ** -58 * cg.max()
    if len(theta) == 1:
        md, mf = S.marginal_dense(x, theta[0], w), S.marginal_fft(x, theta[0], w)
        assert abs(md - mf) <= 2.0 ** -50 * N * max(1.0, abs(float(md)))
        # the dense Hessian's spectrum is a_q^2 + e^-theta: its smallest eigenvalue is at least e^-theta
        aq = S.a_q(N, w).astype(np.float64)
        ev = np.linalg.eigvalsh(S.hessian(N, theta, w).astype(np.float64))
        np.testing.assert_allclose(np.sort(ev), np.sort(aq ** 2 + np.exp(-theta[0])), rtol=1e-10, atol=1e-12)


@needs_ld
def test_expected_information_is_the_curvature_of_the_fft_marginal():
    """-E d^2/dtheta^2 of the mode-by-mode marginal: 1/2 sum_q (u_q / (1 + u_q))^2, u_q = e^theta a_q^2 -- against a central second
    difference of the EXPECTED marginal -1/2 sum_q [(1 + u_q(t0)) / (1 + u_q(t)) + log(1 + u_q(t))]."""
    N, t0, w, h = 300, 0.8, (0.6, -0.2), 1e-4
    a2 = S.a_q(N, w) ** 2
    u0 = np.exp(R.LD(t0)) * a2
    EL = lambda t: -R.LD(0.5) * (((1 + u0) / (1 + np.exp(R.LD(t)) * a2)) + np.log(1 + np.exp(R.LD(t)) * a2)).sum()
    curv = -(EL(t0 + h) - 2 * EL(t0) + EL(t0 - h)) / R.LD(h) ** 2
    assert abs(float(curv) - S.expected_information(N, t0, w)) <= 1e-6 * S.expected_information(N, t0, w)


# ------------------------------------------------------------------------------------------------ 3. the boundary
def test_header_ctypes_and_shim_name_the_stencil_entry_points(M):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muse_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "julia", "HipMuseInference.jl")).read()
    import ctypes
    lib = ctypes.CDLL(M.build_extension())
    for name in ("muse_set_stencil", "muse_get_stencil"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in M._capi.SIGNATURES, name
        assert "ccall((:%s, libmuse_hip)" % name in shim, name
    assert "muse_set_stencil" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import inspect
    assert "stencil" in inspect.signature(M.HipMuseProblem.__init__).parameters
    assert hasattr(M.HipMuseProblem, "set_stencil") and hasattr(M.ShardedMuseProblem, "set_stencil")


# ------------------------------------------------------------------------------------------------ 4. the new kernels' resources
def _regs():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    return regs


def _kernel_notes(path):
    """{kernel name: its metadata block} of every gfx950 kernel of a built library (llvm-readelf --notes on each code object)."""
    import struct
    import subprocess
    import tempfile
    data, out, start = open(path, "rb").read(), {}, 0
    while True:
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", start)
        if i < 0:
            return out
        n, = struct.unpack_from("<Q", data, i + 24)
        pos, end = i + 32, i + 32
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, pos)
            pos += 24
            tid = data[pos:pos + idlen].decode()
            pos += idlen
            if "gfx950" in tid:
                with tempfile.NamedTemporaryFile(suffix=".co") as f:
                    f.write(data[i + off:i + off + size])
                    f.flush()
                    txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
                for b in txt.split("- .agpr_count:")[1:]:
                    out[re.search(r"\.name:\s+(\S+)", b).group(1)] = b
            end = max(end, i + off + size)
        start = max(end, i + 24)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="llvm-readelf not available")
def test_runtime_taps_kernels_keep_the_builtin_twins_budget(M):
    """Every map_score_kernel<SmoothTapsModel<B>, Place, IMPLICIT> of the built library: no scratch, no device-function call, and
    no spilled vector register where its SmoothModel<B> twin has none; and there is one for every built-in stencil kernel."""
    rows = {r[0]: r for r in _regs().library_report(M.build_extension())}
    taps = {k: r for k, r in rows.items() if "15SmoothTapsModel" in k}
    twins = {k: r for k, r in rows.items() if "11SmoothModel" in k}
    assert len(twins) >= 24 and len(taps) == len(twins)
    for k, r in taps.items():
        twin = twins[k.replace("15SmoothTapsModel", "11SmoothModel")]
        _, vgpr, vspill, sspill, scratch, dyn = r
        assert scratch == 0 and not dyn, r
        assert vspill <= twin[2], (r, twin)
        assert vgpr <= 256, r
    # the new per-simulation operator kernels (which regs.py's report, made for the solver kernels, leaves out): no scratch, no
    # spilled register, no call either
    notes = _kernel_notes(M.build_extension())
    small = {n: b for n, b in notes.items() if ("loglike_kernel" in n and "SmoothTapsModel" in n) or "smooth_finish_taps_kernel" in n}
    assert len(small) == 3, sorted(small)
    for n, b in small.items():
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1))
        assert g("private_segment_fixed_size") == 0 and g("vgpr_spill_count") == 0 and g("sgpr_spill_count") == 0, n
        assert not re.search(r"\.uses_dynamic_stack:\s+true", b), n
