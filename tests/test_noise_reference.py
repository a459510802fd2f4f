"""CPU checks of the stencil model with run-time noise (muse_set_noise): the longdouble reference (tests/noise_reference.py) against
stencil_reference and against closed forms, the boundary (header, exports, ctypes, Julia shim), and the new kernels' registers from
the built library's own code object.  No GPU, no oracle."""
import importlib.util
import os
import re

import numpy as np
import pytest

import hp_reference as R
import noise_reference as Q
import stencil_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)

PAIRS = [(0.5, 0.25), (0.3, 0.35)]


def _noise(N, seed=3):
    """A ramp sd in [0.5, 2] and a mask of ~5 % that includes the wrap (0 and N - 1) and never a whole block of up to 12."""
    sd = np.linspace(0.5, 2.0, N)
    mask = np.ones(N, bool)
    mask[[0, N - 1]] = False
    mask[np.random.default_rng(seed).choice(np.arange(1, N - 1), size=max(1, N // 20), replace=False)] = False
    if N >= 24:
        mask[np.arange(12) * N // 12 + 1] = True
    return sd, mask


# ------------------------------------------------------------------------------------------------ 1. neutral noise
@needs_ld
@pytest.mark.parametrize("w", PAIRS)
@pytest.mark.parametrize("N,theta", [(5, [0.3]), (64, [1.0, -0.5]), (301, [1.0, 2.0, 3.0, 0.5])])
def test_unit_noise_without_a_mask_is_stencil_reference_exactly(w, N, theta):
    om, s = Q.weights(N)
    assert np.array_equal(om, np.ones(N)) and np.array_equal(s, np.ones(N))
    xq, zq, cq = Q.sample_x_z(N, 7, 3, theta, w, s)
    xs, zs, cs = S.sample_x_z(N, 7, 3, theta, w)
    assert np.array_equal(xq, xs) and np.array_equal(zq, zs) and np.array_equal(cq, cs)
    x, z = xs.astype(np.float64), (0.7 * zs + 0.1).astype(np.float64)
    for a, b in zip(Q.objective(x, z, theta, w, om), S.objective(x, z, theta, w)):
        assert np.array_equal(a, b)
    assert np.array_equal(Q.exact_map(x, theta, w, om), S.exact_map(x, theta, w))
    assert np.array_equal(Q.implicit_H(N, 17, 1, theta, w, om, s)[0], S.implicit_H(N, 17, 1, theta, w))
    assert np.array_equal(Q.hessian(N, theta, w, om), S.hessian(N, theta, w))


@needs_ld
def test_weights_are_the_two_rounded_operations():
    sd = np.array([0.1, 0.3, 1.0, 1.7, 3.0])
    om, s = Q.weights(5, sd, [1, 1, 0, 1, 1])
    assert np.array_equal(om.astype(np.float64), [1.0 / (0.1 * 0.1), 1.0 / (0.3 * 0.3), 0.0, 1.0 / (1.7 * 1.7), 1.0 / (3.0 * 3.0)])
    assert np.array_equal(s.astype(np.float64), [0.1, 0.3, 0.0, 1.7, 3.0])


# ------------------------------------------------------------------------------------------------ 2. the gradient, the mask, the MAP
@needs_ld
@pytest.mark.parametrize("w", PAIRS)
@pytest.mark.parametrize("N,theta", [(7, [0.4]), (97, [1.0, -0.5, 0.2])])
def test_gradient_is_the_central_difference_of_the_objective(w, N, theta):
    """f is quadratic in z: a central difference has NO truncation error, only the longdouble rounding of f (2^-64 cond-sized),
    divided by 2 h."""
    sd, mask = _noise(N)
    om, s = Q.weights(N, sd, mask)
    x = Q.sample_x_z(N, 11, 0, theta, w, s)[0].astype(np.float64)
    z = (0.6 * Q.sample_x_z(N, 11, 0, theta, w, s)[1] + 0.2).astype(np.float64)
    f0, g, cf, _ = Q.objective(x, z, theta, w, om)
    h = 2.0 ** -10          # a power of two: z +- h e_i is exact in fp64
    for i in list(range(0, N, max(1, N // 9))) + [N - 1]:
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        fd = (Q.objective(x, zp, theta, w, om)[0] - Q.objective(x, zm, theta, w, om)[0]) / R.LD(2 * h)
        assert abs(fd - g[i]) <= 2.0 ** -58 * float(cf) / h, (i, float(fd), float(g[i]))


@needs_ld
def test_a_masked_elements_x_changes_nothing():
    N, theta, w = 97, [1.0, -0.5, 0.2], (0.3, 0.35)
    sd, mask = _noise(N)
    om, s = Q.weights(N, sd, mask)
    x, zt, _ = Q.sample_x_z(N, 11, 0, theta, w, s)
    assert np.all(x[~mask] == 0) and np.all(x[mask] != 0)
    x = x.astype(np.float64)
    z = (0.6 * zt + 0.2).astype(np.float64)
    x2 = x.copy()
    x2[~mask] = 1e30
    for a, b in zip(Q.objective(x, z, theta, w, om), Q.objective(x2, z, theta, w, om)):
        assert np.array_equal(a, b)
    assert np.array_equal(Q.exact_map(x, theta, w, om), Q.exact_map(x2, theta, w, om))
    # ... and an observed element's does
    x3 = x.copy()
    x3[np.flatnonzero(mask)[5]] += 1.0
    assert Q.objective(x3, z, theta, w, om)[0] != Q.objective(x, z, theta, w, om)[0]


@needs_ld
@pytest.mark.parametrize("w", PAIRS)
def test_dense_map_zeroes_the_gradient_and_cg_agrees(w):
    N, theta = 301, [1.0, -0.5, 0.2, 0.7]
    sd, mask = _noise(N)
    om, s = Q.weights(N, sd, mask)
    x = Q.sample_x_z(N, 11, 0, theta, w, s)[0].astype(np.float64)
    zd = Q.exact_map(x, theta, w, om, dense=True)
    zc = Q.exact_map(x, theta, w, om, dense=False)
    lam = float(np.exp(-np.max(theta)))
    b = S.stencil(om * x, w)
    assert np.abs(zd - zc).max() <= 2e-16 * float(np.sqrt(np.dot(b, b))) / lam
    _, g, _, cg = Q.objective(x, zd.astype(np.float64), theta, w, om)        # (objective rounds z to fp64: allow that rounding)
    lam_max = float(om.max()) * (abs(w[0]) + 2 * abs(w[1])) ** 2 + float(np.exp(-np.min(theta)))
    assert np.abs(g).max() <= 2.0 ** -53 * lam_max * np.abs(zd).max() * 2 + 2.0 ** -58 * cg.max()
    # the dense Hessian's smallest eigenvalue is at least min e^-theta, mask or not
    ev = np.linalg.eigvalsh(Q.hessian(N, theta, w, om).astype(np.float64))
    assert ev.min() >= lam * (1 - 1e-12)


# ------------------------------------------------------------------------------------------------ 3. H and the marginal
@needs_ld
def test_mean_implicit_H_approaches_the_expected_information():
    """E over simulations of get_H!'s per-simulation H is the information of the marginal likelihood, 1/2 tr(C^-1 D_i C^-1 D_j):
    within 5 Monte-Carlo standard errors entry by entry."""
    N, theta, w, nsims = 48, [0.8, -0.3], (0.3, 0.35), 300
    sd, mask = _noise(N)
    om, s = Q.weights(N, sd, mask)
    F = Q.expected_information(N, theta, w, om)
    Hs = np.array([Q.implicit_H(N, 5, i, theta, w, om, s)[0].astype(np.float64) for i in range(nsims)])
    err = Hs.std(axis=0, ddof=1) / np.sqrt(nsims)
    assert np.all(np.abs(Hs.mean(axis=0) - F) <= 5 * err), (Hs.mean(axis=0), F, err)
    assert np.all(err[np.diag_indices(2)] < 0.1 * np.abs(np.diag(F)))         # (the comparison has resolving power)


@needs_ld
def test_marginal_gradient_is_the_score_minus_its_expectation():
    """The exact marginal gradient (dense Gaussian algebra over the observed elements) equals MUSE's identity at the exact MAPs within
    the Monte-Carlo error of the expectation; and it is the central difference of the dense marginal log-likelihood."""
    N, theta, w = 40, [0.6, -0.4], (0.5, 0.25)
    sd, mask = _noise(N)
    om, s = Q.weights(N, sd, mask)
    x = Q.sample_x_z(N, 9, 0, [1.0, 0.2], w, s)[0].astype(np.float64)
    gm = Q.marginal_gradient(x, theta, w, om).astype(np.float64)
    est, err = Q.marginal_gradient_mc(x, theta, w, om, s, 21, 400)
    assert np.all(np.abs(est - gm) <= 5 * err), (est, gm, err)

    def logp(th):
        k = R.blocks(N, 2)
        A = S.dense_A(N, w)[mask]
        Cm = A @ (np.exp(np.asarray(th).astype(R.LD))[k][:, None] * A.T) + np.diag(R.LD(1) / om[mask])
        L = S.cholesky(Cm)
        xo = x.astype(R.LD)[mask]
        return -R.LD(0.5) * np.dot(xo, S.chol_solve(L, xo)) - np.log(np.diag(L)).sum()
    h = 1e-5
    for j in range(2):
        tp, tm = np.array(theta), np.array(theta)
        tp[j] += h
        tm[j] -= h
        assert abs(float((logp(tp) - logp(tm)) / (2 * h)) - gm[j]) <= 1e-8 * max(1.0, abs(gm[j]))


# ------------------------------------------------------------------------------------------------ 4. the boundary
def test_header_ctypes_and_shim_name_the_noise_entry_points(M):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muse_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "julia", "HipMuseInference.jl")).read()
    import ctypes
    lib = ctypes.CDLL(M.build_extension())
    for name in ("muse_set_noise", "muse_get_noise"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in M._capi.SIGNATURES, name
        assert "ccall((:%s, libmuse_hip)" % name in shim, name
    # the argument lists agree in length: header, ctypes table, shim
    for name, nargs in (("muse_set_noise", 4), ("muse_get_noise", 4)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, text).group(1)
        assert decl.count(",") + 1 == nargs and len(M._capi.SIGNATURES[name][1]) == nargs, name
        call = re.search(r"ccall\(\(:%s, libmuse_hip\), Cint, \(([^)]*)\)" % name, shim).group(1)
        assert len([a for a in call.split(",") if a.strip()]) == nargs, (name, call)
    assert "muse_set_noise" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import inspect
    params = inspect.signature(M.HipMuseProblem.__init__).parameters
    assert "noise_sd" in params and "mask" in params
    for cls in (M.HipMuseProblem, M.ShardedMuseProblem):
        assert hasattr(cls, "set_noise") and hasattr(cls, "get_noise")


# ------------------------------------------------------------------------------------------------ 5. the new kernels' resources
def _regs():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    return regs


SCRATCH_BOUND = 256     # bytes per lane: the product's bound on a solver kernel's private segment


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="llvm-readelf not available")
def test_runtime_noise_kernels_keep_the_budget(M):
    """Every map_score_kernel<SmoothNoiseModel<B>, Place, IMPLICIT> of the built library: one for every SmoothTapsModel kernel,
    no device-function call (no dynamic stack), scratch within the product bound of 256 B per lane, and no spilled vector
    register where the taps twin has none."""
    rows = {r[0]: r for r in _regs().library_report(M.build_extension())}
    noise = {k: r for k, r in rows.items() if "16SmoothNoiseModel" in k}
    twins = {k: r for k, r in rows.items() if "15SmoothTapsModel" in k}
    assert len(twins) >= 24 and len(noise) == len(twins)
    for k, r in noise.items():
        twin = twins[k.replace("16SmoothNoiseModel", "15SmoothTapsModel")]
        _, vgpr, vspill, sspill, scratch, dyn = r
        print(k, "vgpr", vgpr, "vspill", vspill, "sspill", sspill, "scratch", scratch, "| twin", twin[1:])
        assert not dyn, r
        assert scratch <= SCRATCH_BOUND, r
        assert vspill <= twin[2], (r, twin)
        assert vgpr <= 256, r
