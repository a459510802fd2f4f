"""CPU checks of the stencil model with a response behind the operator (muse_set_link): the longdouble reference
(tests/link_reference.py) against noise_reference at (0, 0) and against its own definitions, the line-search cases the GPU test
keeps (their evaluation counts must not depend on the order of the sums), the boundary (header, exports, ctypes, Julia shim), and
the new kernels' registers from the built library's own code object.  No GPU, no oracle."""
import importlib.util
import os
import re

import numpy as np
import pytest

import hp_reference as R
import link_reference as L
import noise_reference as Q
import stencil_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)

PAIRS = [(0.5, 0.25), (0.3, 0.35)]
LINKS = [(0.25, 0.5), (0.4, 0.3), (-0.2, 0.1)]


def _noise(N, seed=3):
    """test_noise_reference's: a ramp sd in [0.5, 2] and a mask of ~5 % that includes the wrap and never a whole block of up to 12."""
    sd = np.linspace(0.5, 2.0, N)
    mask = np.ones(N, bool)
    mask[[0, N - 1]] = False
    mask[np.random.default_rng(seed).choice(np.arange(1, N - 1), size=max(1, N // 20), replace=False)] = False
    if N >= 24:
        mask[np.arange(12) * N // 12 + 1] = True
    return sd, mask


# ------------------------------------------------------------------------------------------------ 1. the neutral link
@needs_ld
@pytest.mark.parametrize("link", [(0.0, 0.0), None])
@pytest.mark.parametrize("w", PAIRS)
@pytest.mark.parametrize("N,theta", [(5, [0.3]), (64, [1.0, -0.5]), (301, [1.0, 2.0, 3.0, 0.5])])
def test_the_zero_link_is_noise_reference_exactly(w, N, theta, link):
    sd, mask = _noise(N)
    om, s = L.weights(N, sd, mask)
    xl, zl, cl = L.sample_x_z(N, 7, 3, theta, w, s, link)
    xq, zq, cq = Q.sample_x_z(N, 7, 3, theta, w, s)
    assert np.array_equal(xl, xq) and np.array_equal(zl, zq) and np.array_equal(cl, cq)
    x, z = xq.astype(np.float64), (0.7 * zq + 0.1).astype(np.float64)
    for a, b in zip(L.objective(x, z, theta, w, om, link), Q.objective(x, z, theta, w, om)):
        assert np.array_equal(a, b)
    for a, b in zip(L.score(x, z, theta), Q.score(x, z, theta)):
        assert np.array_equal(a, b)
    assert np.array_equal(L.hessian(x, z, theta, w, om, link), Q.hessian(N, theta, w, om))
    assert L.hessian_floor(x, z, theta, w, om, link) == float(np.exp(-np.max(theta)))
    # (Newton on a quadratic is ONE solve of the same system: the same MAP up to the stopping rule of either)
    zq_map = Q.exact_map(x, theta, w, om)
    for dense in (True, False):
        zs = L.exact_map(x, theta, w, om, link, dense=dense)
        assert np.abs(zs - zq_map).max() <= 1e-15 * max(1.0, float(np.abs(zq_map).max()))
    sl, _ = L.score_at_exact_map(x, theta, w, om, link)
    sq, _ = Q.score_at_exact_map(x, theta, w, om)
    assert np.abs(sl - sq).max() <= 1e-13 * max(1.0, float(np.abs(sq).max()))


# ------------------------------------------------------------------------------------------------ 2. gradient, Hessian, MAP
@needs_ld
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("w", PAIRS)
@pytest.mark.parametrize("N,theta", [(7, [0.4]), (97, [1.0, -0.5, 0.2])])
def test_gradient_is_the_central_difference_of_the_objective(w, N, theta, link):
    """f is a polynomial of degree 6 in z: the central difference's truncation error is h^2 / 6 f''' + O(h^4); with the Hessian's
    own central difference as the scale of f''' h (|H(z + h) - H(z - h)| / 2 ~ |f'''| h) the tolerance below is that term with
    room, plus the longdouble rounding of f divided by 2 h."""
    sd, mask = _noise(N)
    om, s = L.weights(N, sd, mask)
    x = L.sample_x_z(N, 11, 0, theta, w, s, link)[0].astype(np.float64)
    z = (0.6 * L.sample_x_z(N, 11, 0, theta, w, s, link)[1] + 0.2).astype(np.float64)
    f0, g, cf, cg = L.objective(x, z, theta, w, om, link)
    h = 2.0 ** -14          # a power of two: z +- h e_i is exact in fp64
    for i in list(range(0, N, max(1, N // 9))) + [N - 1]:
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        fd = (L.objective(x, zp, theta, w, om, link)[0] - L.objective(x, zm, theta, w, om, link)[0]) / R.LD(2 * h)
        d3 = np.abs(L.hessian(x, zp, theta, w, om, link)[i, i] - L.hessian(x, zm, theta, w, om, link)[i, i]) / 2
        assert abs(fd - g[i]) <= float(d3) * h + 2.0 ** -58 * float(cf) / h, (i, float(fd), float(g[i]))
    # ... and the Hessian is the central difference of the gradient (one column)
    i = N // 2
    zp, zm = z.copy(), z.copy()
    zp[i] += h
    zm[i] -= h
    col = (L.objective(x, zp, theta, w, om, link)[1] - L.objective(x, zm, theta, w, om, link)[1]) / R.LD(2 * h)
    H = L.hessian(x, z, theta, w, om, link)
    assert np.abs(col - H[:, i]).max() <= 1e-6 * max(1.0, float(np.abs(H[:, i]).max()))


@needs_ld
@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("w", PAIRS)
def test_dense_and_matrix_free_exact_map_agree(w, link):
    N, theta = 301, [1.0, -0.5, 0.2, 0.7]
    sd, mask = _noise(N)
    om, s = L.weights(N, sd, mask)
    x = L.sample_x_z(N, 11, 0, theta, w, s, link)[0].astype(np.float64)
    zd = L.exact_map(x, theta, w, om, link, dense=True)
    zc = L.exact_map(x, theta, w, om, link, dense=False)
    _, g, _, cg = L.objective(x, zd.astype(np.float64), theta, w, om, link)
    # both end at |g| <= 1e-16 max(cond_g); the eigenvalues of the dense Hessian at the MAP carry that into z
    ev = np.linalg.eigvalsh(L.hessian(x, zd, theta, w, om, link).astype(np.float64))
    assert ev.min() > 0
    assert np.abs(zd - zc).max() <= 2 * 1e-16 * float(cg.max()) * np.sqrt(N) / ev.min()
    assert L.hessian_floor(x, zd, theta, w, om, link) <= ev.min() * (1 + 1e-12)       # (the floor is a lower bound)
    # a masked element's x changes nothing
    x2 = x.copy()
    x2[~mask] = 1e30
    assert np.array_equal(L.exact_map(x2, theta, w, om, link, dense=True), zd)
    # Newton from the MAP stays there
    assert np.abs(L.exact_map(x, theta, w, om, link, z_start=zd) - zd).max() <= 1e-17


@needs_ld
def test_muse_gradient_vanishes_in_expectation_at_the_truth():
    """E_x[score(z*(x))] is what the simulations' mean estimates: with the data drawn at theta itself the MUSE gradient is zero
    within the Monte-Carlo error of the two means."""
    N, theta, w, link, nsims = 60, [0.5, -0.2], (0.5, 0.25), (0.25, 0.5), 200
    sd, mask = _noise(N)
    om, s = L.weights(N, sd, mask)
    gs = []
    for d in range(12):
        x = L.sample_x_z(N, 900 + d, 0, theta, w, s, link)[0].astype(np.float64)
        gs.append(L.score_at_exact_map(x, theta, w, om, link)[0].astype(np.float64))
    sims = np.array([L.score_at_exact_map(L.sample_x_z(N, 31, i, theta, w, s, link)[0].astype(np.float64), theta, w, om, link)[0]
                     .astype(np.float64) for i in range(nsims)])
    err = np.sqrt(sims.var(axis=0, ddof=1) * (1 / nsims + 1 / len(gs)))
    assert np.all(np.abs(np.mean(gs, axis=0) - sims.mean(axis=0)) <= 5 * err)
    x = L.sample_x_z(N, 900, 0, theta, w, s, link)[0].astype(np.float64)
    g = L.muse_gradient(x, theta, w, om, s, link, 31, nsims)
    assert np.allclose(g, gs[0] - sims.mean(axis=0), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 3. the line-search cases
def test_hard_case_counts_do_not_depend_on_the_order_of_the_sums(M):
    """tests/test_gpu_link.py asserts that the engine's (iterations, f_calls) equal optim.lbfgs's on the fp64 numpy objective.  That
    equality across summation orders is empirical, so only cases whose path is insensitive to it are kept: every case of
    link_cases.HARD reaches atol with the same counts in every order of link_cases.ORDERS (exactly rounded, sequential, reversed,
    4 / 8 / 16 interleaved lanes, numpy's pairwise) and with f and g moved by up to an ulp at random, and the link makes the solve take more evaluations than the quadratic
    model's solve of the same data."""
    import link_cases as C
    for case in C.HARD:
        x, fgs, fg_quad = C.hard_problem(case)
        counts = {}
        for name, fg in fgs.items():
            z, info = C.lbfgs(M, fg, x.size, C.ATOL)
            assert info["status"] == 0, (case, name, info)
            counts[name] = (int(info["iterations"]), int(info["f_calls"]))
        assert len(set(counts.values())) == 1, (case, counts)
        _, iq = C.lbfgs(M, fg_quad, x.size, C.ATOL)
        assert iq["status"] == 0 and counts["exact"][1] > int(iq["f_calls"]), (case, counts, iq)


@needs_ld
@pytest.mark.parametrize("w", [None, (0.3, 0.35)])
@pytest.mark.parametrize("N,nth", [(301, 1), (7001, 4), (70001, 4), (1500, 12)])
def test_the_gpu_cases_satisfy_the_hessian_floor_with_room(N, nth, w):
    """The positivity of lambda = min e^-theta - |A|_2^2 max(0, -c) that tests/test_gpu_link.py asserts is a condition on the inputs
    (link, sd, theta), not a measurement: the reference alone satisfies it here, at the exact MAP of the reference's own draw of
    every shape, with room -- at theta ~ -4, omega |r| <~ 9 and |phi''| <~ 2.3 leave about 49 - 21 by that estimate; the computed floors are 48.7 .. 56.3, u being small at these theta."""
    import link_cases as C
    from test_gpu_noise_weights import noise_of, theta_of
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    sd, mask, _ = noise_of(N, nth)
    om, s = L.weights(N, sd, mask)
    x = L.sample_x_z(N, 42, 3, theta, wr, s, C.LINK)[0].astype(np.float64)
    zs = L.exact_map(x, theta, wr, om, C.LINK)
    lam = L.hessian_floor(x, zs, theta, wr, om, C.LINK)
    print("floor", lam, "of", float(np.exp(-np.max(theta))))
    assert lam >= 20.0, lam
    assert L.hessian_floor(x, np.zeros(N), theta, wr, om, C.LINK) >= 20.0                # ... and at the zero start


# ------------------------------------------------------------------------------------------------ 4. the boundary
def test_header_ctypes_and_shim_name_the_link_entry_points(M):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "muse_hip.h")).read(), flags=re.S)
    shim = open(os.path.join(ROOT, "julia", "HipMuseInference.jl")).read()
    import ctypes
    lib = ctypes.CDLL(M.build_extension())
    for name in ("muse_set_link", "muse_get_link"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(lib, name), name
        assert name in M._capi.SIGNATURES, name
        assert "ccall((:%s, libmuse_hip)" % name in shim, name
    for name, nargs in (("muse_set_link", 2), ("muse_get_link", 3)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, text).group(1)
        assert decl.count(",") + 1 == nargs and len(M._capi.SIGNATURES[name][1]) == nargs, name
        call = re.search(r"ccall\(\(:%s, libmuse_hip\), Cint, \(([^)]*)\)" % name, shim).group(1)
        assert len([a for a in call.split(",") if a.strip()]) == nargs, (name, call)
    assert "muse_set_link" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import inspect
    assert "link" in inspect.signature(M.HipMuseProblem.__init__).parameters
    for cls in (M.HipMuseProblem, M.ShardedMuseProblem):
        assert hasattr(cls, "set_link") and hasattr(cls, "get_link")
    # the sentence get_H_(implicit_diff=True) raises with is the engine's own
    from museinference_jl_amd import problem
    src = open(os.path.join(ROOT, "museinference.jl_amd", "csrc", "muse_engine.cpp")).read()
    said = "".join(re.findall(r'"([^"]*)"', src[src.index("kLinkImplicitRefusal ="):src.index(";", src.index("kLinkImplicitRefusal ="))]))
    assert said == problem.LINK_IMPLICIT_REFUSAL


# ------------------------------------------------------------------------------------------------ 5. the new kernels' resources
def _regs():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    return regs


SCRATCH_BOUND = 256     # bytes per lane: the product's bound on a solver kernel's private segment


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="llvm-readelf not available")
def test_link_kernels_keep_the_budget(M):
    """Every map_score_kernel<SmoothLinkModel<B>, Place> of the built library: one for every MAP kernel of SmoothNoiseModel and none
    for its implicit-differentiation pass, no device-function call (no dynamic stack), scratch within the product bound of 256 B
    per lane, no spilled vector register where the noise twin has none, within the 256 registers of one wave per SIMD lane."""
    rows = {r[0]: r for r in _regs().library_report(M.build_extension())}
    link = {k: r for k, r in rows.items() if "15SmoothLinkModel" in k}
    twins = {k: r for k, r in rows.items() if "16SmoothNoiseModel" in k and k.endswith("Lb0EE")}
    assert not [k for k in link if not k.endswith("Lb0EE")]                  # map kernels only
    assert len(twins) == 16 and len(link) == len(twins)
    for k, r in link.items():
        twin = twins[k.replace("15SmoothLinkModel", "16SmoothNoiseModel")]
        _, vgpr, vspill, sspill, scratch, dyn = r
        print(k, "vgpr", vgpr, "vspill", vspill, "sspill", sspill, "scratch", scratch, "| twin", twin[1:])
        assert not dyn, r
        assert scratch <= SCRATCH_BOUND, r
        assert vspill <= twin[2], (r, twin)
        assert vgpr <= 256, r
