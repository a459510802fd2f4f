"""The implicit-differentiation get_H! (src/muse.jl:335-405) for the TWO-PARAMETER family of user models (include/muse_model.h,
MUSE_MODEL_PAIR_SECOND): the generator's second derivatives, the host evaluation, the C ABI's new entries, and -- on the GPU -- the
kernels against tests/pair_implicit_reference.py, a numpy-longdouble restatement with an exact diagonal solve, within the bound that
module derives from the CG stopping rule and fp64 rounding (its docstring), for three models:

    normal_mean_var (generated from its terms), offset_noise (models/offset_noise.h, hand-written, H1 != 0), cubic_mean_var (generated,
    non-Gaussian: CG needs more than one iteration)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hp_reference as R
import pair_implicit_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET_HEADER = os.path.join(ROOT, "museinference.jl_amd", "models", "offset_noise.h")
needs_ld = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)


def cubic_mean_var(M, directory=None):
    return M.ElementwiseModel.from_pair_expressions("cubic_mean_var", directory=directory, **P.CUBIC_TERMS)


def model_of(M, name):
    if name == "offset_noise":
        return M.ElementwiseModel.packaged("offset_noise")
    if name == "cubic_mean_var":
        return cubic_mean_var(M)
    from test_symbolic_model import generated_nmv
    return generated_nmv(M)


def written_values(name, a, b, x, z, n1, n2):
    """The eight operands as include/muse_model.h and the models' headers write them down."""
    iv, sd = np.exp(-b), np.exp(b / 2)
    if name == "offset_noise":
        r = x - z - a
        return dict(ozz=1 + iv, ozx=-iv, gza=iv, gzb=iv * r, sxa=iv, sxb=iv * r, xa=1.0, xb=0.5 * sd * n2)
    if name == "normal_mean_var":
        return dict(ozz=1 + iv, ozx=-1.0, gza=-iv, gzb=-iv * (z - a), sxa=0.0, sxb=0.0, xa=1.0, xb=0.5 * sd * n1)
    zt = a + sd * n1
    hp, hpt = 1 + 0.3 * z * z, 1 + 0.3 * zt * zt
    return dict(ozz=iv + hp * hp - (x - z - z ** 3 / 10) * 0.6 * z, ozx=-hp, gza=-iv, gzb=-iv * (z - a), sxa=0.0, sxb=0.0, xa=hpt,
                xb=0.5 * hpt * sd * n1)


# ------------------------------------------------------------------------------------------------ CPU
def test_generated_header_states_its_second_derivatives(M, tmp_path):
    for m in (cubic_mean_var(M, str(tmp_path)), model_of(M, "normal_mean_var")):
        text = open(m.header).read()
        code = text.split("*/", 1)[1]
        assert m.pair and "#define MUSE_MODEL_PAIR_SECOND 1" in code
        assert "void muse_model_pair_second(const double* c, double x, double z, double* ozz, double* ozx, double* gza, double* gzb," in code
        assert "void muse_model_pair_dx(const double* c, double n1, double n2, double* xa, double* xb, long i)" in code
        assert "MUSE_MODEL_SECOND" not in code and "muse_model_second" not in code       # (the one-parameter family's names)
        assert text.count("muse_model_exp(") == 2 and " exp(" not in code
        subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                               "-include", "math.h", "-x", "c", m.header])


def test_generator_refuses_a_coefficient_derivative_no_coefficient_holds(M, tmp_path):
    with pytest.raises(ValueError, match=r"d c0 / d a = .* is not a function of the coefficients alone"):
        M.ElementwiseModel.from_pair_expressions("bad", directory=str(tmp_path), coefs=["a**2", "exp(b/2)", "exp(-b)"], C="b",
                                                 o="(x - z)**2 + c2*(z - c0)**2", z="c0 + c1*n1", x="z + n2")
    with pytest.raises(ValueError, match=r"d c1 / d b = .* is not a function of the coefficients alone"):
        M.ElementwiseModel.from_pair_expressions("bad", directory=str(tmp_path), coefs=["a", "exp(b**2)", "exp(-b)"], C="b",
                                                 o="(x - z)**2 + c2*(z - c0)**2", z="c0 + c1*n1", x="z + n2")
    assert os.listdir(str(tmp_path)) == []


def _host_evals(M, lib):
    """model_eval / model_eval_second of HipMuseProblem with a NULL context (a model without run-time constants: no GPU)."""
    def ev(a, b, x, z, n1, n2, i=0):
        out = np.empty(12)
        M._capi.check(lib.muse_model_eval(None, float(a), float(b), float(x), float(z), float(n1), float(n2), int(i), M._capi.ptr(out)), lib)
        return dict(zip(("grad", "term", "t0", "c0", "c1", "c2", "c3", "z", "x", "C", "t1"), out.tolist()))

    def ev2(a, b, x, z, n1, n2, i=0):
        out = np.empty(8)
        M._capi.check(lib.muse_model_eval_pair_second(None, float(a), float(b), float(x), float(z), float(n1), float(n2), int(i),
                                                      M._capi.ptr(out)), lib)
        return dict(zip(("ozz", "ozx", "gza", "gzb", "sxa", "sxb", "xa", "xb"), out.tolist()))
    return ev, ev2


@pytest.mark.parametrize("name", P.MODELS)
def test_library_has_second_derivatives_and_evaluates_them_on_the_host(M, name):
    """The library of a header with MUSE_MODEL_PAIR_SECOND loads without a GPU, says muse_model_has_second() = 1, and
    muse_model_eval_pair_second (NULL context) gives the written-down values and the central differences of the header's own
    first-order functions (muse_model_eval)."""
    from museinference_jl_amd.models import _check_pair_second
    lib = M._capi.load_library(model_of(M, name).library())
    assert lib.muse_model_has_second() == 1
    ev, ev2 = _host_evals(M, lib)
    rs = np.random.RandomState(3)
    for _ in range(5):
        a, b, x, z, n1, n2 = rs.randn(6) * [0.5, 0.5, 1.5, 1.0, 1.0, 1.0]
        got, want = ev2(a, b, x, z, n1, n2, 4), written_values(name, a, b, x, z, n1, n2)
        for key in want:
            np.testing.assert_allclose(got[key], want[key], rtol=1e-13, atol=1e-14, err_msg=key)
    theta = np.array([0.3, -0.2, -0.4, 0.5])
    xs, zs = rs.randn(40) * 1.5, rs.randn(40)
    assert _check_pair_second(ev, ev2, theta, xs, zs, 6, 2e-5) <= 2e-5
    # the pad element: zero coefficients cannot be asked for through (a, b); i >= N can
    assert all(np.isfinite(v) for v in ev2(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 10 ** 6).values())


def test_libraries_without_pair_second_say_so(M):
    lib = M._capi.load_library(M.ElementwiseModel.packaged("normal_mean_var").library())
    assert lib.muse_model_has_second() == 0
    out = np.empty(8)
    assert lib.muse_model_eval_pair_second(None, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0, M._capi.ptr(out)) != 0
    assert M.load_library().muse_model_eval_pair_second(None, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0, M._capi.ptr(out)) != 0


def test_unchanged_checker_builds_the_headers(M, O):
    """The CPU checker compiles every user header; its MUSE_MODEL_SECOND branch is the one-parameter family's.  A header with
    MUSE_MODEL_PAIR_SECOND must still build there, and its draw and score match the closed forms."""
    from test_pair_model import blocks
    N, theta = 1001, np.array([0.7, -0.3, 0.4, -0.6])
    K, k = 2, blocks(1001, 2)
    a, sd, iv = theta[k], np.exp(theta[K + k] / 2), np.exp(-theta[K + k])
    n1, n2 = O.normals(5, 3, N)
    with O.user_model(OFFSET_HEADER, "offset_noise"):
        x, z = O.sample_x_z("user", N, 5, 3, theta)
        assert np.array_equal(z, n1)
        np.testing.assert_allclose(x, n1 + a + sd * n2, rtol=1e-14, atol=1e-15)
        zz = 0.7 * z + 0.1
        r = x - zz - a
        want = [np.sum((iv * r)[k == b]) for b in range(K)] + [0.5 * (np.sum((iv * r * r)[k == b]) - np.sum(k == b)) for b in range(K)]
        np.testing.assert_allclose(O.grad_theta("user", x, zz, theta), want, rtol=1e-12, atol=1e-12)
        f, g = O.logLike_and_grad_z("user", x, zz, theta)
        np.testing.assert_allclose(g, -(zz - iv * r), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(f, -0.5 * (np.sum(zz * zz + iv * r * r) + np.sum(theta[K + k])), rtol=1e-13)
    m = cubic_mean_var(M)
    with O.user_model(m.header, m.library_name):
        x, z = O.sample_x_z("user", N, 5, 3, theta)
        np.testing.assert_allclose(z, a + sd * n1, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(x, z + z ** 3 / 10 + n2, rtol=1e-14, atol=1e-15)
        zz = 0.7 * z + 0.1
        d = zz - a
        want = [np.sum((iv * d)[k == b]) for b in range(K)] + [0.5 * (np.sum((iv * d * d)[k == b]) - np.sum(k == b)) for b in range(K)]
        np.testing.assert_allclose(O.grad_theta("user", x, zz, theta), want, rtol=1e-12, atol=1e-12)


@needs_ld
@pytest.mark.parametrize("name", ["normal_mean_var", "offset_noise"])
def test_reference_mean_H_is_the_exact_information(name):
    """The reference itself: E[H] over 2000 streams against the Fisher information of x_i ~ N(mu, 1 + e^tau), to 5 standard errors
    of the per-simulation values (plus the rounding of a mean whose values do not vary at all: H_mu,mu of normal_mean_var)."""
    n, theta = 48, [0.3, -0.4]
    Hs = np.array([P.implicit_H(name, n, 5, s, theta)["H"] for s in range(2000)])
    want = P.exact_information(n, theta[1])
    se = Hs.std(axis=0, ddof=1) / np.sqrt(len(Hs))
    assert np.all(np.abs(Hs.mean(axis=0) - want) <= 5 * se + 1e-12 * np.abs(want).max()), (Hs.mean(axis=0), want, se)
    if name == "offset_noise":
        assert np.abs(np.array([P.implicit_H(name, n, 5, s, theta)["H1"] for s in range(3)])).min() > 0.0


def test_exports_header_and_ctypes_table_agree_on_the_new_entries(M):
    from museinference_jl_amd.build import declared_symbols
    new = {"muse_implicit_H_batch_ex", "muse_implicit_H_columns_ex", "muse_model_eval_pair_second"}
    assert new <= set(declared_symbols())
    text = open(os.path.join(ROOT, "museinference.jl_amd", "_capi.py")).read()
    for n in new:
        assert f'"{n}"' in text
    for lib in (M.load_library(), M._capi.load_library(M.ElementwiseModel.packaged("offset_noise").library())):   # raises on a missing symbol
        for n in new:
            assert getattr(lib, n).restype is ctypes.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", M._capi.library_path()], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("muse_")}
    assert exported == set(declared_symbols())


def test_cg_keywords_of_get_H(M):
    """implicit_diff_cg_kwargs: maxiter, reltol, abstol are applied, Pl only as the identity, anything else is refused -- before the
    problem is touched."""
    from museinference_jl_amd.muse import _cg_keywords
    assert _cg_keywords(None) == {"cg_maxiter": 100}
    assert _cg_keywords(dict(maxiter=7, reltol=1e-3, abstol=1e-9, Pl=None)) == {"cg_maxiter": 7, "cg_reltol": 1e-3, "cg_abstol": 1e-9}
    assert _cg_keywords(dict(Pl=np.eye(3))) == {"cg_maxiter": 100}
    for bad in (np.ones((2, 2)), 2 * np.eye(2), "jacobi", lambda v: v):
        with pytest.raises(ValueError, match="Pl must be the identity"):
            M.get_H_(None, None, implicit_diff=True, implicit_diff_cg_kwargs={"Pl": bad})
    with pytest.raises(ValueError, match=r"unsupported key\(s\) \['verbose'\]"):
        M.get_H_(None, None, implicit_diff=True, implicit_diff_cg_kwargs={"maxiter": 5, "verbose": True})


# ------------------------------------------------------------------------------------------------ GPU
THETAS = {2: [0.3, -0.4], 4: [0.2, -0.1, 0.4, -0.3], 8: [0.2, -0.1, 0.3, 0.0, 0.4, -0.3, 0.1, -0.5]}
THETAS_CUBIC = {2: [0.3, -1.2], 4: [0.2, -0.1, -1.0, -1.3], 8: [0.2, -0.1, 0.3, 0.0, -1.0, -1.3, -0.9, -1.4]}   # small e^b: ozz > 0 at every MAP
CASES = [(300, 2), (7001, 4), (10000, 8), (70001, 4)]     # the first three: streaming, one workgroup; the last: clusters


def theta_of(name, nth):
    return np.array((THETAS_CUBIC if name == "cubic_mean_var" else THETAS)[nth])


def within(got, want, bound, what):
    err = np.abs(got - want)
    print(what, "max |err| / bound =", float(np.max(err / np.maximum(bound, 1e-300))), "max |err| =", float(err.max()))
    assert np.all(err <= 2.0 * bound), (what, err, 2.0 * bound)


@needs_ld
@pytest.mark.gpu
@pytest.mark.parametrize("N,nth", CASES)
@pytest.mark.parametrize("name", P.MODELS)
def test_implicit_H_against_the_reference(gpu, M, name, N, nth):
    """Three simulations per case, every entry: |H - H*| <= 2 (|gzp| reltol |b_q| / min ozz + rounding) with the MAP solved to 1e-10 and
    CG at its defaults; one CG iteration for the Gaussian models (b is an eigenvector of the diagonal Hessian's block), at least two for
    the cubic one.  Odd N: the pad element."""
    theta = theta_of(name, nth)
    prob = M.HipMuseProblem(None, model=model_of(M, name), ntheta=nth, N=N)
    assert prob.has_second_derivatives
    info = prob.placement_info()
    assert (info["workgroups_per_element"] > 1) == (N == 70001)
    Hs, its = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10)
    for s in range(3):
        ref = P.implicit_H(name, N, 17, s, theta)
        within(Hs[s], ref["H"], ref["bound"](), f"{name} N={N} nth={nth} sim {s}")
    assert np.all(its >= 2) if name == "cubic_mean_var" else np.all(its == 1), its
    # the legacy entry is the _ex entry with the default arguments: the same bits
    Hl = np.empty_like(Hs)
    il = np.zeros_like(its)
    th = M._capi.f8(theta, nth)
    prob._check(prob._lib.muse_implicit_H_batch(prob._ctx, 17, 0, 3, M._capi.ptr(th), 1e-10, 100, M._capi.ptr(Hl), M._capi.ptr(il)))
    assert Hl.tobytes() == Hs.tobytes() and np.array_equal(il, its)
    # H1 is zero: the reference's H2 alone; for offset_noise that is not H
    H2, _ = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10, H1_is_zero=True)
    for s in range(3):
        ref = P.implicit_H(name, N, 17, s, theta)
        within(H2[s], ref["H2"], ref["bound_H2"](), f"{name} N={N} H2 sim {s}")
        if name == "offset_noise":
            assert np.abs(H2[s] - Hs[s]).max() > 1.0
    # no CG iteration: H = H1
    H1, i0 = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10, cg_maxiter=0)
    assert np.all(i0 == 0)
    for s in range(3):
        ref = P.implicit_H(name, N, 17, s, theta)
        within(H1[s], ref["H1"], ref["bound_H1"], f"{name} N={N} H1 sim {s}")
    prob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,nth", [(300, 2), (7001, 4), (70001, 4)])
@pytest.mark.parametrize("name", ["offset_noise", "cubic_mean_var"])
def test_columns_equal_the_batch_in_both_split_regimes(gpu, M, name, N, nth):
    """muse_implicit_H_columns over the full column range is the batch bit for bit -- with one column per element (few simulations:
    the batch spreads the columns over the GPU) and with all columns in one element (many simulations) -- CG counts included."""
    theta = theta_of(name, nth)
    prob = M.HipMuseProblem(None, model=model_of(M, name), ntheta=nth, N=N)
    many = 600 if N < 20000 else 80          # more simulations than half the launch's slots: one element per simulation
    few, _ = prob.implicit_H_batch(11, 2, 5, theta)
    big, ib = prob.implicit_H_batch(11, 0, many, theta)
    cols, ic = prob.implicit_H_columns(11, 0, 0, many * nth, theta)
    assert np.array_equal(cols.reshape(many, nth, nth).transpose(0, 2, 1), big) and np.array_equal(ic.reshape(many, nth), ib)
    assert few.tobytes() == big[2:5].tobytes()
    part, _ = prob.implicit_H_columns(11, 0, 3, 3 * nth + 2, theta)      # a range that begins and ends inside a simulation
    assert np.array_equal(part, cols[3:3 * nth + 2])
    prob.close()


@needs_ld
@pytest.mark.gpu
def test_a_loose_cg_tolerance_on_the_cubic_model(gpu, M):
    """cg_reltol = 1e-3: no more iterations than the default, fewer somewhere, and the result within the same bound formula at that
    tolerance; cg_abstol above every |b| stops CG at once (H = H1 = 0 for this model)."""
    N, nth = 7001, 4
    theta = theta_of("cubic_mean_var", nth)
    prob = M.HipMuseProblem(None, model=model_of(M, "cubic_mean_var"), ntheta=nth, N=N)
    Hd, itd = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10)
    Hl, itl = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10, cg_reltol=1e-3)
    print("CG iterations: default", itd.tolist(), "reltol 1e-3", itl.tolist())
    assert np.all(itl <= itd) and np.all(itl >= 1)
    for s in range(3):
        ref = P.implicit_H("cubic_mean_var", N, 17, s, theta)
        within(Hl[s], ref["H"], ref["bound"](1e-3), f"reltol 1e-3 sim {s}")
    H0, it0 = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10, cg_abstol=1e9)
    assert np.all(it0 == 0) and np.all(H0 == 0.0)
    for bad in (dict(cg_reltol=-1.0), dict(cg_abstol=float("nan")), dict(cg_maxiter=-1)):
        with pytest.raises(M.MuseError):
            prob.implicit_H_batch(17, 0, 1, theta, **bad)
    prob.close()


@pytest.mark.gpu
def test_other_models_refuse_what_their_kernels_do_not_honour(gpu, M):
    """The implicit kernels of the built-in models run CG's defaults and always form H1: the _ex entries refuse anything else
    instead of ignoring it, and give the legacy entry's bits at the defaults."""
    prob = M.HipMuseProblem(None, model="funnel", ntheta=2, N=1000)
    H, its = prob.implicit_H_batch(5, 0, 2, [0.1, 0.2])
    Hl, il = np.empty_like(H), np.zeros_like(its)
    th = M._capi.f8([0.1, 0.2], 2)
    prob._check(prob._lib.muse_implicit_H_batch(prob._ctx, 5, 0, 2, M._capi.ptr(th), 1e-1, 100, M._capi.ptr(Hl), M._capi.ptr(il)))
    assert Hl.tobytes() == H.tobytes() and np.array_equal(il, its)
    for kw in (dict(H1_is_zero=True), dict(cg_reltol=1e-3), dict(cg_abstol=1e-9), dict(cg_maxiter=0)):
        with pytest.raises(M.MuseError, match="two-parameter family|cg_maxiter"):
            prob.implicit_H_batch(5, 0, 2, [0.1, 0.2], **kw)
    prob.close()


@pytest.mark.gpu
def test_check_model_consistency_covers_the_pair_second_derivatives(gpu, M):
    for name in ("offset_noise", "cubic_mean_var"):
        prob = M.HipMuseProblem(None, model=model_of(M, name), ntheta=4, N=2001)
        res = M.check_model_consistency(prob, theta_of(name, 4), rng=4)
        assert res["second"] <= 2e-5 and max(res["grad_z"], res["grad_theta"]) <= 2e-5 + res["noise_floor"], res
        prob.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K,truth,nsims", [(1, [0.8, 0.5], 512), (2, [0.8, -0.6, 0.5, 1.0], 256)])
def test_muse_on_offset_noise_against_the_exact_posterior(gpu, M, K, truth, nsims):
    """muse() on models/offset_noise.h at N = 10^4, then get_J! and get_H! by implicit differentiation with as many simulations as the
    loop used: the reported sigma against the exact marginal posterior (x_i ~ N(mu_k, 1 + e^tau_k): tests/test_pair_model.py's
    exact_posterior and its bound); the finite-difference get_H! on the same run under the same bound; H1-is-zero, applied through
    get_H_, gives another H."""
    from test_pair_model import PRIOR_SIGMA, exact_posterior
    N = 10000
    model = M.ElementwiseModel.packaged("offset_noise")
    tmp = M.HipMuseProblem(None, model=model, ntheta=2 * K, N=N)
    x, _ = tmp.sample_x_z(M.SimRng(99, M.DATA_SIM), truth)
    tmp.close()
    mode, sigma = exact_posterior(x, K)
    prob = M.HipMuseProblem(x, model=model, ntheta=2 * K, prior=M.GaussianPrior(0.0, PRIOR_SIGMA))
    res = M.muse(prob, [0.0] * (2 * K), rng=20240, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-6, alpha=1.0,
                 get_covariance=False)
    dev = np.abs(np.asarray(res.theta) - mode) / (sigma / np.sqrt(nsims))
    assert np.all(dev < 4.0), (res.theta, mode, dev)
    M.get_J_(res, prob, nsims=nsims)
    tol = 5.0 * 0.5 * np.sqrt(2.0 / (nsims - 1)) + 0.03
    got = {}
    for how, kw in (("implicit", dict(implicit_diff=True)), ("finite differences", {}),
                    ("implicit, H1 = 0", dict(implicit_diff=True, implicit_diff_H1_is_zero=True, implicit_diff_cg_kwargs=dict(maxiter=50, Pl=None)))):
        res.Hs, res.H = [], None
        M.get_H_(res, prob, nsims=nsims, **kw)
        got[how] = (np.sqrt(np.diag(np.atleast_2d(res.Sigma))), np.array(res.H))
        print(how, "sigma / exact", got[how][0] / sigma)
    for how in ("implicit", "finite differences"):
        assert np.all(np.abs(got[how][0] / sigma - 1.0) < tol), (how, got[how][0], sigma)
    assert np.abs(got["implicit, H1 = 0"][1] - got["implicit"][1]).max() > 1.0
    prob.close()
