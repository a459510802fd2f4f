"""User-supplied elementwise models (include/muse_model.h): SimpleMuseProblem's closures (src/simple.jl:79-95) as a C header
compiled into an engine library of its own (museinference_jl_amd.ElementwiseModel) -- and, for the tests, into a build of the
CPU oracle that compiles the SAME text (oracle.user_model).  The example is museinference.jl_amd/models/cubic.h: a funnel
seen through x = z + z^3/10 + n (non-Gaussian posterior, non-quadratic MAP objective).

not gpu: the model's own consistency on the oracle (gradient and score against finite differences of logLike, the family
identity, the MAP against scipy), the library's exports and refusals.
gpu: the HIP path against the oracle in every placement of the solver kernel (sampler bit-exact; identical iteration and
evaluation counts; MAPs to 1e-9 and scores to 1e-10 for solves of up to 20 iterations -- on longer ones, 50-60 iterations of
a non-quadratic objective at N = 10^4, the tree-ordered and the sequential sums drift apart along the SAME path, and the
stated agreement is a thousandth of the solver's own tolerance: MAPs to 1e-3 atol, scores to 1e-6), the batched finite-difference H, whole muse() runs against the independent restatement, a model written from source,
and the built-in funnel re-expressed as a user model (bit-identical to the built-in one)."""
import ctypes
import os

import numpy as np
import pytest

from test_gpu_parity import assert_same_path_or_close, hess_inf_cubic

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CUBIC = os.path.join(ROOT, "museinference.jl_amd", "models", "cubic.h")


def h(z):
    return z + 0.1 * z ** 3


def cubic_logLike(x, z, theta, N):
    """-1/2 sum [(x - h(z))^2 + e^-theta_k z^2] - 1/2 sum n_k theta_k in numpy (blocks as the engine's)."""
    nth = len(theta)
    k = (np.arange(N) * nth) // N
    th = np.asarray(theta, dtype=np.float64)[k]
    return -0.5 * np.sum((x - h(z)) ** 2 + np.exp(-th) * z ** 2) - 0.5 * np.sum(th)


# ------------------------------------------------------------------------------------------------ CPU
def test_cubic_model_on_the_oracle_is_what_its_header_says(O):
    theta = [0.4, -0.3, 0.9]
    N = 301
    with O.user_model(CUBIC, "cubic"):
        assert O.lib().mo_user_model_name() == b"cubic"
        x, z = O.sample_x_z("user", N, 17, 3, theta)
        n1, n2 = O.normals(17, 3, N)
        k = (np.arange(N) * 3) // N
        np.testing.assert_allclose(z, np.array([O.exp_fixed(0.5 * t) for t in theta])[k] * n1, rtol=1e-15)
        np.testing.assert_allclose(x, h(z) + n2, rtol=1e-14, atol=1e-15)
        zz = 0.6 * z + 0.05
        f, g = O.logLike_and_grad_z("user", x, zz, theta)
        np.testing.assert_allclose(f, cubic_logLike(x, zz, theta, N), rtol=1e-13)
        # grad_z logLike against the closed form and against central differences of the value
        np.testing.assert_allclose(g, (x - h(zz)) * (1 + 0.3 * zz ** 2) - np.exp(-np.asarray(theta))[k] * zz, rtol=1e-12, atol=1e-13)
        for i in (0, 150, 300):
            e = np.zeros(N)
            e[i] = 1e-5
            fd = (cubic_logLike(x, zz + e, theta, N) - cubic_logLike(x, zz - e, theta, N)) / 2e-5
            np.testing.assert_allclose(g[i], fd, rtol=1e-6, atol=1e-8)
        # the family identity: the score assembled from B = z^2 is d logLike / d theta
        s = O.grad_theta("user", x, zz, theta)
        for j in range(3):
            tp, tm = np.array(theta), np.array(theta)
            tp[j] += 1e-5
            tm[j] -= 1e-5
            fd = (O.logLike_and_grad_z("user", x, zz, tp)[0] - O.logLike_and_grad_z("user", x, zz, tm)[0]) / 2e-5
            np.testing.assert_allclose(s[j], fd, rtol=1e-7)
        # the MAP: stationary, and the minimiser scipy finds
        zh, info = O.zhat_at_theta("user", x, np.zeros(N), theta, 1e-8)
        assert info["status"] == 0 and info["gnorm"] <= 1e-8 and info["iterations"] > 3
        from scipy.optimize import minimize
        r = minimize(lambda v: -cubic_logLike(x, v, theta, N), np.zeros(N), method="L-BFGS-B",
                     jac=lambda v: -((x - h(v)) * (1 + 0.3 * v ** 2) - np.exp(-np.asarray(theta))[k] * v), options={"gtol": 1e-10, "ftol": 1e-15})
        np.testing.assert_allclose(zh, r.x, atol=2e-6)
    assert O.lib().mo_user_model_name() is None   # back in the plain oracle


def test_gaussian_funnel_header_equals_the_built_in_funnel_on_the_oracle(O):
    """models/gaussian_funnel.h (the built-in funnel written as a user's header) in the oracle's user-model build: the same bits
    as the oracle's own funnel -- draw, logLike, gradient, MAP, solver record, score (the GPU twin of this test compares
    the two engine libraries)."""
    hdr = os.path.join(ROOT, "museinference.jl_amd", "models", "gaussian_funnel.h")
    N, theta = 1500, [0.7, -0.4, 1.2]
    ref = {}
    for tag in ("funnel", "user"):
        ctx = O.user_model(hdr, "gaussian_funnel")
        with ctx:   # (the user build holds the built-in models too: both run in the same library)
            x, z = O.sample_x_z(tag, N, 3, 9, theta)
            f, g = O.logLike_and_grad_z(tag, x, 0.5 * z, theta)
            zh, info = O.zhat_at_theta(tag, x, np.zeros(N), theta, 1e-8)
            ref[tag] = (x, z, f, g, zh, tuple(info[k] for k in ("iterations", "f_calls", "status", "f_min", "gnorm")), O.grad_theta(tag, x, zh, theta))
    for a, b in zip(ref["funnel"], ref["user"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_examples_and_packaged_headers_are_well_formed():
    """examples/*.py compile; every packaged model header is plain C (gcc -fsyntax-only with the contract's macro)."""
    import glob
    import py_compile
    import subprocess
    for f in glob.glob(os.path.join(ROOT, "examples", "*.py")):
        py_compile.compile(f, doraise=True)
    headers = glob.glob(os.path.join(ROOT, "museinference.jl_amd", "models", "*.h")) + glob.glob(os.path.join(HERE, "models", "*.h"))
    assert len(headers) >= 4
    for h_ in headers:
        subprocess.check_call(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                               "-include", "math.h", "-x", "c", h_])


def test_check_model_consistency_on_the_oracle(M, O):
    """check_model_consistency (what AD guarantees in the reference has to be checked for a hand-written header) through an
    oracle-backed problem on CPU: the shipped example passes, a header whose score term is not its objective's B fails."""
    from oracle_problem import OracleMuseProblem
    with O.user_model(CUBIC, "cubic"):
        res = M.check_model_consistency(OracleMuseProblem(None, model="user", ntheta=3, N=2001), [0.4, -0.3, 0.9], rng=5)
        assert res["grad_z"] <= 2e-5 + res["noise_floor"] and res["grad_theta"] <= 2e-5 + res["noise_floor"] and res["noise_floor"] < 1e-4
    with O.user_model(os.path.join(HERE, "models", "wrong_score.h"), "wrong_score"):
        with pytest.raises(AssertionError) as e:
            M.check_model_consistency(OracleMuseProblem(None, model="user", ntheta=2, N=500), [0.4, -0.3])
        assert "grad_theta" in str(e.value)
    res = M.check_model_consistency(OracleMuseProblem(None, model="smooth", ntheta=2, N=300), [1.0, 2.0])   # any problem
    assert max(res["grad_z"], res["grad_theta"]) <= 2e-5 + res["noise_floor"]


def test_model_library_exports_and_refusals(M):
    """The model's engine library is the same C ABI (every symbol of include/muse_hip.h) holding MUSE_MODEL_USER only;
    libmuse_hip.so refuses MUSE_MODEL_USER; neither has a CPU path."""
    from test_capi_exports import declared_symbols
    model = M.ElementwiseModel.packaged("cubic")
    lib = M._capi.load_library(model.library())
    raw = ctypes.CDLL(model.library())
    for n in declared_symbols():
        assert hasattr(raw, n), n
    assert lib.muse_model_name(3) == b"cubic" and lib.muse_model_name(0) is None
    main = M.load_library()
    assert main.muse_model_name(0) == b"funnel" and main.muse_model_name(2) == b"smooth" and main.muse_model_name(3) is None
    ctx = ctypes.c_void_p()
    assert main.muse_ctx_create(3, 100, 1, 0, ctypes.byref(ctx)) == -1 and b"built-in models only" in main.muse_last_error()
    assert lib.muse_ctx_create(0, 100, 1, 0, ctypes.byref(ctx)) == -1 and b"MUSE_MODEL_USER only" in lib.muse_last_error()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(M.MuseError) as e:
            M.HipMuseProblem(None, model=model, N=16)
        assert "no HIP device" in str(e.value)
    with pytest.raises(ValueError):
        M.ElementwiseModel("bad name", CUBIC)
    with pytest.raises(ValueError):
        M.HipMuseProblem(None, model="cubic", N=16)   # a name is not a model: pass the ElementwiseModel


# ------------------------------------------------------------------------------------------------ GPU
PLACEMENTS = [  # (N, ntheta, theta, placement, split) -> every instantiation of the solver kernel a user model gets
    (37, 1, [0.3], -1, 0),                 # PlaceResident<256,1>
    (300, 3, [0.4, -0.3, 0.9], -1, 0),
    (2000, 1, [1.0], -1, 0),               # PlaceResident<512,4>
    (2000, 2, [0.5, -0.5], -1, 4),         # register clusters of 4 workgroups
    (10000, 1, [1.0], -1, 0),              # PlaceResident<512,10> (x, g in LDS)
    (10000, 4, [0.2, -0.3, -1.0, 0.0], -1, 0),
    (10000, 2, [1.0, 1.5], -1, 0),         # strongly non-linear: 100-130 iterations per solve
    (10000, 1, [0.2], -1, 2),
    (9001, 2, [0.0, 0.7], -1, 8),
    (7001, 1, [-0.4], 0, 0),               # streaming, one workgroup
    (300, 2, [0.1, 0.2], 0, 0),            # PlaceStreaming<256>
    (30011, 8, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], -1, 0),
    (70001, 2, [0.3, -0.2], -1, 0),        # N >= 65536: streaming clusters
]


def make(M, x, N, nth, placement, split, model=None, prior=None):
    prob = M.HipMuseProblem(x, model=model or M.ElementwiseModel.packaged("cubic"), ntheta=nth, N=None if x is not None else N, prior=prior)
    if placement >= 0:
        prob.set_placement(placement)
    if split:
        prob.set_element_split(split)
    return prob


@pytest.mark.gpu
@pytest.mark.parametrize("N,nth,theta,placement,split", PLACEMENTS)
def test_cubic_model_hip_against_oracle(gpu, M, O, N, nth, theta, placement, split):
    with O.user_model(CUBIC, "cubic"):
        xdata, _ = O.sample_x_z("user", N, 77, M.DATA_SIM, np.zeros(nth))
        prob = make(M, xdata, N, nth, placement, split)
        # per-sim operators: the draw bit for bit, logLike / grad / score to rounding
        for sim in (0, 2**40 + 7):
            x, z = prob.sample_x_z(M.SimRng(1234, sim), theta)
            xo, zo = O.sample_x_z("user", N, 1234, sim, theta)
            assert np.array_equal(z, zo) and np.array_equal(x, xo)
        zz = 0.7 * zo + 0.1
        f, g = prob.logLike_and_grad_z_logLike(xo, zz, theta)
        fo, go = O.logLike_and_grad_z("user", xo, zz, theta)
        np.testing.assert_allclose(f, fo, rtol=1e-12)
        np.testing.assert_allclose(g, go, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(prob.grad_theta_logLike(xo, zz, theta), O.grad_theta("user", xo, zz, theta), rtol=1e-12)
        # the map of muse!: data + sims, from zero, from the simulation's z, warm
        nsims = 5 if N > 20000 else 13
        for z0_mode in (0, 1):
            g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4, z0_mode=z0_mode)
            go, zo, io = O.map_and_score_batch("user", N, 42, 3, 3 + nsims, theta, atol=1e-4, x_data=xdata, z0_mode=z0_mode)
            zh = prob.get_zhat(0, nsims + 1)
            long = int(io["iterations"].max()) > 20
            same = assert_same_path_or_close(info, io, zh, zo, g, go, 1e-4, theta, "funnel", ctx=f"z0_mode {z0_mode}",
                                             hess_inf=hess_inf_cubic(theta, zo, 1e-4),
                                             z_atol=1e-7 if long else 1e-9, g_rtol=1e-6 if long else 1e-10)
            # (a solve of 100+ iterations may leave the oracle's path -- the helper then bounds it by what the tolerance implies)
            assert same.all() if not long else same.mean() >= 0.8, (info["iterations"], io["iterations"], info["f_calls"], io["f_calls"])
            assert info["iterations"].min() >= 2   # not a one-step problem: the line search and the history are exercised
            print(N, nth, placement, split, "z0_mode", z0_mode, "iterations", io["iterations"].min(), io["iterations"].max())
        th2 = np.asarray(theta) + 0.05
        g2, info2 = prob.map_and_score_batch(42, 3, 3 + nsims, th2, include_data=True, atol=1e-4, z0_mode=M.Z0_WARM)
        go2, zo2, io2 = O.map_and_score_batch("user", N, 42, 3, 3 + nsims, th2, atol=1e-4, x_data=xdata, z0_mode=2, zhat=zo.copy())
        if same.all():   # the warm restart starts from the first map's MAPs: comparable where those were the same
            assert np.array_equal(info2["f_calls"], io2["f_calls"]) or long
            np.testing.assert_allclose(g2, go2, rtol=1e-6 if long else 1e-10)
        prob.close()


@pytest.mark.gpu
def test_cubic_model_fd_jacobian_multi_map_and_refusal(gpu, M, O):
    N, nth, theta = 3000, 2, np.array([0.4, -0.2])
    step = np.array([0.05, 0.04])
    with O.user_model(CUBIC, "cubic"):
        prob = make(M, None, N, nth, -1, 0)
        Hs, info = prob.fd_jacobian_batch(9, 0, 5, theta, step, atol=1e-4)
        _, zfid, _ = O.map_and_score_batch("user", N, 9, M.MASTER_SIM, M.MASTER_SIM + 1, theta, atol=1e-4, z0_mode=0)
        for s in range(5):
            np.testing.assert_allclose(Hs[s], O.fd_jacobian("user", N, 9, s, theta, step, zfid[0], atol=1e-4), rtol=1e-8, atol=1e-9)
        # several maps (several thetas) in ONE launch = the same maps one by one
        thetas = np.array([[0.4, -0.2], [0.0, 0.3], [1.0, 1.0]])
        tot = prob.map_and_score_multi_async(5, 0, 20, thetas, atol=1e-4, z0_mode=0, result_area=1)
        gm, im = prob.batch_wait(tot, 1)
        for m, th in enumerate(thetas):
            g1, i1 = prob.map_and_score_batch(5, 0, 20, th, atol=1e-4, z0_mode=0)
            assert np.array_equal(gm[20 * m:20 * (m + 1)], g1) and np.array_equal(im[20 * m:20 * (m + 1)], i1)
        prob.close()


@pytest.mark.gpu
def test_cubic_model_whole_muse_run(gpu, M, O):
    """muse() + get_J! + get_H! (finite differences) on the user's model: the native loop and the Python loop against the
    independent restatement (tests/muse_reference.py) on the oracle's map, and the reference's own statistical criterion
    (test/runtests.jl:31: the estimate within a few sigma of the truth)."""
    import muse_reference as R
    from golden.make_golden import OracleMap, covariance, gaussian_prior
    N, nth, nsims, truth = 6000, 2, 48, np.array([0.5, -0.5])
    with O.user_model(CUBIC, "cubic"):
        x, _ = O.sample_x_z("user", N, 2024, M.DATA_SIM, truth)
        pg, ph = gaussian_prior(3.0)
        hist, theta_o, gs_o = R.muse_loop(OracleMap("user", x, nth, 11, nsims, atol=1e-4), [0.0, 0.0], nsims=nsims, prior_grad_t=pg,
                                          prior_hess_t=ph, maxsteps=8, theta_rtol=1e-2, alpha=0.7)
        J_o, Hs_o, H_o, _ = covariance("user", x, nth, 11, theta_o, gs_o, max(1, nsims // 10), atol=1e-4)
    prob = make(M, x, N, nth, -1, 0, prior=M.GaussianPrior(0.0, 3.0))
    for native in (True, False):
        res = M.muse(prob, [0.0, 0.0], rng=11, nsims=nsims, maxsteps=8, theta_rtol=1e-2, grad_z_logLike_atol=1e-4, alpha=0.7,
                     get_covariance=True, native=native)
        np.testing.assert_allclose(np.array([hh["θ"] for hh in res.history]), np.array([hh["θ"] for hh in hist]), rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(res.theta, theta_o, rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(res.J, J_o, rtol=1e-8)
        np.testing.assert_allclose(res.H, H_o, rtol=1e-6, atol=1e-9 * np.abs(H_o).max())
    sigma = np.sqrt(np.diag(res.Sigma))
    assert np.all(np.abs(res.theta - truth) / sigma < 4.0), (res.theta, sigma)
    assert np.all(sigma < 0.1)
    prob.close()


@pytest.mark.gpu
def test_check_model_consistency_on_hip(gpu, M):
    for N, nth, theta in [(10000, 2, [0.5, -0.5]), (70000, 1, [0.2])]:
        prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("cubic"), ntheta=nth, N=N)
        res = M.check_model_consistency(prob, theta, rng=3)
        assert max(res["grad_z"], res["grad_theta"]) <= 2e-5 + res["noise_floor"], res
        assert prob.has_second_derivatives and res["second"] <= 2e-5, res    # (cubic.h defines MUSE_MODEL_SECOND)
        prob.close()


@pytest.mark.gpu
def test_funnel_as_user_model_equals_the_built_in_funnel(gpu, M):
    """The built-in funnel written as a user's header (museinference.jl_amd/models/gaussian_funnel.h: the same arithmetic) gives the same
    BITS as MUSE_MODEL_FUNNEL -- scores, MAPs, solver infos -- in the resident, streaming and cluster placements: the
    user-model seam adds nothing to the kernel."""
    model = M.ElementwiseModel.packaged("gaussian_funnel")
    for N, nth, theta, placement in [(10000, 1, [1.0], -1), (10000, 3, [1.0, 0.0, -1.0], -1), (5000, 2, [0.3, 0.6], 0), (70000, 1, [0.5], -1)]:
        a = M.HipMuseProblem(None, model="funnel", ntheta=nth, N=N)
        b = M.HipMuseProblem(None, model=model, ntheta=nth, N=N)
        for p in (a, b):
            if placement >= 0:
                p.set_placement(placement)
        n = 40 if N <= 10000 else 6
        ga, ia = a.map_and_score_batch(3, 0, n, theta, atol=1e-6, z0_mode=0)
        gb, ib = b.map_and_score_batch(3, 0, n, theta, atol=1e-6, z0_mode=0)
        assert np.array_equal(ga, gb) and ia.tobytes() == ib.tobytes()
        assert np.array_equal(a.get_zhat(0, n), b.get_zhat(0, n))
        a.close()
        b.close()


NOISE_SECOND_SOURCE = '''
#include "muse_model.h"
#define MUSE_MODEL_NAME "noise_second"
#define MUSE_MODEL_SECOND 1
/* the built-in noise model (z ~ N(0,1), x ~ N(z, e^theta): A = z^2, B = (x - z)^2) with its second derivatives -- the member
   of the family whose B depends on x, i.e. whose implicit-differentiation H has an H1 term */
MUSE_MODEL_FN void muse_model_sample(double sd, double n1, double n2, double* z, double* x, long i) { (void)i; *z = n1; *x = n1 + sd * n2; }
MUSE_MODEL_FN double muse_model_grad(double iv, double x, double z, double* acc, long i) {
    (void)i;
    const double r = x - z, t = iv * r;
    *acc = fma(z, z, fma(t, r, *acc));
    return z - t;
}
MUSE_MODEL_FN double muse_model_score_term(double x, double z, long i) { (void)i; const double r = x - z; return r * r; }
MUSE_MODEL_FN void muse_model_second(double iv, double x, double z, double* ozz, double* ozx, double* bz, double* bx, long i) {
    (void)i;
    *ozz = iv + 1.0;
    *ozx = -iv;
    *bz = -2.0 * (x - z);
    *bx = 2.0 * (x - z);
}
MUSE_MODEL_FN double muse_model_dx_dsd(double sd, double n1, double n2, long i) { (void)i; (void)sd; (void)n1; return n2; }
'''


def test_implicit_H_of_a_user_model_on_the_oracle(O):
    """get_H! implicit-differentiation branch (src/muse.jl:335-405) for a header with second derivatives (cubic.h): the CPU
    checker's H from muse_model_second / muse_model_dx_dsd against central differences of the same map (tight MAPs)."""
    theta = [0.3, -0.2]
    with O.user_model(CUBIC, "cubic"):
        H, its = O.implicit_H("user", 2000, 5, 0, theta, atol=1e-12)
        assert np.all(its >= 5) and H[0, 1] == 0.0 and H[1, 0] == 0.0     # (elementwise model: blocks do not couple)
        _, zfid, _ = O.map_and_score_batch("user", 2000, 5, 0, 1, theta, atol=1e-12, z0_mode=0)
        Hfd = O.fd_jacobian("user", 2000, 5, 0, theta, [1e-4] * 2, zfid[0], atol=1e-12)
        np.testing.assert_allclose(H, Hfd, rtol=1e-7, atol=1e-6)
    with O.user_model(os.path.join(HERE, "models", "wrong_score.h"), "wrong_score"):   # a header without them
        assert O.lib().mo_implicit_H(3, 100, 1, 1, 0, O._p(np.zeros(1)), ctypes.c_double(0.1), 10, O._p(np.zeros(1)), None) == -1


def test_second_derivative_check_on_the_host(M):
    """muse_model_eval (the header's functions for one element, on the host: no GPU, no context for a model without run-time
    constants) and the check built on it: cubic.h's second derivatives pass, a wrong one is caught."""
    from museinference_jl_amd import models as MM
    lib = M._capi.load_library(M.ElementwiseModel.packaged("cubic").library())
    assert lib.muse_model_has_second() == 1 and M.load_library().muse_model_has_second() == 1

    def ev(iv, sd, x, z, n1, n2, i=0):
        out = np.full(12, -7.0)
        assert lib.muse_model_eval(None, iv, sd, x, z, n1, n2, int(i), M._capi.ptr(out)) == 0
        assert out[10] == -7.0 and out[11] == -7.0     # a header of the one-parameter family writes ten doubles, as it always did
        return dict(zip(("grad", "term", "B", "ozz", "ozx", "bz", "bx", "z", "x", "dx_dsd"), out.tolist()))
    e = ev(0.7, 1.2, 0.9, 0.4, -0.3, 0.8)
    hp, r = 1 + 0.3 * 0.16, 0.9 - h(0.4)
    np.testing.assert_allclose([e["grad"], e["B"], e["ozz"], e["ozx"], e["bz"], e["bx"]],
                               [0.7 * 0.4 - r * hp, 0.16, 0.7 + hp * hp - r * 0.24, -hp, 0.8, 0.0], rtol=1e-14)
    zs = 1.2 * -0.3
    np.testing.assert_allclose([e["z"], e["x"], e["dx_dsd"]], [zs, h(zs) + 0.8, (1 + 0.3 * zs * zs) * -0.3], rtol=1e-14)
    rs = np.random.RandomState(2)
    x, z, theta = rs.randn(600), 0.7 * rs.randn(600), np.array([0.4, -0.3])
    assert MM._check_second(ev, theta, x, z, 8, 2e-5) <= 2e-5
    for wrong in ("ozz", "ozx", "bz", "dx_dsd"):
        def bad(*a, _w=wrong):
            d = ev(*a)
            d[_w] = 1.05 * d[_w] + 0.01
            return d
        with pytest.raises(AssertionError) as err:
            MM._check_second(bad, theta, x, z, 8, 2e-5)
        assert wrong in str(err.value)
    main = M.load_library()
    assert main.muse_model_eval(None, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0, M._capi.ptr(np.empty(10))) == -1   # built-in models: refused


@pytest.mark.gpu
@pytest.mark.parametrize("N,nth,theta,split", [(3000, 2, [0.4, -0.2], 0), (10000, 1, [0.3], 0), (9999, 3, [0.5, 0.0, -0.4], 0),
                                                (70001, 2, [0.3, 0.1], 0)])
def test_implicit_H_of_the_cubic_model_against_the_oracle(gpu, M, O, N, nth, theta, split):
    """Row f1 for a user-supplied model: get_H! by implicit differentiation through the header's second derivatives -- per-sim H
    and CG iteration counts against the CPU checker's build of the same header, whole simulations and column ranges, and
    (tight MAP) against central differences of the same map."""
    with O.user_model(CUBIC, "cubic"):
        prob = make(M, None, N, nth, -1, split)
        Hs, its = prob.implicit_H_batch(5, 0, 3, theta, atol=1e-1, cg_maxiter=100)
        for s in range(3):
            Ho, io = O.implicit_H("user", N, 5, s, theta, atol=1e-1, cg_maxiter=100)
            assert np.all(np.abs(its[s] - io) <= 1), (its[s], io)     # (the CG stop compares tree-ordered with sequential sums)
            np.testing.assert_allclose(Hs[s], Ho, rtol=1e-7, atol=1e-7 * np.abs(Ho).max())
        cols, ci = prob.implicit_H_columns(5, 0, 1, 2 * nth, theta)           # columns 1 .. 2 nth - 1 of the (sim, column) list
        want = np.concatenate([Hs[s].T for s in range(2)])[1:2 * nth]
        assert np.array_equal(cols, want) or np.allclose(cols, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        Ht, _ = prob.implicit_H_batch(5, 0, 1, theta, atol=1e-10)
        _, zfid, _ = O.map_and_score_batch("user", N, 5, 0, 1, theta, atol=1e-12, z0_mode=0)
        Hfd = O.fd_jacobian("user", N, 5, 0, theta, [1e-4] * nth, zfid[0], atol=1e-12)
        np.testing.assert_allclose(Ht[0], Hfd, rtol=2e-6, atol=2e-6 * np.abs(Hfd).max())
        prob.close()


@pytest.mark.gpu
def test_implicit_H_of_built_in_models_written_as_user_models(gpu, M):
    """The funnel and the noise model written as headers with second derivatives give the built-in models' implicit-differentiation
    H (closed forms in the kernel) -- the noise model being the member with an H1 term (B depends on x)."""
    cases = [("funnel", M.ElementwiseModel.packaged("gaussian_funnel"), 10000, 3, [1.0, 0.0, -1.0]),
             ("funnel", M.ElementwiseModel.packaged("gaussian_funnel"), 70001, 1, [0.5]),
             ("noise", M.ElementwiseModel.from_source("noise_second", NOISE_SECOND_SOURCE), 3001, 1, [0.4]),
             ("noise", M.ElementwiseModel.from_source("noise_second", NOISE_SECOND_SOURCE), 66001, 1, [-0.3])]
    for name, model, N, nth, theta in cases:
        a = M.HipMuseProblem(None, model=name, ntheta=nth, N=N)
        b = M.HipMuseProblem(None, model=model, ntheta=nth, N=N)
        Ha, ia = a.implicit_H_batch(5, 0, 4, theta)
        Hb, ib = b.implicit_H_batch(5, 0, 4, theta)
        assert np.array_equal(ia, ib), (name, N, ia, ib)
        np.testing.assert_allclose(Hb, Ha, rtol=1e-11, atol=1e-11 * np.abs(Ha).max())
        a.close()
        b.close()


@pytest.mark.gpu
def test_get_H_implicit_diff_on_a_user_model(gpu, M, O):
    """muse() + get_H!(implicit_diff=true) (src/muse.jl:335-405) on the non-Gaussian user model: the same H, within Monte-Carlo and
    finite-difference accuracy, as the finite-difference branch on the same streams."""
    with O.user_model(CUBIC, "cubic"):
        x, _ = O.sample_x_z("user", 4000, 9, M.DATA_SIM, [0.2, -0.3])
    prob = M.HipMuseProblem(x, model=M.ElementwiseModel.packaged("cubic"), ntheta=2, prior=M.GaussianPrior(0.0, 3.0))
    res = M.muse(prob, [0.0, 0.0], rng=2, nsims=40, maxsteps=6)
    M.get_H_(res, prob, nsims=8, implicit_diff=True)
    a = res.H.copy()
    assert len(res.metadata["implicit_diff_cg_hists"]) == 8
    res.Hs, res.H = [], None
    M.get_H_(res, prob, nsims=8)
    np.testing.assert_allclose(a, res.H, rtol=0.05, atol=0.05 * np.abs(res.H).max())
    prob.close()


@pytest.mark.gpu
def test_model_from_source_text(gpu, M):
    """ElementwiseModel.from_source: a header given as text (here the noise-scale member of the family with a Laplace-like
    smooth prior), compiled on first use on the GPU box itself, and its contract check."""
    src = '''
#include "muse_model.h"
#define MUSE_MODEL_NAME "softprior"
/* z = n1 (prior N(0,1) times exp(-z^4/4), handled as part of A; the draw ignores the quartic factor: a MAP objective, not a
   sampler test), x ~ N(z, e^theta):  A = z^2 + z^4/2, B = (x - z)^2 */
MUSE_MODEL_FN void muse_model_sample(double sd, double n1, double n2, double* z, double* x, long i) { (void)i; *z = n1; *x = n1 + sd * n2; }
MUSE_MODEL_FN double muse_model_grad(double iv, double x, double z, double* acc, long i) {
    (void)i;
    const double r = x - z, t = iv * r, z2 = z * z;
    *acc = fma(0.5, z2 * z2, fma(z, z, fma(t, r, *acc)));
    return fma(z2, z, z - t);
}
MUSE_MODEL_FN double muse_model_score_term(double x, double z, long i) { (void)i; const double r = x - z; return r * r; }
'''
    model = M.ElementwiseModel.from_source("softprior", src)
    prob = M.HipMuseProblem(None, model=model, ntheta=1, N=4000)
    g, info = prob.map_and_score_batch(1, 0, 8, [0.2], atol=1e-6, z0_mode=0)
    assert np.all(info["status"] == 0) and np.all(info["gnorm"] <= 1e-6) and np.all(info["iterations"] >= 2)
    # stationarity by the per-sim operator: grad_z logLike at the MAP of sim 0
    x, _ = prob.sample_x_z(M.SimRng(1, 0), [0.2])
    zh = prob.get_zhat(0, 1)[0]
    _, gz = prob.logLike_and_grad_z_logLike(x, zh, [0.2])
    assert np.abs(gz).max() <= 1e-6
    np.testing.assert_allclose(g[0], 0.5 * (np.exp(-0.2) * np.sum((x - zh) ** 2) - 4000), rtol=1e-10)
    # a header without MUSE_MODEL_SECOND: the implicit-differentiation H is refused (the finite-difference branch is not)
    assert not prob.has_second_derivatives
    with pytest.raises(M.MuseError) as e:
        prob.implicit_H_batch(9, 0, 2, [0.2])
    assert "second derivatives" in str(e.value)
    assert np.isnan(prob.model_eval(1.0, 1.0, 0.3, 0.2, 0.1, 0.4)["ozz"])
    prob.close()
    bad = src.replace('"softprior"', '"badpad"').replace("return r * r;", "return r * r + 1.0;")
    with pytest.raises(M.MuseError) as e:
        M.HipMuseProblem(None, model=M.ElementwiseModel.from_source("badpad", bad), ntheta=1, N=100)
    assert "muse_model_score_term(0, 0, N) must be 0" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("transport", ["shm", "rccl"])
def test_user_model_through_the_exchange_between_ranks(gpu, M, transport):
    """The sharded map body (solver launch + exchange of the score blocks) in a user model's library, one rank: the
    communicator id comes from libmuse_hip.so, the communicator lives in the model's library; identical to the plain map."""
    N, nth, theta = 6000, 2, [0.3, -0.4]
    p = M.HipMuseProblem(np.random.default_rng(3).normal(size=N), model=M.ElementwiseModel.packaged("cubic"), ntheta=nth)
    p.comm_init(1, 0, M.HipMuseProblem.comm_unique_id(transport))
    assert p.comm_transport() == transport and p.comm_ranks_seen() == 1
    rows = 32
    for b in (0, 24):
        g, info = p.map_and_score_batch(0, b, b + 24, theta, include_data=(b == 0), atol=1e-3)
        n = p.map_and_score_batch_gather_async(0, b, b + 24, theta, rows, include_data=(b == 0), atol=1e-3, result_area=1)
        g_all, info2 = p.batch_wait_gathered(n, rows, 1)
        assert np.array_equal(g_all[0, :n], g) and np.all(g_all[0, n:] == 0.0) and np.array_equal(info, info2)
    p.comm_destroy()
    p.close()


@pytest.mark.gpu
def test_muse_is_calibrated_on_the_non_gaussian_user_model(gpu, M):
    """The reference's acceptance criterion (test/runtests.jl:31,56,81: |theta - truth| / sigma small) as an ensemble: 24 data
    sets of the cubic model -- a non-Gaussian posterior with no closed form, the case MUSE is for -- each with its own master
    seed: the standardized errors (theta_hat - truth) / sigma_MUSE have mean 0 and a standard deviation of about 1."""
    model, truth = M.ElementwiseModel.packaged("cubic"), np.array([0.0, -1.0])
    zs = []
    for d in range(24):
        sim = M.HipMuseProblem(None, model=model, ntheta=2, N=20000)
        x, _ = sim.sample_x_z(M.SimRng(100 + d, M.DATA_SIM), truth)
        sim.close()
        prob = M.HipMuseProblem(x, model=model, ntheta=2, prior=M.GaussianPrior(0.0, 3.0))
        r = M.muse(prob, [0.0, 0.0], nsims=200, rng=d, grad_z_logLike_atol=1e-4, theta_rtol=1e-3, get_covariance=True)
        zs.append((r.theta - truth) / np.sqrt(np.diag(r.Sigma)))
        prob.close()
    zs = np.array(zs)
    assert np.all(np.abs(zs.mean(0)) < 4.0 / np.sqrt(24)), zs.mean(0)
    assert np.all((0.5 < zs.std(0)) & (zs.std(0) < 1.5)), zs.std(0)
    assert np.abs(zs).max() < 4.0


@pytest.mark.gpu
def test_user_model_contexts_do_not_leak(gpu, M):
    """Contexts of two engine libraries (built-in models / a user's model) created, used and destroyed in turn: the device's
    free memory comes back (every library frees its own scratch, results, history and lanes)."""
    import torch
    cubic = M.ElementwiseModel.packaged("cubic")

    def cycle(k):
        p = M.HipMuseProblem(None, model=cubic if k % 2 else "funnel", ntheta=2, N=10000)
        p.set_concurrency(2)
        p.map_and_score_batch(1, 0, 64, [0.1, -0.2], atol=1e-3)
        p.fd_jacobian_batch(1, 0, 4, [0.1, -0.2], [0.05, 0.05], atol=1e-3)
        p.close()

    for k in range(4):
        cycle(k)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for k in range(60):
        cycle(k)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 << 20, (free0, free1)


# ---------------------------------------------------------------------------------- per-element constants (what a closure captures)
SPECTRUM_SOURCE = '''
#define MUSE_MODEL_NAME "spectrum"
/* z_i ~ N(0, e^theta_k P_i) with a KNOWN spectrum P_i (a table compiled into the header: accessor P(i)), x_i ~ N(z_i, 1):
   -logLike = 1/2 sum [ (x - z)^2 + e^-theta z^2 / P_i ] + 1/2 sum n_k theta_k (+ the theta-free 1/2 sum log P_i) */
MUSE_MODEL_FN void muse_model_sample(double sd, double n1, double n2, double* z, double* x, long i) {
    *z = (sd * sqrt(P(i))) * n1;
    *x = *z + n2;
}
MUSE_MODEL_FN double muse_model_grad(double iv, double x, double z, double* acc, long i) {
    const double r = x - z, t = (iv / P(i)) * z;
    *acc = fma(t, z, fma(r, r, *acc));
    return t - r;
}
MUSE_MODEL_FN double muse_model_score_term(double x, double z, long i) {
    (void)x;
    return (z * z) / P(i);
}
'''


def spectrum(N):
    k = np.arange(N) % 200
    return 25.0 / (1.0 + k) ** 1.5 + 0.05        # a repeated power law: three decades of signal-to-noise


def spectrum_exact(x, P, nth, prior_sigma=3.0):
    """Posterior mode and sigma per block of x_i ~ N(0, 1 + e^theta_k P_i): the model is jointly Gaussian, MUSE is exact."""
    from scipy.optimize import brentq
    N = x.size
    kb = (np.arange(N) * nth) // N
    mode, sigma = np.empty(nth), np.empty(nth)
    for b in range(nth):
        xb, Pb = x[kb == b], P[kb == b]
        f = lambda t: 0.5 * np.sum(np.exp(t) * Pb * (xb ** 2 - (1 + np.exp(t) * Pb)) / (1 + np.exp(t) * Pb) ** 2) - t / prior_sigma ** 2
        mode[b] = brentq(f, -8.0, 8.0, xtol=1e-13)
        w = np.exp(mode[b]) * Pb / (1 + np.exp(mode[b]) * Pb)
        sigma[b] = 1.0 / np.sqrt(0.5 * np.sum(w ** 2) + 1.0 / prior_sigma ** 2)
    return mode, sigma


def test_model_with_per_element_constants_on_the_oracle(M, O, tmp_path):
    """ElementwiseModel.from_source(constants={"P": ...}): the table is compiled into the header (accessor P(i), MUSE_MODEL_N).
    On the oracle's build of the generated header: muse() returns the exact marginal posterior (mode to sigma/sqrt(nsims),
    Sigma = sigma^2) -- the spectrum enters draw, gradient and score consistently."""
    from oracle_problem import OracleBatchedProblem
    N, nth, truth, nsims = 3001, 2, [0.5, -0.7], 200
    P = spectrum(N)
    model = M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P": P})
    text = open(model.header).read()
    assert "#define MUSE_MODEL_N 3001" in text and "static const double P_table[3002]" in text
    with O.user_model(model.header, model.library_name):
        x, z = O.sample_x_z("user", N, 99, M.DATA_SIM, truth)
        n1, n2 = O.normals(99, M.DATA_SIM, N)
        kb = (np.arange(N) * nth) // N
        np.testing.assert_allclose(z, np.exp(0.5 * np.asarray(truth))[kb] * np.sqrt(P) * n1, rtol=1e-14)
        res = M.check_model_consistency(OracleBatchedProblem(None, model="user", ntheta=nth, N=N), truth)
        assert max(res["grad_z"], res["grad_theta"]) <= 2e-5 + res["noise_floor"]
        prob = OracleBatchedProblem(x, model="user", ntheta=nth, prior=M.GaussianPrior(0.0, 3.0), nthreads=8)
        r = M.muse(prob, [0.0] * nth, rng=20240, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-7, alpha=1.0, get_covariance=True)
    mode, sigma = spectrum_exact(x, P, nth)
    assert np.all(np.abs(r.theta - mode) / (sigma / np.sqrt(nsims)) < 4.0), (r.theta, mode)
    assert np.all(np.abs(np.sqrt(np.diag(r.Sigma)) / sigma - 1.0) < 0.3)
    assert np.all(np.abs(mode - np.asarray(truth)) / sigma < 4.0)
    with pytest.raises(ValueError):
        M.ElementwiseModel.from_source("bad", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P": P, "Q": P[:10]})
    with pytest.raises(ValueError):
        M.ElementwiseModel.from_source("bad", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P": np.where(np.arange(N) == 7, np.nan, P)})
    with pytest.raises(ValueError):
        M.ElementwiseModel.from_source("bad", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P q": P})
    # the same source with another table is another header, hence another library
    other = M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P": 2.0 * P})
    assert other.header != model.header and other.library_name != model.library_name


def test_runtime_constants_equal_compiled_tables_on_the_oracle(M, O, tmp_path):
    """Run-time constants (include/muse_model.h: MUSE_MODEL_NCONST, muse_const; ElementwiseModel.from_source(...,
    runtime_constants=["P"])): the same model source reads P(i) from a vector set at run time instead of from a table
    compiled into the header -- the same bits on the checker, and another vector without another build."""
    N = 3001
    P = spectrum(N)
    table = M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P": P})
    runtime = M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, directory=str(tmp_path), runtime_constants=["P"])
    assert "#define MUSE_MODEL_NCONST 1" in open(runtime.header).read() and runtime.runtime_constants == ["P"]
    th = [0.5, -0.7]
    with O.user_model(table.header, table.library_name):
        xt, zt = O.sample_x_z("user", N, 99, 5, th)
        gt, zht, it = O.map_and_score_batch("user", N, 42, 0, 4, th, atol=1e-6, z0_mode=0)
    with O.user_model(runtime.header, runtime.library_name):
        O.set_constants(0, P)
        xr, zr = O.sample_x_z("user", N, 99, 5, th)
        gr, zhr, ir = O.map_and_score_batch("user", N, 42, 0, 4, th, atol=1e-6, z0_mode=0)
        assert np.array_equal(xt, xr) and np.array_equal(zt, zr) and np.array_equal(gt, gr) and np.array_equal(zht, zhr)
        assert it.tobytes() == ir.tobytes()
        O.set_constants(0, 2.0 * P)
        x2, _ = O.sample_x_z("user", N, 99, 5, th)
        assert not np.array_equal(x2, xr)
        with pytest.raises(ValueError):
            O.set_constants(1, P)                      # the header declares one constant
    with pytest.raises(ValueError):
        M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, directory=str(tmp_path), constants={"P": P}, runtime_constants=["P"])
    with pytest.raises(ValueError):
        M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, directory=str(tmp_path), runtime_constants=["P q"])


@pytest.mark.gpu
@pytest.mark.parametrize("N,nth,placement,split", [(10000, 2, -1, 0), (9999, 1, -1, 4), (70001, 2, -1, 0), (2001, 1, 0, 0)])
def test_runtime_constants_on_hip(gpu, M, O, N, nth, placement, split):
    """The same on the engine (muse_set_constants): ONE library for every N and every P -- draw bit for bit and MAP / counts /
    scores against the checker with the same vector, in the resident, cluster and streaming placements; the vector replaced
    without a build; two contexts of the library with different vectors, launching in turn, each see their own; the native
    muse! loops run on it."""
    model = M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, runtime_constants=["P"])
    P = spectrum(N)
    truth = [0.5, -0.7][:nth]
    with O.user_model(model.header, model.library_name):
        O.set_constants(0, P)
        x, _ = O.sample_x_z("user", N, 99, M.DATA_SIM, truth)
        prob = make(M, x, N, nth, placement, split, model=model, prior=M.GaussianPrior(0.0, 3.0))
        with pytest.raises((M.MuseError, ValueError)):
            prob.set_constants("P", P[:-1])            # one entry per element
        with pytest.raises(M.MuseError):
            prob.set_constants("P", np.where(np.arange(N) == 3, np.inf, P))
        prob.set_constants("P", P)
        other = make(M, x, N, nth, placement, split, model=model, prior=M.GaussianPrior(0.0, 3.0))
        other.set_constants("P", 3.0 * P)              # installs ITS vector for the library ...
        for vec, p in ((P, prob), (3.0 * P, other), (P, prob)):     # ... and every context still sees its own when it launches
            O.set_constants(0, vec)
            xs, zs = p.sample_x_z(M.SimRng(5, 3), truth)
            xo, zo = O.sample_x_z("user", N, 5, 3, truth)
            assert np.array_equal(xs, xo) and np.array_equal(zs, zo)
            n = 6
            g, info = p.map_and_score_batch(42, 0, n, truth, include_data=True, atol=1e-6, z0_mode=0)
            go, zo, io = O.map_and_score_batch("user", N, 42, 0, n, truth, atol=1e-6, x_data=x, z0_mode=0)
            same = assert_same_path_or_close(info, io, p.get_zhat(0, n + 1), zo, g, go, 1e-6, truth, "funnel",
                                             hess_inf=1.0 + np.exp(-min(truth)) / np.min(vec))     # grad^2 f = 1 + e^-theta / P_i
            assert same.all()
        # The pointers travel with every LAUNCH (round 5; a process-wide device symbol before): maps of the two contexts enqueued
        # back to back, none waited for until all are in flight, give what each context gives alone.
        alone = {}
        for name, p in (("prob", prob), ("other", other)):
            p.set_normals_cache(False)
            alone[name] = p.map_and_score_batch(17, 0, 24, truth, include_data=True, atol=1e-6, z0_mode=0)
        pend = []
        for k in range(3):
            for name, p in (("prob", prob), ("other", other)):
                pend.append((name, p, k, p.map_and_score_batch_async(17, 0, 24, truth, include_data=True, atol=1e-6, z0_mode=0,
                                                                     result_area=k)))
        for name, p, k, n in pend:
            g, info = p.batch_wait(n, k)
            assert np.array_equal(g, alone[name][0]) and np.array_equal(info, alone[name][1]), (name, k)
        assert not np.array_equal(alone["prob"][0], alone["other"][0])
        other.close()
        prob.set_constants("P", 2.0 * P)               # another spectrum: no build
        O.set_constants(0, 2.0 * P)
        g, info = prob.map_and_score_batch(42, 0, 4, truth, atol=1e-6, z0_mode=1)
        go, zo, io = O.map_and_score_batch("user", N, 42, 0, 4, truth, atol=1e-6, z0_mode=1)
        assert np.array_equal(info["f_calls"], io["f_calls"])
        np.testing.assert_allclose(g, go, rtol=1e-9)
    a = prob.run_muse(7, [0.0] * nth, nsims=24, maxsteps=4, theta_rtol=0.0, atol=1e-4, alpha=0.8, device_loop=False)
    b = prob.run_muse(7, [0.0] * nth, nsims=24, maxsteps=4, theta_rtol=0.0, atol=1e-4, alpha=0.8, device_loop=True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    prob.close()


SPECTRUM_SIZES = (10000, 9999, 70001)     # (tests/prebuild_models.py compiles these libraries ahead of time)


@pytest.mark.gpu
@pytest.mark.parametrize("N,nth,truth,placement,split", [(10000, 2, [0.5, -0.7], -1, 0), (9999, 1, [0.3], -1, 4), (70001, 2, [0.2, -0.3], -1, 0)])
def test_model_with_per_element_constants_on_hip(gpu, M, O, N, nth, truth, placement, split):
    """The same model on the engine, in the resident, cluster and streaming placements (odd N: the pad element and the phantom
    slots behind it index the table's last entry): draw bit for bit and MAP / counts / scores against the oracle's build of the
    generated header; the engine refuses another N; muse() returns the exact marginal posterior."""
    P = spectrum(N)
    # (default directory, museinference.jl_amd/models/user/: the library, named after the hash of the generated header, is
    #  compiled once per tree and N -- ~40 s -- not once per test run)
    model = M.ElementwiseModel.from_source("spectrum", SPECTRUM_SOURCE, constants={"P": P})
    with pytest.raises(M.MuseError) as e:
        M.HipMuseProblem(None, model=model, ntheta=nth, N=N + 1)
    assert "built for another N" in str(e.value)
    with O.user_model(model.header, model.library_name):
        x, _ = O.sample_x_z("user", N, 99, M.DATA_SIM, truth)
        prob = make(M, x, N, nth, placement, split, model=model, prior=M.GaussianPrior(0.0, 3.0))
        xs, zs = prob.sample_x_z(M.SimRng(5, 3), truth)
        xo, zo = O.sample_x_z("user", N, 5, 3, truth)
        assert np.array_equal(xs, xo) and np.array_equal(zs, zo)
        n = 9
        g, info = prob.map_and_score_batch(42, 0, n, truth, include_data=True, atol=1e-6, z0_mode=0)
        go, zo, io = O.map_and_score_batch("user", N, 42, 0, n, truth, atol=1e-6, x_data=x, z0_mode=0)
        same = assert_same_path_or_close(info, io, prob.get_zhat(0, n + 1), zo, g, go, 1e-6, truth, "funnel",
                                         hess_inf=1.0 + np.exp(-min(truth)) / np.min(P))     # grad^2 f = 1 + e^-theta / P_i
        assert same.all()
    nsims = 256 if N <= 10000 else 64
    r = M.muse(prob, [0.0] * nth, rng=20240, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-7, alpha=1.0, get_covariance=True)
    mode, sigma = spectrum_exact(x, P, nth)
    assert np.all(np.abs(r.theta - mode) / (sigma / np.sqrt(nsims)) < 4.0), (r.theta, mode)
    assert np.all(np.abs(np.sqrt(np.diag(r.Sigma)) / sigma - 1.0) < 0.3)
    prob.close()
