"""The per-element exponential of device code (csrc/model_math.hpp, muse::model_exp: what muse_model_exp resolves to in a header's
per-element functions) and the two shipped models that call it, on the GPU against the CPU checker.

  * the BITS of the device exponential, read back through the sampler of tests/models/exp_probe.h, against the checker's
    fixed-sequence exp over the argument set of tests/test_muse_exp.py and the special arguments;
  * models/stochastic_volatility.h and models/lognormal_obs.h in every placement of the solver kernel: the draw bit for bit, the
    maps on the checker's path (identical iteration and evaluation counts, MAPs to 1e-9, scores to 1e-10), placement independence,
    get_H! by implicit differentiation and by finite differences, a whole muse() run.

The libraries are built by the non-GPU tests of tests/test_model_exp_models.py (and by build()): this file finds them built."""
import numpy as np
import pytest

import model_exp_cases as K
from test_gpu_parity import assert_same_path_or_close
from test_model_exp_models import LN, PROBE, SV, sv_implicit_H


# ------------------------------------------------------------------------------------------------ the bits
@pytest.mark.gpu
def test_device_exp_has_the_bits_of_the_fixed_sequence_exp(gpu, M, O):
    xs = K.arguments()
    N = xs.size
    sel = np.where(np.isposinf(xs), 1.0, np.where(np.isneginf(xs), 2.0, np.where(np.isnan(xs), 3.0, 0.0)))
    prob = M.HipMuseProblem(None, model=M.ElementwiseModel("exp_probe", PROBE), ntheta=1, N=N)
    prob.set_constants(0, np.where(np.isfinite(xs), xs, 0.0))
    prob.set_constants(1, sel)
    x, _ = prob.sample_x_z(M.SimRng(1, 0), [0.0])
    prob.close()
    want = np.array([O.exp_fixed(v) for v in xs])
    bad = ~K.same_bits(x, want)
    assert not bad.any(), (int(bad.sum()), xs[bad][:8], x[bad][:8], want[bad][:8])
    assert (sel > 0).sum() == 3 and np.isnan(x).sum() == 1 and np.isposinf(x).sum() > 3 and (x == 0.0).sum() > 3
    assert ((x > 0) & (x < 2.0 ** -1022)).sum() > 10_000                       # subnormal results were among them


# ------------------------------------------------------------------------------------------------ the models against the checker
def hess_inf_sv(theta, zo, atol):
    """The infinity norm of grad_z^2 f of the stochastic-volatility model near a MAP: ozz = 1/2 x^2 e^-z + iv, and at a MAP
    1/2 x^2 e^-z = 1/2 + iv (z - mu) +- atol."""
    theta = np.asarray(theta, dtype=np.float64)
    K_ = theta.size // 2
    iv = float(np.exp(-theta[K_:].min()))
    return 0.5 + iv * (1.0 + float(np.abs(zo).max()) + float(np.abs(theta[:K_]).max())) + atol


def hess_inf_ln(theta, zo, atol):
    """... of the log-normal observation model: ozz = iv + e^z - (x - h) e^(z/2) / 2, and at a MAP (x - h) e^(z/2) = iv z +- atol."""
    iv, m = float(np.exp(-np.min(theta))), float(np.abs(zo).max())
    return iv * (1.0 + 0.5 * m) + float(np.exp(m)) + atol


def against_the_checker(M, O, header, name, hess_inf, N, nth, theta, placement, split, nsims, long, resident):
    model = M.ElementwiseModel.packaged(name)
    with O.user_model(header, name):
        xdata, _ = O.sample_x_z("user", N, 77, M.DATA_SIM, np.zeros(nth))
        prob = M.HipMuseProblem(xdata, model=model, ntheta=nth)
        if placement >= 0:
            prob.set_placement(placement)
        if split:
            prob.set_element_split(split)
        ran = prob.placement_info()
        assert ran["resident"] == resident, (name, N, nth, ran)     # (the placement that runs is the one the row is about)
        for sim in (0, 2**40 + 7):   # the draw, bit for bit
            x, z = prob.sample_x_z(M.SimRng(1234, sim), theta)
            xo, zo = O.sample_x_z("user", N, 1234, sim, theta)
            assert np.array_equal(z, zo) and np.array_equal(x, xo)
        zz = 0.7 * zo + 0.1
        f, g = prob.logLike_and_grad_z_logLike(xo, zz, theta)
        fo, go = O.logLike_and_grad_z("user", xo, zz, theta)
        np.testing.assert_allclose(f, fo, rtol=1e-12)
        np.testing.assert_allclose(g, go, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(prob.grad_theta_logLike(xo, zz, theta), O.grad_theta("user", xo, zz, theta), rtol=1e-11, atol=1e-11)
        for z0_mode in (0, 1):
            g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4, z0_mode=z0_mode)
            go, zo, io = O.map_and_score_batch("user", N, 42, 3, 3 + nsims, theta, atol=1e-4, x_data=xdata, z0_mode=z0_mode)
            zh = prob.get_zhat(0, nsims + 1)
            many = long      # (the cubic test's rule for long solves: MAPs to 1e-7, scores to 1e-6 along the same path, a same-path share of 0.8)
            print(name, N, nth, placement, split, "z0_mode", z0_mode, "iterations", io["iterations"].min(), io["iterations"].max(), ran)
            same = assert_same_path_or_close(info, io, zh, zo, g, go, 1e-4, theta, "funnel", ctx=f"z0_mode {z0_mode}",
                                             hess_inf=hess_inf(theta, zo, 1e-4), z_atol=1e-7 if many else 1e-9, g_rtol=1e-6 if many else 1e-10)
            assert same.all() if not long else same.mean() >= 0.8, (info["iterations"], io["iterations"], info["f_calls"], io["f_calls"])
            assert info["iterations"].min() >= 2
        prob.close()


SV_ROWS = [  # (N, theta, placement, split, sims, long, resident)
    (37, [0.3, -0.5], -1, 0, 13, False, True),                      # PlaceResident<256, 1>
    (513, [0.3, -0.5], -1, 0, 13, False, True),                     # PlaceResident<512, 4>
    (2000, [0.2, -0.4, -0.3, 0.1], -1, 4, 13, False, True),         # register clusters of four workgroups
    (4097, [0.3, -0.5], -1, 0, 13, False, True),                    # PlaceResident<512, 10>, odd N: the pad element
    (300, [0.3, -0.5], 0, 0, 13, False, False),                     # streaming, one workgroup
    (65537, [0.3, -0.5], -1, 0, 3, False, False),                   # streaming clusters
    (4097, [-0.5, 0.4, 0.1, -0.2, 0.5, -1.0, -0.3, 0.2], -1, 0, 13, True, False),   # four blocks: fenced, the streaming kernel runs
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,theta,placement,split,nsims,long,resident", SV_ROWS)
def test_stochastic_volatility_hip_against_the_checker(gpu, M, O, N, theta, placement, split, nsims, long, resident):
    against_the_checker(M, O, SV, "stochastic_volatility", hess_inf_sv, N, len(theta), theta, placement, split, nsims, long, resident)


LN_ROWS = [(37, [0.0], -1, 13, False, True), (513, [-0.5], -1, 13, False, True), (300, [-0.5, -0.2], 0, 13, False, False),
           (4097, [-0.5], -1, 13, True, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,theta,placement,nsims,long,resident", LN_ROWS)
def test_lognormal_obs_hip_against_the_checker(gpu, M, O, N, theta, placement, nsims, long, resident):
    against_the_checker(M, O, LN, "lognormal_obs", hess_inf_ln, N, len(theta), theta, placement, 0, nsims, long, resident)


@pytest.mark.gpu
@pytest.mark.parametrize("name,theta", [("stochastic_volatility", [0.3, -0.5]), ("stochastic_volatility", [-0.5, 0.4, 0.1, -0.2, 0.5, -1.0, -0.3, 0.2]),
                                        ("lognormal_obs", [-0.5])])
def test_placement_independence_with_an_exponential(gpu, M, name, theta):
    """N = 4097: the LDS-resident solve (ten element pairs per thread, the exponential inlined ten times over) and the streaming one
    give the same bits -- scores, solver records, MAPs.  Where the engine's fence routed the resident shape (the eight-parameter
    stochastic-volatility kernel keeps its state in scratch) both runs are the streaming kernel's, and the test says so."""
    N, out = 4097, []
    model = M.ElementwiseModel.packaged(name)
    sim = M.HipMuseProblem(None, model=model, ntheta=len(theta), N=N)
    x, _ = sim.sample_x_z(M.SimRng(77, M.DATA_SIM), np.zeros(len(theta)))      # the data: the DATA_SIM draw at theta = 0
    sim.close()
    for placement in (-1, 0):
        prob = M.HipMuseProblem(x, model=model, ntheta=len(theta))
        if placement == 0:
            prob.set_placement(0)
        ran = prob.placement_info()
        if placement == -1 and not ran["resident"]:
            print(f"{name} ntheta={len(theta)}: the resident map kernel is beyond the scratch bound, the streaming placement ran: {ran}")
        g, info = prob.map_and_score_batch(42, 0, 12, theta, include_data=True, atol=1e-4, z0_mode=0)
        out.append((g, info.tobytes(), prob.get_zhat(0, 13), ran))
        prob.close()
    assert not out[1][3]["resident"] and out[0][3]["resident"] == (len(theta) == 2 or name != "stochastic_volatility")
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])


@pytest.mark.gpu
def test_the_fence_routes_what_is_beyond_the_bound_and_nothing_else(gpu, M):
    """The engine's fence of resident map kernels (muse_engine.cpp, map_unfit_mask) against what the libraries' code objects say
    (profiles/r18_model_exp_resources.txt): at N = 4097 -- PlaceResident<512, 10> -- the two- and four-block stochastic-volatility
    kernels (328 / 296 bytes of scratch per lane) stream, the one-block kernel (8 bytes) and every kernel of lognormal_obs, cubic and
    normal_mean_var stay resident; smaller placements of stochastic_volatility are untouched; and set_placement(0) still streams."""
    cases = [("stochastic_volatility", 2, 4097, True), ("stochastic_volatility", 4, 4097, False), ("stochastic_volatility", 8, 4097, False),
             ("stochastic_volatility", 4, 2000, True), ("stochastic_volatility", 8, 300, True),
             ("lognormal_obs", 1, 4097, True), ("lognormal_obs", 8, 4097, True),
             ("cubic", 1, 4097, True), ("cubic", 8, 4097, True), ("cubic", 1, 10000, True),
             ("normal_mean_var", 2, 4097, True), ("normal_mean_var", 4, 4097, True), ("normal_mean_var", 8, 4097, True), ("normal_mean_var", 8, 10000, True)]
    for name, nth, N, resident in cases:
        prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged(name), ntheta=nth, N=N)
        ran = prob.placement_info()
        assert ran["resident"] == resident and ran["workgroups_per_element"] == 1, (name, nth, N, ran)
        prob.set_placement(0)
        assert not prob.placement_info()["resident"], (name, nth, N)
        prob.close()


# ------------------------------------------------------------------------------------------------ get_H!
@pytest.mark.gpu
def test_implicit_and_fd_H_of_stochastic_volatility(gpu, M, O):
    """get_H! by implicit differentiation through muse_model_pair_second / muse_model_pair_dx against the numpy restatement at the
    checker's MAP (the checker itself has no implicit-differentiation H of the two-parameter family; the Hessian in z is diagonal,
    so with the diagonal preconditioner one CG iteration solves a column exactly: rtol 1e-9), the unpreconditioned CG against the
    same to its stopping rule, and against the checker's finite-difference Jacobian to the tolerance of the cubic model's test."""
    N, theta = 3000, [0.3, -0.5]
    prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("stochastic_volatility"), ntheta=2, N=N)
    assert prob.has_second_derivatives
    Hj, itj = prob.implicit_H_batch(5, 0, 3, theta, atol=1e-10, cg_Pl="jacobi")
    Hc, itc = prob.implicit_H_batch(5, 0, 3, theta, atol=1e-10)
    assert np.all(itj == 1) and np.all(itc > 1)
    with O.user_model(SV, "stochastic_volatility"):
        for s in range(3):
            _, zfid, _ = O.map_and_score_batch("user", N, 5, s, s + 1, theta, atol=1e-12, z0_mode=0)
            Ho = sv_implicit_H(O, N, 5, s, theta, zfid[0])
            np.testing.assert_allclose(Hj[s], Ho, rtol=1e-9, atol=1e-9 * np.abs(Ho).max())
            np.testing.assert_allclose(Hc[s], Ho, rtol=1e-6, atol=1e-6 * np.abs(Ho).max())       # (CG stops at sqrt(eps) |b|)
        _, zfid, _ = O.map_and_score_batch("user", N, 5, 0, 1, theta, atol=1e-12, z0_mode=0)
        Hfd = O.fd_jacobian("user", N, 5, 0, theta, [1e-4] * 2, zfid[0], atol=1e-12)
        np.testing.assert_allclose(Hj[0], Hfd, rtol=2e-6, atol=2e-6 * np.abs(Hfd).max())
        # ... and the engine's own finite-difference branch against the checker's
        step = np.array([0.05, 0.04])
        Hs, _ = prob.fd_jacobian_batch(9, 0, 3, theta, step, atol=1e-4)
        _, zf, _ = O.map_and_score_batch("user", N, 9, M.MASTER_SIM, M.MASTER_SIM + 1, theta, atol=1e-4, z0_mode=0)
        for s in range(3):
            np.testing.assert_allclose(Hs[s], O.fd_jacobian("user", N, 9, s, theta, step, zf[0], atol=1e-4), rtol=1e-8, atol=1e-9)
    prob.close()


@pytest.mark.gpu
def test_implicit_H_of_lognormal_obs(gpu, M, O):
    """One-parameter family: the implicit-differentiation batch against the checker's (CG counts within one, H to 1e-7 as for the
    cubic model), and with Pl = "jacobi" one CG iteration per column and the same H."""
    N, theta = 3000, [-0.3]
    prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("lognormal_obs"), ntheta=1, N=N)
    Hs, its = prob.implicit_H_batch(5, 0, 3, theta, atol=1e-1, cg_maxiter=100)
    with O.user_model(LN, "lognormal_obs"):
        for s in range(3):
            Ho, io = O.implicit_H("user", N, 5, s, theta, atol=1e-1, cg_maxiter=100)
            assert np.all(np.abs(its[s] - io) <= 1), (its[s], io)
            np.testing.assert_allclose(Hs[s], Ho, rtol=1e-7, atol=1e-7 * np.abs(Ho).max())
    Hj, itj = prob.implicit_H_batch(5, 0, 3, theta, atol=1e-8, cg_Pl="jacobi")
    Hc, _ = prob.implicit_H_batch(5, 0, 3, theta, atol=1e-8)
    assert np.all(itj == 1), itj
    np.testing.assert_allclose(Hj, Hc, rtol=1e-6)
    prob.close()


# ------------------------------------------------------------------------------------------------ muse()
@pytest.mark.gpu
def test_muse_on_stochastic_volatility(gpu, M):
    """muse() end to end on the model MUSE is for: N = 10^4, truth (mu, tau) = (-0.5, 0.4), 100 simulations, with the covariance:
    the estimate within 4 sigma of the truth per component; the device-resident loop gives the host loop's bits (where the loop
    kernel is beyond the scratch bound muse_run_device hands the run to the host loop: the same comparison holds)."""
    N, truth = 10000, np.array([-0.5, 0.4])
    model = M.ElementwiseModel.packaged("stochastic_volatility")
    sim = M.HipMuseProblem(None, model=model, ntheta=2, N=N)
    x, _ = sim.sample_x_z(M.SimRng(2024, M.DATA_SIM), truth)
    sim.close()
    prob = M.HipMuseProblem(x, model=model, ntheta=2, prior=M.GaussianPrior(0.0, 3.0))
    kw = dict(nsims=100, maxsteps=4, theta_rtol=0.0, atol=1e-4, alpha=0.7)
    b = prob.run_muse(11, [0.0, 0.0], device_loop=False, **kw)
    a = prob.run_muse(11, [0.0, 0.0], device_loop=True, **kw)
    assert a[0] == b[0] == 4 and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and a[4].tobytes() == b[4].tobytes()
    res = M.muse(prob, [0.0, 0.0], rng=11, nsims=100, maxsteps=30, theta_rtol=1e-3, grad_z_logLike_atol=1e-4, get_covariance=True)
    sigma = np.sqrt(np.diag(res.Sigma))
    print("stochastic volatility: theta", res.theta, "sigma", sigma, "truth", truth)
    assert np.all(np.abs(np.asarray(res.theta) - truth) / sigma < 4.0), (res.theta, sigma)
    prob.close()
