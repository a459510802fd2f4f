"""-m gpu: the HIP path against the extended-precision reference (tests/hp_reference.py) alone -- no oracle in any assertion.

What parity with the oracle cannot see (a formula or constant both sides share) and what it never compared (a solver record's
f_min and gnorm) are checked here against the mathematics:
- the generator on the device within the committed bound K_GEN of tests/test_hp_reference.py;
- the per-sim operators at block and workgroup edges within C_ROUND 2^-53 cond (hp_reference's docstring derives C_ROUND = 16);
- every solver record against the MAP the kernel wrote out: (a) status g_converged => |grad f_hp(zhat)|_inf <= atol + the
  gradient's rounding bound (the kernel tests its own fp64 gradient); (b) |gnorm - |grad f_hp(zhat)|_inf| <= that bound, for
  every status; (c) f_min = f_hp(zhat) within C_ROUND 2^-53 cond_f; (d) the score = score_hp(zhat) within its bound; (e) for the
  Gaussian models zhat - z* = H^-1 g: per element |g_i| / H_ii (diagonal models), |g|_2 / lambda_min with
  lambda_min >= e^{-theta_max} (smooth: A^T A is positive semi-definite);
- the implicit-differentiation H against the reference's, at rtol 1e-6 (CG's stopping rule, not rounding: test_hp_reference.py).
"""
import numpy as np
import pytest

import hp_reference as R
from test_hp_reference import K_GEN

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

GAUSSIAN = ("funnel", "noise", "smooth", "normal_mean_var")


def check_records(model, xs, theta, zh, g, info, atol, ctx=""):
    """(a)-(e) of the module docstring for every element; xs[e] the element's x.  Returns the statuses seen."""
    for e in range(len(info)):
        c = f"{ctx} element {e} status {info['status'][e]}"
        f, gz, cf, cg = R.objective(model, xs[e], zh[e], theta)
        gi = np.abs(gz).astype(np.float64)
        gb = float(R.rounding(cg).max())
        if info["status"][e] == 0:
            assert gi.max() <= atol + gb, (c, gi.max(), atol)
        assert abs(info["gnorm"][e] - gi.max()) <= gb, (c, "gnorm", info["gnorm"][e], gi.max(), gb)
        assert abs(info["f_min"][e] - f) <= R.rounding(cf), (c, "f_min", info["f_min"][e], float(f), float(R.rounding(cf)))
        s, cs = R.score(model, xs[e], zh[e], theta)
        assert (np.abs(g[e] - s) <= R.rounding(cs)).all(), (c, "score", g[e], s.astype(np.float64))
        if model in GAUSSIAN:
            zs = R.exact_map(model, xs[e], theta)
            dz = np.abs((zh[e] - zs).astype(np.float64))
            if model == "smooth":
                lam = np.exp(-np.max(theta))
                assert np.linalg.norm(dz) <= (np.linalg.norm(gi) + np.sqrt(gi.size) * gb) / lam, c
            else:
                assert (dz <= (gi + gb) / R.diag_hessian(model, xs[e], zh[e], theta).astype(np.float64)).all(), c
    return set(int(s) for s in info["status"])


def xs_of(prob, M, seed, sim_begin, sim_end, theta, xdata=None):
    rows = [] if xdata is None else [np.asarray(xdata, np.float64)]
    for sim in range(sim_begin, sim_end):
        rows.append(prob.sample_x_z(M.SimRng(seed, sim), theta)[0])
    return rows


def run_map(prob, M, model, theta, xdata, *, seed=42, s0=3, nsims=8, atol=1e-4, z0_mode=0, ctx=""):
    g, info = prob.map_and_score_batch(seed, s0, s0 + nsims, theta, include_data=xdata is not None, atol=atol, z0_mode=z0_mode)
    zh = prob.get_zhat(0, len(info))
    return check_records(model, xs_of(prob, M, seed, s0, s0 + nsims, theta, xdata), theta, zh, g, info, atol, ctx)


# ------------------------------------------------------------------------------------------------ 1. the generator
def test_device_generator_within_K(gpu, M):
    """noise at theta = 0: z = n1 exactly, x = fl(n1 + n2) (sd = exp(0) = 1 exactly).  2.4e6 elements over four sims."""
    N = 600_000
    prob = M.HipMuseProblem(None, model="noise", ntheta=1, N=N)
    for sim in (0, 1, 3, 2**40 + 7):
        x, z = prob.sample_x_z(M.SimRng(1234, sim), [0.0])
        h1, h2, r = R.normals(1234, sim, N)
        tol = K_GEN * 2.0**-52 * np.maximum(1.0, r.astype(np.float64))
        assert (np.abs(z - h1).astype(np.float64) <= tol).all(), sim
        # x: two normals within K each, then one rounding of their sum
        assert (np.abs(x - (h1 + h2)).astype(np.float64) <= 2 * tol + R.U * np.abs(x)).all(), sim
    prob.close()


# ------------------------------------------------------------------------------------------------ 2. per-sim operators
EDGE_N = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 9999, 10000, 10001, 65535, 65536, 65537]


def _operators(M, model, lib_model, N, theta):
    prob = M.HipMuseProblem(None, model=lib_model, ntheta=len(theta), N=N)
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    zz = 0.7 * z + 0.1
    f, gz = prob.logLike_and_grad_z_logLike(x, zz, theta)
    fh, gh, cf, cg = R.objective(model, x, zz, theta)
    ctx = (model, N, len(theta))
    assert abs(-f - fh) <= R.rounding(cf), ctx
    assert (np.abs(-gz - gh) <= R.rounding(cg)).all(), ctx
    s, cs = R.score(model, x, zz, theta)
    assert (np.abs(prob.grad_theta_logLike(x, zz, theta) - s) <= R.rounding(cs)).all(), ctx
    prob.close()


@pytest.mark.parametrize("N", EDGE_N)
def test_operators_at_the_edges(gpu, M, N):
    rng = np.random.default_rng(N)
    for model in ("funnel", "noise", "smooth"):
        for nth in ([1] if model == "noise" else [1, 2, 3, 8, 9, 33, 64]):
            if nth <= N and (model != "smooth" or N >= 5):     # (the engine's stencil model needs N >= 5)
                _operators(M, model, model, N, np.round(rng.uniform(-1.0, 1.5, nth), 3))


@pytest.mark.parametrize("N", EDGE_N)
def test_user_model_operators_at_the_edges(gpu, M, N):
    rng = np.random.default_rng(N)
    cubic, pair = M.ElementwiseModel.packaged("cubic"), M.ElementwiseModel.packaged("normal_mean_var")
    for nth in (1, 2, 3, 8, 9, 33, 64):
        if nth <= N:
            _operators(M, "cubic", cubic, N, np.round(rng.uniform(-1.0, 1.0, nth), 3))
    for nth in (2, 4, 8):
        if nth <= N:
            _operators(M, "normal_mean_var", pair, N, np.round(rng.uniform(-1.0, 1.0, nth), 3))


# ------------------------------------------------------------------------------------------------ 3. solver records
def _lin(n):
    return list(np.round(np.linspace(-1.0, 1.5, n), 3))


def _builtin_rows():
    """(model, N, ntheta, theta, placement, split): every solver instantiation of test_user_model.PLACEMENTS for funnel (as listed)
    and noise (one component), then the stencil model's placements and the big tier."""
    from test_user_model import PLACEMENTS
    rows = [("funnel", N, nth, list(th), pl, sp) for N, nth, th, pl, sp in PLACEMENTS]
    for N, nth, th, pl, sp in PLACEMENTS:
        if ("noise", N, 1, [th[0]], pl, sp) not in rows:
            rows.append(("noise", N, 1, [th[0]], pl, sp))
    rows += [("funnel", 9999, 1, [-0.4], -1, 0), ("noise", 513, 1, [0.3], 0, 0),      # odd N: the pad element
             ("smooth", 601, 4, [1.0, 2.0, 3.0, 0.5], -1, 0), ("smooth", 66001, 2, [1.0, 2.5], -1, 0),
             ("funnel", 9999, 33, _lin(33), -1, 0), ("smooth", 3001, 17, _lin(17), -1, 0), ("funnel", 10000, 64, _lin(64), -1, 0),
             ("funnel", 10000, 16, _lin(16), -1, 4)]
    return rows


BUILTIN = _builtin_rows()


def _make(M, model, xdata, N, nth, placement, split):
    prob = M.HipMuseProblem(xdata, model=model, ntheta=nth, N=None if xdata is not None else N)
    if placement >= 0:
        prob.set_placement(placement)
    if split:
        prob.set_element_split(split)
    return prob


@pytest.mark.parametrize("model,N,nth,theta,placement,split", BUILTIN)
def test_records_describe_their_map(gpu, M, model, N, nth, theta, placement, split):
    theta = np.asarray(theta)
    draw = M.HipMuseProblem(None, model=model, ntheta=nth, N=N)
    xdata = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    draw.close()
    prob = _make(M, model, xdata, N, nth, placement, split)
    nsims = 4 if N > 20000 else 8
    for z0_mode in (0, 1):
        run_map(prob, M, model, theta, xdata, nsims=nsims, z0_mode=z0_mode, ctx=f"z0_mode {z0_mode}")
    run_map(prob, M, model, theta + 0.05, xdata, nsims=nsims, atol=1e-6, z0_mode=M.Z0_WARM, ctx="warm")
    if nth == 1 and model != "smooth":     # the speculating trial (solver.hpp, eval SPEC) switched off: debug bit 5
        prob.debug_flags(1 << 5)
        run_map(prob, M, model, theta, xdata, nsims=nsims, z0_mode=0, ctx="no speculation")
        prob.debug_flags(0)
    prob.close()


def _user_records(M, name, placements):
    lib_model = M.ElementwiseModel.packaged(name)
    for N, nth, theta, placement, split in placements:
        theta = np.asarray(theta)
        draw = M.HipMuseProblem(None, model=lib_model, ntheta=nth, N=N)
        xdata = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
        draw.close()
        prob = _make(M, lib_model, xdata, N, nth, placement, split)
        nsims = 3 if N > 20000 else 6
        for z0_mode in (0, 1):
            run_map(prob, M, name, theta, xdata, nsims=nsims, z0_mode=z0_mode, ctx=f"{name} {N} {nth} {placement} {split} z0 {z0_mode}")
        prob.close()


def test_records_of_the_cubic_placements(gpu, M):
    from test_user_model import PLACEMENTS
    _user_records(M, "cubic", PLACEMENTS)


def test_records_of_the_pair_placements(gpu, M):
    from test_pair_model import PLACEMENTS
    _user_records(M, "normal_mean_var", PLACEMENTS)


def test_records_of_a_multi_map_launch_and_two_lanes(gpu, M):
    N, nth, seed, nsims, atol = 4097, 2, 9, 6, 1e-5
    prob = M.HipMuseProblem(None, model="funnel", ntheta=nth, N=N)
    prob.set_concurrency(2)
    thetas = np.array([[0.3, -0.2], [1.0, 0.4], [-0.6, 0.9]])
    n = prob.map_and_score_multi_async(seed, 0, nsims, thetas, atol=atol)
    g, info = prob.batch_wait(n, 0)
    zh = prob.get_zhat(0, n)
    for m, th in enumerate(thetas):       # element e of map m: row and slot m n + e (include/muse_hip.h)
        rows = slice(m * nsims, (m + 1) * nsims)
        check_records("funnel", xs_of(prob, M, seed, 0, nsims, th), th, zh[rows], g[rows], info[rows], atol, f"map {m}")
    # the second lane (result area 1) keeps MAP slots of its own, which muse_get_zhat does not address (include/muse_hip.h):
    # its records must be those of the same map on lane 0, whose MAPs are checked
    n0 = prob.map_and_score_batch_async(seed, 10, 10 + nsims, thetas[1], atol=atol, result_area=0)
    g0, i0 = prob.batch_wait(n0, 0)
    check_records("funnel", xs_of(prob, M, seed, 10, 10 + nsims, thetas[1]), thetas[1], prob.get_zhat(0, n0), g0, i0, atol, "lane 0")
    n1 = prob.map_and_score_batch_async(seed, 10, 10 + nsims, thetas[1], atol=atol, result_area=1)
    g1, i1 = prob.batch_wait(n1, 1)
    assert np.array_equal(g1, g0) and np.array_equal(i1, i0)
    prob.close()


@pytest.mark.parametrize("model,theta", [("funnel", [0.3]), ("noise", [-0.4])])
def test_records_of_streaming_clusters_drawing_in_the_background(gpu, M, model, theta):
    """test_streaming_clusters_draw_the_next_problem_in_the_background's case: 150 problems on 64 clusters of 8."""
    N, nsims, seed = 70001, 150, 31
    draw = M.HipMuseProblem(None, model=model, ntheta=1, N=N)
    xdata = draw.sample_x_z(M.SimRng(seed, M.DATA_SIM), theta)[0]
    draw.close()
    prob = M.HipMuseProblem(xdata, model=model, ntheta=1, N=N)
    g, info = prob.map_and_score_batch(seed, 0, nsims, theta, include_data=True, atol=1e-4, z0_mode=0)
    zh = prob.get_zhat(0, nsims + 1)
    xs = [xdata] + [prob.sample_x_z(M.SimRng(seed, sim), theta)[0] for sim in range(nsims)]
    check_records(model, xs, theta, zh, g, info, 1e-4)     # all 151: the data element, then first to third problems of a cluster
    prob.close()


def test_records_that_did_not_converge_on_the_gradient(gpu, M):
    """smooth at an atol below what rounding lets the gradient reach: the solves end f_converged (or x_converged, or with a
    failed line search); gnorm, f_min and the score must still describe the MAP written out."""
    seen = set()
    for N, theta in ((64, [1.0, 2.0, -0.5]), (601, [1.0, 2.0, 3.0, 0.5])):
        prob = M.HipMuseProblem(None, model="smooth", ntheta=len(theta), N=N)
        seen |= run_map(prob, M, "smooth", np.asarray(theta), None, seed=9, s0=0, nsims=16, atol=1e-15)
        prob.close()
    assert seen - {0}, seen


def test_saved_maps_of_a_muse_run(gpu, M):
    """muse(save_MAPs=True) runs the host loop (the native loop refuses save_MAPs): every iteration's saved data MAP is
    g-converged at its theta and within |g_i| / H_ii of the closed form."""
    N, atol = 3000, 1e-9
    draw = M.HipMuseProblem(None, model="funnel", ntheta=1, N=N)
    x = draw.sample_x_z(M.SimRng(5, M.DATA_SIM), [0.0])[0]
    draw.close()
    prob = M.HipMuseProblem(x, model="funnel", ntheta=1, prior=M.GaussianPrior(0.0, 3.0))
    res = M.muse(prob, [1.0], rng=11, nsims=16, maxsteps=3, theta_rtol=0.0, grad_z_logLike_atol=atol, save_MAPs=True)
    assert len(res.history) >= 2
    for h in res.history:
        th = np.atleast_1d(np.asarray(h["θ"], dtype=np.float64))
        z = np.asarray(h["ẑ_dat"], dtype=np.float64)
        _, g, _, cg = R.objective("funnel", x, z, th)
        gi, gb = np.abs(g).astype(np.float64), float(R.rounding(cg).max())
        assert gi.max() <= atol + gb
        dz = np.abs((z - R.exact_map("funnel", x, th)).astype(np.float64))
        assert (dz <= (gi + gb) / R.diag_hessian("funnel", x, z, th).astype(np.float64)).all()
    prob.close()


# ------------------------------------------------------------------------------------------------ 4. implicit H
@pytest.mark.parametrize("model,N,theta", [("funnel", 64, [0.3]), ("funnel", 4097, [0.3, -0.5, 1.0, 0.2]), ("funnel", 257, [0.4, -0.1]),
                                           ("noise", 4097, [-0.2]), ("noise", 65, [0.5]),
                                           ("smooth", 513, [1.0, 0.5, 1.5]), ("smooth", 4096, [1.0, 2.0]), ("smooth", 5, [1.0])])
def test_implicit_H_against_the_reference(gpu, M, model, N, theta):
    """rtol 1e-6: CG stops at a relative residual of sqrt(eps) (the reference's cg defaults), times cond(A) <= ~50 here."""
    prob = M.HipMuseProblem(None, model=model, ntheta=len(theta), N=N)
    Hs, _ = prob.implicit_H_batch(17, 0, 3, theta, atol=1e-10, cg_maxiter=1000)
    for s in range(3):
        Hh = R.implicit_H(model, N, 17, s, theta).astype(np.float64)
        np.testing.assert_allclose(Hs[s], Hh, rtol=1e-6, atol=1e-6 * np.abs(Hh).max(), err_msg=f"sim {s}")
    prob.close()


@pytest.mark.parametrize("N,theta", [(65, [0.3]), (4097, [0.5, -0.3, 0.2])])
def test_implicit_H_of_the_cubic_header(gpu, M, N, theta):
    prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("cubic"), ntheta=len(theta), N=N)
    Hs, _ = prob.implicit_H_batch(17, 0, 2, theta, atol=1e-10, cg_maxiter=1000)
    for s in range(2):
        x, _ = prob.sample_x_z(M.SimRng(17, s), theta)
        zh, _ = prob.zhat_at_theta(x, np.zeros(N), theta, 1e-10)
        Hh = R.implicit_H("cubic", N, 17, s, theta, zhat_start=zh).astype(np.float64)
        np.testing.assert_allclose(Hs[s], Hh, rtol=1e-6, atol=1e-6 * np.abs(Hh).max(), err_msg=f"sim {s}")
    prob.close()
