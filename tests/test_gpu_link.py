"""-m gpu: the stencil model with a pointwise response behind the operator (muse_set_link; csrc/models.hpp, SmoothLinkModel) against
the longdouble reference tests/link_reference.py -- no oracle in any assertion (the oracle knows nothing of phi).

Shapes, noise and mask are the twin's (tests/test_gpu_noise_weights.py: N = 301, 7001 x 4, 70001 x 4 in both placements of the
search direction, 1500 x 12; the ramp sd in [0.5, 2]; the mask with 0, N - 1, a lane-0 and a lane-63 element and a pair of
neighbours two cluster members own), theta is its theta_of (~ -4), the link (0.25, 0.5): monotone, phi' between ~0.96 and ~1.7
over the draws' range.  The harder case is link_cases.HARD: N = 301, theta = 0, link (0.4, 0.3), where HagerZhang brackets and
bisects in these kernels for the first time.

Bounds (link_reference's docstring derives them): z equals the draw of the SAME context before set_link, byte for byte; x within
dpa(|A| |z|) |A| tol_z + s gen + rounding(cond_x), the twin's bound with phi' carried through it, and exactly 0 where masked;
logLike rtol 1e-12 and grad_z rtol 1e-13 relative to the largest component (the project's stated tolerances), each no tighter than
the reference's own rounding bound; MAPs |zhat - z*|_inf <= 2 atol / lambda with z* Newton's from zhat and lambda the Hessian's
floor (hessian_floor, asserted > 0 at z* and at zhat -- tests/test_link_reference.py holds that the reference alone satisfies it
with room; the harder case uses the dense Hessian's computed smallest eigenvalue); scores within the reference's rounding bound at
the engine's MAP.

test_muse_native_and_host_loop_agree_and_reach_the_reference_root: measured |theta_hat - root| is printed (DESIGN section 3
records it)."""
import numpy as np
import pytest

import hp_reference as R
import link_cases as C
import link_reference as L
import stencil_reference as S
from test_exact_marginal import PRIOR_SIGMA
from test_gpu_noise_weights import SHAPES, STENCILS, VARIANTS, _same, noise_of, theta_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

ATOL = C.ATOL
LINK = C.LINK


def make(M, N, nth, split=0, w=None, x=None, link=LINK, prior=None):
    prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, N=None if x is not None else N, stencil=w, prior=prior)
    if split:
        prob.set_element_split(split)
    info = prob.placement_info()
    sd, mask, marked = noise_of(N, nth, info["threads"], info["workgroups_per_element"])
    prob.set_noise(sd, mask)
    if link is not None:
        prob.set_link(link)
    return prob, sd, mask, marked


def _floor(x, zs, zh, theta, wr, om, link):
    lam = min(L.hessian_floor(x, zs, theta, wr, om, link), L.hessian_floor(x, zh, theta, wr, om, link))
    assert lam > 0, lam
    return lam


# ------------------------------------------------------------------------------------------------ 1. sampler and operators
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth", SHAPES)
def test_sampler_and_operators_against_the_reference(gpu, M, N, nth, w):
    from test_hp_reference import K_GEN
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    prob, sd, mask, _ = make(M, N, nth, w=w, link=None)
    x_plain, z_plain = prob.sample_x_z(M.SimRng(5, 1), theta)
    assert prob.get_link() == ((0.0, 0.0), False)
    prob.set_link(LINK)
    assert prob.get_link() == (LINK, True)
    om, s = L.weights(N, sd, mask)
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    assert z.tobytes() == z_plain.tobytes()                           # the link does not enter z
    assert x.tobytes() != x_plain.tobytes()
    assert np.all(x[~mask] == 0.0) and not np.signbit(x[~mask]).any() and np.all(x[mask] != 0.0)
    xh, zh, cx = L.sample_x_z(N, 5, 1, theta, wr, s, LINK)
    rn = R.normals(5, 1, N)[2].astype(np.float64)
    gen = K_GEN * 2.0 ** -52 * np.maximum(1.0, rn)
    tolz = gen * np.exp(0.5 * theta)[R.blocks(N, nth)] + 4 * R.U * np.abs(zh).astype(np.float64)
    assert (np.abs(z - zh).astype(np.float64) <= tolz).all()
    slope = L._dpa(S.stencil_abs(np.abs(zh) + tolz, wr), LINK).astype(np.float64)     # phi' carried through the twin's bound
    tolx = slope * S.stencil_abs(tolz, wr).astype(np.float64) + s.astype(np.float64) * gen + L.rounding(cx)
    err = np.abs(x - xh).astype(np.float64)
    print("x: largest error / bound", float((err[mask] / tolx[mask]).max()))
    assert (err <= tolx).all()
    # logLike and grad_z at a point away from the MAP, a masked x overwritten on the way
    zz = 0.7 * z + 0.1
    xj = x.copy()
    xj[~mask] = np.resize([np.nan, np.inf, -np.inf, 1e30], int((~mask).sum()))
    f, gz = prob.logLike_and_grad_z_logLike(xj, zz, theta)
    fh, gh, cf, cg = L.objective(x, zz, theta, wr, om, LINK)
    gmax = float(np.abs(gh).max())
    print("logLike rel", abs(-f - float(fh)) / abs(float(fh)), "grad rel", float(np.abs(-gz - gh).max() / gmax),
          "bounds rel", float(L.rounding(cf)) / abs(float(fh)), float(L.rounding(cg).max()) / gmax)
    assert abs(-f - fh) <= max(1e-12 * abs(float(fh)), float(L.rounding(cf)))
    assert (np.abs(-gz - gh).astype(np.float64) <= np.maximum(1e-13 * gmax, L.rounding(cg))).all()
    sc, cs = L.score(x, zz, theta)
    assert (np.abs(prob.grad_theta_logLike(xj, zz, theta) - sc) <= R.rounding(cs)).all()
    zs_e, rec = prob.zhat_at_theta(xj, np.zeros(N), theta, ATOL)
    assert rec["status"] == 0
    zs = L.exact_map(x, theta, wr, om, LINK, z_start=zs_e)
    lam = _floor(x, zs, zs_e, theta, wr, om, LINK)
    assert np.abs(zs_e - zs).astype(np.float64).max() <= 2 * ATOL / lam
    prob.close()


# ------------------------------------------------------------------------------------------------ 2. maps
def _check_records(wr, om, xs, theta, zh, g, info, ctx, link=LINK):
    for e in range(len(info)):
        c = (ctx, e, int(info["status"][e]))
        assert info["status"][e] == 0, c
        f, gz, cf, cg = L.objective(xs[e], zh[e], theta, wr, om, link)
        gi, gb = np.abs(gz).astype(np.float64), float(L.rounding(cg).max())
        assert gi.max() <= ATOL + gb, (c, gi.max())
        assert abs(info["gnorm"][e] - gi.max()) <= gb, c
        assert abs(info["f_min"][e] - f) <= L.rounding(cf), c
        sc, cs = L.score(xs[e], zh[e], theta)
        assert (np.abs(g[e] - sc) <= R.rounding(cs)).all(), (c, g[e], sc.astype(np.float64))
        zs = L.exact_map(xs[e], theta, wr, om, link, z_start=zh[e])
        lam = _floor(xs[e], zs, zh[e], theta, wr, om, link)
        dz = np.abs(zh[e] - zs).astype(np.float64).max()
        assert dz <= 2 * ATOL / lam, (c, dz, 2 * ATOL / lam)


@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_maps_against_the_reference_and_their_invariances(gpu, M, N, nth, split, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    draw, sd, mask, _ = make(M, N, nth, split=split, w=w)
    om, _ = L.weights(N, sd, mask)
    xdata = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    nsims = 3
    xs = [xdata] + [draw.sample_x_z(M.SimRng(42, sim), theta)[0] for sim in range(3, 3 + nsims)]
    draw.close()
    prob, _, _, _ = make(M, N, nth, split=split, w=w, x=xdata)
    info_p = prob.placement_info()
    if N == 70001:
        assert info_p["workgroups_per_element"] > 1 and info_p["direction_in_lds"] == (split == 0), info_p
    g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=ATOL)
    zh = prob.get_zhat(0, nsims + 1)
    _check_records(wr, om, xs, theta, zh, g, info, (N, nth, split, w))
    # the link is applied: the same maps without it give other scores
    prob.set_link(None)
    g0, _ = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=ATOL)
    assert g0.tobytes() != g.tobytes()
    prob.set_link(LINK)
    # bit-equal: the placement asked for (S256 / S512 / clusters as muse_set_placement reaches them), the batch's split into
    # launches, the result area, the multi-map launch, a warm restart
    with pytest.raises(M.MuseError):
        prob.set_placement(1)
    for placement in (0, -1):
        prob.set_placement(placement)
        g2, i2 = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=ATOL)
        assert g2.tobytes() == g.tobytes() and i2.tobytes() == info.tobytes(), placement
        assert prob.get_zhat(0, nsims + 1).tobytes() == zh.tobytes(), placement
    for lo, hi in ((3, 4), (4, 6)):
        g2, i2 = prob.map_and_score_batch(42, lo, hi, theta, atol=ATOL)
        assert g2.tobytes() == g[1 + lo - 3:1 + hi - 3].tobytes() and i2.tobytes() == info[1 + lo - 3:1 + hi - 3].tobytes(), (lo, hi)
    for area in (1, 3):
        n = prob.map_and_score_batch_async(42, 3, 3 + nsims, theta, include_data=True, atol=ATOL, result_area=area)
        g2, i2 = prob.batch_wait(n, area)
        assert g2.tobytes() == g.tobytes() and i2.tobytes() == info.tobytes(), area
    if nth <= M._capi.MAX_THETA:
        thetas = np.stack([theta, theta + 0.05])
        n = prob.map_and_score_multi_async(42, 3, 3 + nsims, thetas, include_data=True, atol=ATOL)
        g2, i2 = prob.batch_wait(n, 0)
        assert g2[:nsims + 1].tobytes() == g.tobytes() and i2[:nsims + 1].tobytes() == info.tobytes()
        g3, i3 = prob.map_and_score_batch(42, 3, 3 + nsims, theta + 0.05, include_data=True, atol=ATOL)
        assert g2[nsims + 1:].tobytes() == g3.tobytes() and i2[nsims + 1:].tobytes() == i3.tobytes()
    warm = []
    for _ in range(2):
        prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4)
        gw, iw = prob.map_and_score_batch(42, 3, 3 + nsims, theta + 0.05, include_data=True, atol=ATOL, z0_mode=M.Z0_WARM)
        assert np.all(iw["status"] == 0)
        warm.append((gw.tobytes(), iw.tobytes(), prob.get_zhat(0, nsims + 1).tobytes()))
    assert warm[0] == warm[1]
    prob.close()


# ------------------------------------------------------------------------------------------------ 3. the line search did real work
@pytest.mark.parametrize("k", range(len(C.HARD)))
def test_harder_case_line_search_against_optim_lbfgs(gpu, M, k):
    """Measured on one MI355X (this file's first run): see the printed counts."""
    case = C.HARD[k]
    N, theta, link = case["N"], np.asarray(case["theta"], float), case["link"]
    x, sd, mask, om, s, wr = C.hard_data(case)
    prob = M.HipMuseProblem(None, model="smooth", ntheta=theta.size, N=N, stencil=case["w"], noise_sd=sd, mask=mask)
    _, rq = prob.zhat_at_theta(x, np.zeros(N), theta, ATOL)                # the noise twin on the same data: a quadratic solve
    prob.set_link(link)
    zh, rec = prob.zhat_at_theta(x, np.zeros(N), theta, ATOL)
    prob.close()
    zo, io = C.lbfgs(M, C.hard_problem(case)[1]["exact"], N, ATOL)
    print("engine", int(rec["iterations"]), int(rec["f_calls"]), "optim.lbfgs", io["iterations"], io["f_calls"], "noise twin",
          int(rq["iterations"]), int(rq["f_calls"]))
    assert rec["status"] == 0 and rq["status"] == 0 and io["status"] == 0
    assert rec["f_calls"] > rq["f_calls"]                                   # more evaluations than the quadratic solve takes
    zs = L.exact_map(x, theta, wr, om, link, z_start=zh)
    ev = min(np.linalg.eigvalsh(L.hessian(x, v, theta, wr, om, link).astype(np.float64)).min() for v in (zs, zh))
    assert ev > 0
    assert np.abs(zh - zs).astype(np.float64).max() <= 2 * ATOL / ev
    assert np.abs(zo.numpy() - zs).astype(np.float64).max() <= 2 * ATOL / ev
    assert (int(rec["iterations"]), int(rec["f_calls"])) == (io["iterations"], io["f_calls"])


# ------------------------------------------------------------------------------------------------ 4. the zero link: the bits before
def _everything(M, prob, theta, nsims):
    theta = np.asarray(theta, float)
    out = []
    n = nsims + 1
    g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4, z0_mode=M.Z0_ZERO)
    out += [g, info, prob.get_zhat(0, n)]
    g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta + 0.05, include_data=True, atol=1e-6, z0_mode=M.Z0_WARM)
    out += [g, info, prob.get_zhat(0, n)]
    step = 0.1 * np.ones(theta.size)
    Hs, hinfo = prob.fd_jacobian_batch(42, 0, 2, theta, step, atol=1e-5)
    F, finfo = prob.fd_values_columns(42, 0, 0, 2 * theta.size, theta, np.stack([step, -step], axis=1), atol=1e-5)
    cols, cinfo = prob.fd_jacobian_columns(42, 0, 0, 2 * theta.size, theta, step, atol=1e-5)
    out += [Hs, hinfo, F, finfo, cols, cinfo]
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    f, gz = prob.logLike_and_grad_z_logLike(x, 0.7 * z + 0.1, theta)
    out += [x, z, np.array([f]), gz, prob.grad_theta_logLike(x, 0.7 * z + 0.1, theta)]
    zs, rec = prob.zhat_at_theta(x, np.zeros(prob.N), theta, 1e-6)
    out += [zs, np.atleast_1d(rec)]
    return out


def _trajectory(M, prob, nth):
    out = []
    for native in (True, False):
        res = M.muse(prob, [0.0] * nth, rng=7, nsims=6, maxsteps=3, theta_rtol=1e-12, grad_z_logLike_atol=1e-4, alpha=0.7, native=native)
        out += [np.asarray(res.theta, float)] + [np.asarray(h[key], float) for h in res.history for key in ("θ", "g_like_sims", "g_post′")]
    return out


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_the_zero_link_gives_the_bits_of_the_context_before(gpu, M, N, nth, split, w, noise):
    theta = np.round(np.linspace(-1.0, 1.5, nth), 3)
    draw = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=w)
    x = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    draw.close()
    prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, stencil=w)
    if split:
        prob.set_element_split(split)
    if noise:
        sd, mask, _ = noise_of(N, nth)
        prob.set_noise(sd, mask)
    nsims = 2 if N > 20000 else 4
    traj = N <= 7001 and nth <= M._capi.MAX_THETA
    assert prob.get_link() == ((0.0, 0.0), False)
    base_ops = _everything(M, prob, theta, nsims)
    base = base_ops + (_trajectory(M, prob, nth) if traj else [])
    prob.set_link((0.0, 0.0))
    assert prob.get_link() == ((0.0, 0.0), True) and prob.get_noise()[2] == noise and prob.get_stencil()[1] == (w is not None)
    _same(_everything(M, prob, theta, nsims) + (_trajectory(M, prob, nth) if traj else []), base, "link (0, 0)")
    prob.set_link(LINK)                                                # another link in between leaves nothing behind
    g, _ = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4)
    assert g.tobytes() != base[0].tobytes()
    prob.set_link(None)
    assert prob.get_link() == ((0.0, 0.0), False)
    _same(_everything(M, prob, theta, nsims), base_ops, "set_link(None)")
    prob.close()


# ------------------------------------------------------------------------------------------------ 5. get_H!
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_get_H_finite_differences_and_the_refused_implicit_branch(gpu, M, N, nth, split, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    prob, sd, mask, _ = make(M, N, nth, split=split, w=w)
    om, s = L.weights(N, sd, mask)
    nsim = 2
    before = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)
    zb = prob.get_zhat(0, 2)
    step = 0.02 * (1.0 + np.arange(nth) / (nth + 1.0))
    n = nsim * nth
    Fpm, fi = prob.fd_values_columns(9, 3, 0, n, theta, np.stack([step, -step], axis=1), atol=ATOL)
    assert np.all(fi["status"] == 0)
    want = (-0.5 * Fpm[:, 1] + 0.5 * Fpm[:, 0]) / step[np.arange(n) % nth][:, None]
    cols, ci = prob.fd_jacobian_columns(9, 3, 0, n, theta, step, atol=ATOL)
    assert np.all(ci["status"] == 0) and np.array_equal(cols, want)
    Hs, hi = prob.fd_jacobian_batch(9, 3, 3 + nsim, theta, step, atol=ATOL)
    assert np.all(hi["status"] == 0) and np.array_equal(Hs, want.reshape(nsim, nth, nth).transpose(0, 2, 1))
    # ... and the values are the reference's: the score at theta0, at the exact MAP, of the draw at theta0 +- step e_j
    k, iv = R.blocks(N, nth), np.exp(-theta)
    for j in range(1 if N > 20000 else min(nth, 2)):       # (the large shape: one column, both grid points)
        for gpt, sign in ((0, 1.0), (1, -1.0)):
            tp = theta.copy()
            tp[j] += sign * step[j]
            xq = L.sample_x_z(N, 9, 3, tp, wr, s, LINK)[0].astype(np.float64)
            sc, zs = L.score_at_exact_map(xq, theta, wr, om, LINK)
            lam = L.hessian_floor(xq, zs, theta, wr, om, LINK)
            assert lam > 0
            dz = 2 * ATOL / lam
            _, cs = L.score(xq, zs.astype(np.float64), theta)
            dsc = np.array([iv[b] * (np.abs(zs[k == b]).astype(np.float64).sum() * dz + 0.5 * (k == b).sum() * dz * dz) for b in range(nth)])
            assert (np.abs(Fpm[j, gpt] - sc).astype(np.float64) <= dsc + 4 * R.rounding(cs)).all(), (j, gpt, Fpm[j, gpt], sc.astype(np.float64))
    # the implicit-differentiation branch is refused, with the reason, before any launch
    from museinference_jl_amd.problem import LINK_IMPLICIT_REFUSAL
    with pytest.raises(M.MuseError) as e1:
        prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=ATOL)
    assert LINK_IMPLICIT_REFUSAL in str(e1.value)
    with pytest.raises(M.MuseError) as e2:
        prob.implicit_H_columns(9, 3, 0, nth, theta)
    assert LINK_IMPLICIT_REFUSAL in str(e2.value)
    if nth <= M._capi.MAX_THETA and N <= 7001:
        res = M.MuseResult()
        res.theta = theta.copy()
        with pytest.raises(M.MuseError) as e3:
            M.get_H_(res, prob, theta, rng=9, nsims=2, implicit_diff=True)
        assert LINK_IMPLICIT_REFUSAL in str(e3.value)
    # a map afterwards gives the bytes it gave before
    after = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert prob.get_zhat(0, 2).tobytes() == zb.tobytes()
    prob.close()


# ------------------------------------------------------------------------------------------------ 6. muse()
def test_muse_native_and_host_loop_agree_and_reach_the_reference_root(gpu, M):
    from scipy.optimize import root
    N, nth, nsims, truth, seed = 1000, 2, 32, [1.0, 0.2], 20240
    prior = M.GaussianPrior(0.0, PRIOR_SIGMA)
    draw, sd, mask, _ = make(M, N, nth)
    x = draw.sample_x_z(M.SimRng(99, M.DATA_SIM), truth)[0]
    draw.close()
    om, s = L.weights(N, sd, mask)
    prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, prior=prior, noise_sd=sd, mask=mask, link=LINK)
    results = []
    for native in (True, False):
        # (atol 1e-5: at theta ~ 1 this link's Hessian has a condition number of a few thousand and f ~ 800, and a solve cannot
        #  push |g| below ~1e-6 before f stops changing in fp64 -- at the twin's 1e-7 every MAP ends F_CONVERGED on rounding noise
        #  and the two loops, whose theta differ in the last bit, drift 2e-9 apart; alpha 0.7, the reference's default: full steps
        #  can settle into a two-cycle around the root of a non-linear model)
        res = M.muse(prob, [0.0] * nth, rng=seed, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-5, alpha=0.7,
                     get_covariance=True, native=native)
        results.append(res)
    prob.close()
    t_native, t_host = (np.asarray(r.theta, float) for r in results)
    np.testing.assert_allclose(t_host, t_native, rtol=1e-9, atol=1e-12)
    starts = {}
    fun = lambda t: L.muse_gradient(x, t, S.BUILTIN, om, s, LINK, seed, nsims, starts) - np.asarray(t) / PRIOR_SIGMA ** 2
    sol = root(fun, t_native, tol=1e-10)
    assert sol.success, sol.message
    sigma = np.sqrt(np.diag(np.atleast_2d(results[0].Sigma)))
    for name, t in (("native", t_native), ("host", t_host)):
        dev = np.abs(t - sol.x) / (sigma / np.sqrt(nsims))
        print("muse", name, "theta", t, "root", sol.x, "|theta - root|", np.abs(t - sol.x), "in sigma / sqrt(nsims)", dev, "sigma", sigma)
        assert np.all(dev < 4.0), (t, sol.x, dev)


# ------------------------------------------------------------------------------------------------ 7. the mask is real
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_masked_data_never_enters(gpu, M, N, nth, split):
    theta = theta_of(nth)
    draw, sd, mask, _ = make(M, N, nth, split=split)
    x = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    draw.close()
    out = []
    for junk in (None, 1e30, np.nan, np.inf, -np.inf):
        xd = x.copy()
        if junk is not None:
            xd[~mask] = junk
        prob, _, _, _ = make(M, N, nth, split=split, x=xd)
        g, info = prob.map_and_score_batch(42, 0, 1, theta, include_data=True, atol=ATOL)
        out.append((g[0].tobytes(), info[0].tobytes(), prob.get_zhat(0, 1).tobytes()))
        assert info["status"][0] == 0
        prob.close()
    assert all(o == out[0] for o in out[1:])


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_context_as_it_was(gpu, M):
    for model in ("funnel", "noise"):
        p = M.HipMuseProblem(None, model=model, ntheta=1, N=64)
        g0, _ = p.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
        for call in (lambda: p.set_link(LINK), lambda: p.set_link(None), lambda: p.get_link()):
            with pytest.raises(M.MuseError):
                call()
        g1, _ = p.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
        assert g0.tobytes() == g1.tobytes()
        p.close()
    with pytest.raises(M.MuseError):
        M.HipMuseProblem(None, model="funnel", ntheta=1, N=64, link=LINK)
    u = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("cubic"), ntheta=1, N=64)
    g0, _ = u.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
    with pytest.raises(M.MuseError):
        u.set_link(LINK)
    g1, _ = u.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
    assert g0.tobytes() == g1.tobytes()
    u.close()
    N, nth = 64, 2
    p = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, link=LINK)
    assert p.get_link() == (LINK, True) and not p.get_noise()[2]           # (a link without a noise map: unit vectors of its own)
    g0, i0 = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    for bad in ((np.nan, 0.5), (0.25, np.inf), (-np.inf, 0.0), (np.nan, np.nan)):
        with pytest.raises(M.MuseError):
            p.set_link(bad)
        assert p.get_link() == (LINK, True)                                # the context keeps the link it had
    with pytest.raises(ValueError):
        p.set_link((0.1, 0.2, 0.3))
    g1, i1 = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    assert g0.tobytes() == g1.tobytes() and i0.tobytes() == i1.tobytes()
    p.set_link(None)
    g2, _ = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    q = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N)
    g3, _ = q.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    assert g2.tobytes() == g3.tobytes() and g2.tobytes() != g0.tobytes()
    p.close()
    q.close()
