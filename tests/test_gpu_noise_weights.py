"""-m gpu: the stencil model with a noise variance per element and a mask (muse_set_noise; csrc/models.hpp, SmoothNoiseModel)
against the longdouble reference tests/noise_reference.py -- no oracle in any assertion (the oracle knows nothing of Omega).

Shapes, the smallest that reach each code path: N = 301 (one trip, the pad element), 7001 x 4 theta (several trips, block
boundaries off wave boundaries), 70001 x 4 theta (clusters, the search direction in LDS and -- under an element split of 4 -- in
HBM, as muse_placement_info reports), 1500 x 12 theta (the big tier).  Noise: a ramp sd in [0.5, 2]; mask: about 5 % of the
elements, among them 0 and N - 1 (the periodic wrap), an element owned by lane 0 and one owned by lane 63 of a wave, and a pair
of neighbours that two workgroups of the cluster own; never a whole theta block (the conditions are asserted on the indices).

theta: components in [-4.04, -3.91], so that e^-theta is in [49, 57] and the Hessian A^T Omega A + diag e^-theta (omega <= 4, |A| <= 1)
has a condition number below 1.1: a solve then reaches atol = 1e-8 before the objective stops changing in fp64 (the reasoning of
test_gpu_fd_highprec.theta_of), and every record must say status 0.

Bounds (noise_reference's docstring derives them): z bit-exact against the fp64 product the kernel forms is not available to a
longdouble reference, so "bit-exact" is held as: z equals the draw of the SAME context before muse_set_noise, byte for byte (the
noise does not enter z), and that draw is within the generator's committed bound of the reference; x within |A| tol_z + s gen +
rounding(cond_x), the bound of test_gpu_stencil with the noise normal scaled by s -- one ulp-scale rounding of the expression plus
the draws' own errors; x exactly 0 where masked.  logLike rtol 1e-12 and grad_z rtol 1e-13 (relative to the largest component):
the project's stated tolerances.  MAPs: |zhat - z*|_inf <= 2 atol / lambda_min.  Scores: the reference's rounding bound at the
engine's MAP.  Implicit H: noise_reference.implicit_H_bound with dz = 2 atol / lambda_min, the max-norm distance its derivation
names.  (At these theta that distance is rigorous, not only asserted: H is strictly diagonally dominant -- the off-diagonal
row sums of A^T Omega A are at most max omega |A|_1 |A|_inf = 4 for both stencils, whose weights sum to 1, against a diagonal of
at least e^-theta >= 49 -- so |H^-1|_inf <= 1 / (49 - 4) (Varah) and |zhat - z*|_inf <= |g|_inf / 45 < 2 atol / 49.)"""
import numpy as np
import pytest

import hp_reference as R
import noise_reference as Q
import stencil_reference as S
from test_exact_marginal import PRIOR_SIGMA

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

ATOL = 1e-8
SHAPES = [(301, 1), (7001, 4), (70001, 4), (1500, 12)]
# (N, ntheta, element split): 70001 in both placements of the search direction
VARIANTS = [(301, 1, 0), (7001, 4, 0), (70001, 4, 0), (70001, 4, 4), (1500, 12, 0)]
STENCILS = [None, (0.3, 0.35)]


def theta_of(nth):
    return np.round(0.1 * (np.linspace(-0.4, 0.9, nth) + 0.013 * np.cos(3.0 * np.arange(nth))) - 4.0, 4)


def noise_of(N, nth, threads=256, csize=1):
    """(sd, mask, marked): the ramp, the mask and the indices the docstring promises, asserted here."""
    sd = np.linspace(0.5, 2.0, N)
    pair_lane = lambda i: (i // 2) % 64
    group = lambda i: ((i // 2) % (csize * threads)) // threads
    lane0, lane63 = 2 * 64, 2 * 127 + 1                 # pair 64 (lane 0 of the second wave), pair 127 (lane 63 of it)
    wa, wb = 2 * threads - 1, 2 * threads               # last element of workgroup 0's first row, first of workgroup 1's
    marked = [0, N - 1, lane0, lane63] + ([wa, wb] if wb < N - 1 else [])
    assert pair_lane(lane0) == 0 and pair_lane(lane63) == 63 and lane63 < N - 1
    if csize > 1:
        assert wb == wa + 1 and group(wa) != group(wb), (group(wa), group(wb))
    mask = np.ones(N, bool)
    mask[marked] = False
    rest = np.setdiff1d(np.arange(N), marked)
    mask[np.random.default_rng(N).choice(rest, size=N // 20 - len(marked), replace=False)] = False
    k = R.blocks(N, nth)
    assert all(mask[k == b].any() for b in range(nth)) and not mask[marked].any()
    assert 0.04 <= (~mask).mean() <= 0.06
    return sd, mask, marked


def make(M, N, nth, split=0, w=None, x=None, noise=True, prior=None):
    prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, N=None if x is not None else N, stencil=w, prior=prior)
    if split:
        prob.set_element_split(split)
    info = prob.placement_info()
    sd, mask, marked = noise_of(N, nth, info["threads"], info["workgroups_per_element"])
    if noise:
        prob.set_noise(sd, mask)
    return prob, sd, mask, marked


# ------------------------------------------------------------------------------------------------ 1. sampler and operators
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth", SHAPES)
def test_sampler_and_operators_against_the_reference(gpu, M, N, nth, w):
    from test_hp_reference import K_GEN
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    prob, sd, mask, _ = make(M, N, nth, w=w, noise=False)
    _, z_plain = prob.sample_x_z(M.SimRng(5, 1), theta)
    prob.set_noise(sd, mask)
    gsd, gmask, rt = prob.get_noise()
    assert rt and np.array_equal(gsd, sd) and np.array_equal(gmask, mask)
    om, s = Q.weights(N, sd, mask)
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    assert z.tobytes() == z_plain.tobytes()                           # the noise does not enter z
    assert np.all(x[~mask] == 0.0) and not np.signbit(x[~mask]).any() and np.all(x[mask] != 0.0)
    xh, zh, cx = Q.sample_x_z(N, 5, 1, theta, wr, s)
    rn = R.normals(5, 1, N)[2].astype(np.float64)
    gen = K_GEN * 2.0 ** -52 * np.maximum(1.0, rn)
    tolz = gen * np.exp(0.5 * theta)[R.blocks(N, nth)] + 4 * R.U * np.abs(zh).astype(np.float64)
    assert (np.abs(z - zh).astype(np.float64) <= tolz).all()
    tolx = S.stencil_abs(tolz, wr).astype(np.float64) + s.astype(np.float64) * gen + R.rounding(cx)
    err = np.abs(x - xh).astype(np.float64)
    print("x: largest error / bound", float((err[mask] / tolx[mask]).max()))
    assert (err <= tolx).all()
    # logLike and grad_z at a point away from the MAP, a masked x overwritten on the way
    zz = 0.7 * z + 0.1
    xj = x.copy()
    xj[~mask] = np.resize([np.nan, np.inf, -np.inf, 1e30], int((~mask).sum()))   # (the usual fills of a masked pixel, by turns)
    f, gz = prob.logLike_and_grad_z_logLike(xj, zz, theta)
    fh, gh, cf, cg = Q.objective(x, zz, theta, wr, om)
    print("logLike rel", abs(-f - float(fh)) / abs(float(fh)), "grad rel", float(np.abs(-gz - gh).max() / np.abs(gh).max()))
    assert abs(-f - fh) <= 1e-12 * abs(fh)
    assert np.abs(-gz - gh).max() <= 1e-13 * np.abs(gh).max()
    assert (np.abs(-gz - gh) <= R.rounding(cg)).all()
    sc, cs = Q.score(x, zz, theta)
    assert (np.abs(prob.grad_theta_logLike(xj, zz, theta) - sc) <= R.rounding(cs)).all()
    zs, _ = prob.zhat_at_theta(xj, np.zeros(N), theta, ATOL)
    lam = float(np.exp(-np.max(theta)))
    assert np.abs(zs - Q.exact_map(x, theta, wr, om)).astype(np.float64).max() <= 2 * ATOL / lam
    prob.close()


# ------------------------------------------------------------------------------------------------ 2. maps
def _check_records(wr, om, xs, theta, zh, g, info, ctx):
    lam = float(np.exp(-np.max(theta)))
    for e in range(len(info)):
        c = (ctx, e, int(info["status"][e]))
        assert info["status"][e] == 0, c
        f, gz, cf, cg = Q.objective(xs[e], zh[e], theta, wr, om)
        gi, gb = np.abs(gz).astype(np.float64), float(R.rounding(cg).max())
        assert gi.max() <= ATOL + gb, (c, gi.max())
        assert abs(info["gnorm"][e] - gi.max()) <= gb, c
        assert abs(info["f_min"][e] - f) <= R.rounding(cf), c
        sc, cs = Q.score(xs[e], zh[e], theta)
        assert (np.abs(g[e] - sc) <= R.rounding(cs)).all(), (c, g[e], sc.astype(np.float64))
        dz = np.abs(zh[e] - Q.exact_map(xs[e], theta, wr, om)).astype(np.float64).max()
        assert dz <= 2 * ATOL / lam, (c, dz, 2 * ATOL / lam)


@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_maps_against_the_reference_and_their_invariances(gpu, M, N, nth, split, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    draw, sd, mask, _ = make(M, N, nth, split=split, w=w)
    om, _ = Q.weights(N, sd, mask)
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
    # bit-equal: the placement asked for, the batch's split into launches, the result area, the multi-map launch.  The stencil
    # model streams whatever is asked: muse_set_placement takes 0 (streaming) and -1 (by N alone) for it and refuses 1 (resident),
    # with or without noise (test_gpu_stencil's placements) -- so every value the call accepts is run, and the refusal is held.
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
    prob.close()


# ------------------------------------------------------------------------------------------------ 3. neutral noise: the parent's bits
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
    out += [Hs, hinfo, F, finfo]
    Hi, its = prob.implicit_H_batch(42, 0, 2, theta, atol=1e-6)
    out += [Hi, its]
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    f, gz = prob.logLike_and_grad_z_logLike(x, 0.7 * z + 0.1, theta)
    out += [x, z, np.array([f]), gz, prob.grad_theta_logLike(x, 0.7 * z + 0.1, theta)]
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, k)


@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_unit_noise_without_a_mask_gives_the_bits_of_the_context_before(gpu, M, N, nth, split, w):
    theta = np.round(np.linspace(-1.0, 1.5, nth), 3)
    draw = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=w)
    x = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    draw.close()
    prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, stencil=w)
    if split:
        prob.set_element_split(split)
    nsims = 2 if N > 20000 else 4
    sd0, m0, rt0 = prob.get_noise()
    assert not rt0 and np.all(sd0 == 1.0) and m0.all()
    base = _everything(M, prob, theta, nsims)
    prob.set_noise(np.ones(N))
    assert prob.get_noise()[2] and prob.get_stencil()[1] == (w is not None)
    _same(_everything(M, prob, theta, nsims), base, "sd = 1, no mask")
    prob.set_noise(1.0, np.ones(N, bool))                              # a scalar sd, an explicit all-observed mask
    _same(_everything(M, prob, theta, nsims)[:3], base[:3], "sd = 1, mask of ones")
    sd, mask, _ = noise_of(N, nth)
    prob.set_noise(sd, mask)                                           # other noise in between leaves nothing behind
    g, _ = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4)
    assert g.tobytes() != base[0].tobytes()
    prob.set_noise(None)
    assert not prob.get_noise()[2]
    _same(_everything(M, prob, theta, nsims), base, "set_noise(None)")
    prob.close()


# ------------------------------------------------------------------------------------------------ 4. get_H!
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_get_H_branches(gpu, M, N, nth, split, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    prob, sd, mask, _ = make(M, N, nth, split=split, w=w)
    om, s = Q.weights(N, sd, mask)
    nsim = 2
    # finite differences: the Jacobian entries are the combination of the raw values, bit for bit
    step = 0.02 * (1.0 + np.arange(nth) / (nth + 1.0))
    n = nsim * nth
    Fpm, fi = prob.fd_values_columns(9, 3, 0, n, theta, np.stack([step, -step], axis=1), atol=ATOL)
    assert np.all(fi["status"] == 0)
    want = (-0.5 * Fpm[:, 1] + 0.5 * Fpm[:, 0]) / step[np.arange(n) % nth][:, None]
    cols, ci = prob.fd_jacobian_columns(9, 3, 0, n, theta, step, atol=ATOL)
    assert np.all(ci["status"] == 0) and np.array_equal(cols, want)
    Hs, hi = prob.fd_jacobian_batch(9, 3, 3 + nsim, theta, step, atol=ATOL)
    assert np.all(hi["status"] == 0) and np.array_equal(Hs, want.reshape(nsim, nth, nth).transpose(0, 2, 1))
    # ... and the values are the reference's: the score at the exact MAP of the draw at theta0 + step e_j, within the distance
    # of the engine's MAP from it carried into the score (noise_reference's docstring) plus the score's rounding
    k, iv, lam = R.blocks(N, nth), np.exp(-theta), float(np.exp(-np.max(theta)))
    dz = 2 * ATOL / lam
    for j in range(min(nth, 2)):
        tp = theta.copy()
        tp[j] += step[j]
        xq = Q.sample_x_z(N, 9, 3, tp, wr, s)[0].astype(np.float64)
        sc, zs = Q.score_at_exact_map(xq, theta, wr, om)
        _, cs = Q.score(xq, zs.astype(np.float64), theta)
        # (x itself carries the draw's error, which moves the score by |d score / d x| dx: below the rounding bound's scale)
        dsc = np.array([iv[b] * (np.abs(zs[k == b]).astype(np.float64).sum() * dz + 0.5 * (k == b).sum() * dz * dz) for b in range(nth)])
        assert (np.abs(Fpm[j, 0] - sc).astype(np.float64) <= dsc + 4 * R.rounding(cs)).all(), (j, Fpm[j, 0], sc.astype(np.float64))
    # implicit differentiation at the default CG tolerance
    Hi, its = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=ATOL, cg_maxiter=200)
    print("CG iterations", its.tolist())
    assert np.all(its >= 2)
    for e in range(nsim):
        Hd, vs, zh = Q.implicit_H(N, 9, 3 + e, theta, wr, om, s)
        bound = Q.implicit_H_bound(theta, wr, om, zh, vs, dz)            # (dz: the max-norm distance, as the bound is derived)
        err = np.abs(Hi[e] - Hd).astype(np.float64)
        print("implicit H: largest error / bound", float((err / bound).max()))
        assert (err <= bound).all(), (e, Hi[e], Hd.astype(np.float64), bound)
    # the columns entry is the batch entry in both imp_split regimes (one column per element; all columns in one element)
    many = 300 if N < 20000 else 40
    if N == 70001 and split:
        many = 0                                                       # (one placement of the large case carries the long launch)
    if many:
        few, _ = prob.implicit_H_batch(11, 2, 5, theta)
        big, ib = prob.implicit_H_batch(11, 0, many, theta)
        colsi, ic = prob.implicit_H_columns(11, 0, 0, many * nth, theta)
        assert np.array_equal(colsi.reshape(many, nth, nth).transpose(0, 2, 1), big) and np.array_equal(ic.reshape(many, nth), ib)
        assert few.tobytes() == big[2:5].tobytes()
    else:
        few, fi_ = prob.implicit_H_batch(11, 2, 5, theta)
        colsi, ic = prob.implicit_H_columns(11, 2, 0, 3 * nth, theta)
        assert np.array_equal(colsi.reshape(3, nth, nth).transpose(0, 2, 1), few) and np.array_equal(ic.reshape(3, nth), fi_)
    prob.close()


# ------------------------------------------------------------------------------------------------ 5. the mask is real
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


# ------------------------------------------------------------------------------------------------ 6. muse() against the exact posterior
def test_muse_against_the_exact_marginal_posterior(gpu, M):
    N, nth, nsims, truth = 4096, 2, 256, [1.0, 0.2]
    prior = M.GaussianPrior(0.0, PRIOR_SIGMA)
    draw, sd, mask, _ = make(M, N, nth)
    x = draw.sample_x_z(M.SimRng(99, M.DATA_SIM), truth)[0]
    draw.close()
    om, _ = Q.weights(N, sd, mask)
    mode, sigma = Q.posterior_mode(x, S.BUILTIN, om, nth, PRIOR_SIGMA)
    assert np.all(np.abs(mode - np.asarray(truth)) / sigma < 4.0)       # (the exact mode is where the data say it is)
    prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, prior=prior, noise_sd=sd, mask=mask)
    thetas = []
    for native in (True, False):
        res = M.muse(prob, [0.0] * nth, rng=20240, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-7, alpha=1.0,
                     get_covariance=True, native=native)
        dev = np.abs(np.asarray(res.theta) - mode) / (sigma / np.sqrt(nsims))
        print("exact marginal: native", native, "theta", res.theta, "mode", mode, "dev", dev)
        assert np.all(dev < 4.0), (res.theta, mode, dev)                # test_exact_marginal.check's first criterion
        got = np.sqrt(np.diag(np.atleast_2d(res.Sigma)))
        print("  sigma", got, sigma)
        assert np.all(np.abs(got / sigma - 1.0) < 5.0 * 0.5 * np.sqrt(2.0 / (nsims - 1)) + 0.02), (got, sigma)     # ... and its second
        thetas.append(np.asarray(res.theta))
    np.testing.assert_allclose(thetas[1], thetas[0], rtol=1e-9, atol=1e-12)
    prob.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_context_as_it_was(gpu, M):
    for model in ("funnel", "noise"):
        p = M.HipMuseProblem(None, model=model, ntheta=1, N=64)
        g0, _ = p.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
        for call in (lambda: p.set_noise(np.ones(64)), lambda: p.set_noise(None), lambda: p.get_noise()):
            with pytest.raises(M.MuseError):
                call()
        g1, _ = p.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
        assert g0.tobytes() == g1.tobytes()
        p.close()
    with pytest.raises(M.MuseError):
        M.HipMuseProblem(None, model="funnel", ntheta=1, N=64, noise_sd=np.ones(64))
    u = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("cubic"), ntheta=1, N=64)
    g0, _ = u.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
    with pytest.raises(M.MuseError):
        u.set_noise(np.ones(64))
    g1, _ = u.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
    assert g0.tobytes() == g1.tobytes()
    u.close()
    N, nth = 64, 2
    sd, mask = np.linspace(0.5, 2.0, N), np.ones(N, bool)
    mask[[0, 5, N - 1]] = False
    p = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, noise_sd=sd, mask=mask)
    g0, i0 = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)

    def bad_cases():
        for v in (np.nan, np.inf, 0.0, -1.0):
            b = sd.copy()
            b[7] = v
            yield b, mask.astype(float)
        for v in (0.5, 2.0, -1.0, np.nan):
            m = mask.astype(float)
            m[9] = v
            yield sd, m
        for blk in range(nth):                                         # a mask that hides a whole theta block
            m = np.ones(N)
            m[R.blocks(N, nth) == blk] = 0.0
            yield sd, m
    for b, m in bad_cases():
        with pytest.raises(M.MuseError):
            p._check(p._lib.muse_set_noise(p._ctx, M._capi.ptr(M._capi.f8(b, N)), M._capi.ptr(M._capi.f8(m, N)), M._capi.MEM_HOST))
        gsd, gm, rt = p.get_noise()
        assert rt and np.array_equal(gsd, sd) and np.array_equal(gm, mask)         # the context keeps the noise it had
    with pytest.raises(ValueError):
        p.set_noise(np.ones(N - 1))
    g1, i1 = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    assert g0.tobytes() == g1.tobytes() and i0.tobytes() == i1.tobytes()
    p.close()
