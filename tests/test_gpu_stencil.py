"""-m gpu: the stencil model with run-time weights (muse_set_stencil; csrc/models.hpp, SmoothTapsModel).

5.  at (1/2, 1/4) the run-time kernels give the built-in's BITS (scores, MAPs, records, both get_H! branches, a muse() trajectory),
    and set_stencil(None) afterwards launches the built-in kernels again;
6.  other weights against the longdouble reference (tests/stencil_reference.py) within its rounding bounds, the MAP within
    atol / lambda_min of the dense solve, and independent of the element split's placement;
7.  (1, 0) is the funnel;
8.  muse(get_covariance=True) against the exact posterior of the circulant Gaussian model (test_exact_marginal.py's criteria);
9.  both get_H! branches per simulation against the dense longdouble H, and at the exact mode against the expected information;
10. refusals.
No oracle in any assertion."""
import numpy as np
import pytest
from scipy.optimize import brentq

import hp_reference as R
import stencil_reference as S
from test_exact_marginal import PRIOR_SIGMA

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

WEIGHTS = [(0.7, 0.15), (0.6, -0.2), (0.0, 0.5), (1.0, 0.0)]


def _lin(n, lo=-1.0, hi=1.5):
    return list(np.round(np.linspace(lo, hi, n), 3))


def _data(M, N, theta, w=None, seed=77):
    draw = M.HipMuseProblem(None, model="smooth", ntheta=len(theta), N=N, stencil=w)
    x = draw.sample_x_z(M.SimRng(seed, M.DATA_SIM), theta)[0]
    draw.close()
    return x


# ------------------------------------------------------------------------------------------------ 5. the same bits
def _everything(M, prob, theta, nsims, native):
    """What a context computes, as a list of arrays: cold map, warm map, FD Jacobian, implicit H, a muse() trajectory."""
    theta = np.asarray(theta, float)
    out = []
    n = nsims + 1
    g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4, z0_mode=M.Z0_ZERO)
    out += [g, info, prob.get_zhat(0, n)]
    g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta + 0.05, include_data=True, atol=1e-6, z0_mode=M.Z0_WARM)
    out += [g, info, prob.get_zhat(0, n)]
    Hs, hinfo = prob.fd_jacobian_batch(42, 0, 2, theta, 0.1 * np.ones(theta.size), atol=1e-5)
    out += [Hs, hinfo]
    Hi, its = prob.implicit_H_batch(42, 0, 2, theta, atol=1e-6)
    out += [Hi, its]
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    f, gz = prob.logLike_and_grad_z_logLike(x, 0.7 * z + 0.1, theta)
    out += [x, z, np.array([f]), gz, prob.grad_theta_logLike(x, 0.7 * z + 0.1, theta)]
    # (more than MAX_THETA components: the native loops refuse them, the Python loop over the batched maps runs)
    res = M.muse(prob, theta, rng=11, nsims=nsims, maxsteps=3, theta_rtol=0.0, grad_z_logLike_atol=1e-5, native=native)
    out += [np.asarray(res.theta)] + [np.asarray(h["θ"], dtype=np.float64) for h in res.history]
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), (what, k)


@pytest.mark.parametrize("N,nth,split", [(4096, 1, 0), (4096, 4, 0), (4096, 12, 0), (100000, 1, 0), (100000, 4, 8), (100000, 12, 0),
                                         (100000, 12, 8), (4097, 4, 0), (65537, 1, 0), (5, 1, 0), (300, 12, 0)])
def test_builtin_weights_give_the_builtin_bits(gpu, M, N, nth, split):
    theta = _lin(nth)
    x = _data(M, N, theta)
    nsims = 3 if N > 20000 else 6

    def make():
        p = M.HipMuseProblem(x, model="smooth", ntheta=nth, prior=M.GaussianPrior(0.0, 3.0))
        if split:
            p.set_element_split(split)
        return p
    native = nth <= M._capi.MAX_THETA
    ref = make()
    assert ref.get_stencil() == ((0.5, 0.25), False)
    base = _everything(M, ref, theta, nsims, native)
    ref.close()
    prob = make()
    prob.set_stencil((0.5, 0.25))
    assert prob.get_stencil() == ((0.5, 0.25), True)
    if N == 100000:   # both placements of the search direction are what this case is for
        assert prob.placement_info()["direction_in_lds"] == (split == 0)
    _same(_everything(M, prob, theta, nsims, native), base, "run-time weights (1/2, 1/4)")
    prob.set_stencil((0.6, -0.2))       # other weights in between leave nothing behind
    prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=1e-4)
    prob.set_stencil(None)
    assert prob.get_stencil() == ((0.5, 0.25), False)
    _same(_everything(M, prob, theta, nsims, native), base, "set_stencil(None)")
    prob.close()


# ------------------------------------------------------------------------------------------------ 6. other weights
def _check_records(w, xs, theta, zh, g, info, atol, ctx):
    """Every record against the MAP the kernel wrote out: gradient <= atol + rounding for g_converged, gnorm, f_min and score at
    the engine's own zhat within the reference's bounds; N <= 400: |zhat - z*|_inf <= (atol + rounding) / min_k e^{-theta_k}."""
    lam = float(np.exp(-np.max(theta)))
    for e in range(len(info)):
        c = (ctx, e, int(info["status"][e]))
        f, gz, cf, cg = S.objective(xs[e], zh[e], theta, w)
        gi, gb = np.abs(gz).astype(np.float64), float(R.rounding(cg).max())
        assert info["status"][e] == 0, c            # (atol is far above what rounding lets the gradient reach)
        assert gi.max() <= atol + gb, (c, gi.max())
        assert abs(info["gnorm"][e] - gi.max()) <= gb, c
        assert abs(info["f_min"][e] - f) <= R.rounding(cf), c
        s, cs = S.score(xs[e], zh[e], theta)
        assert (np.abs(g[e] - s) <= R.rounding(cs)).all(), (c, g[e], s.astype(np.float64))
        if xs[e].size <= 400:
            dz = np.abs(zh[e] - S.exact_map(xs[e], theta, w)).astype(np.float64).max()
            # zhat - z* = H^-1 g, H = A^T A + diag(e^-theta) with smallest eigenvalue >= min_k e^-theta_k
            assert dz <= (atol + gb) / lam, (c, dz, (atol + gb) / lam)


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("N,nth", [(5, 1), (257, 3), (400, 12), (4097, 1), (4096, 3), (3001, 12), (66001, 3)])
def test_operators_and_maps_against_the_reference(gpu, M, w, N, nth):
    theta = np.asarray(_lin(nth))
    prob = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=w)
    # per-simulation operators
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    xh, zh_, cx = S.sample_x_z(N, 5, 1, theta, w)
    from test_hp_reference import K_GEN
    rn = R.normals(5, 1, N)[2].astype(np.float64)
    sd = np.exp(0.5 * theta)[R.blocks(N, nth)]
    gen = K_GEN * 2.0 ** -52 * np.maximum(1.0, rn)                   # (test_hp_reference.py: the generator's committed bound)
    tolz = gen * sd + 4 * R.U * np.abs(zh_).astype(np.float64)       # ... times sd; the exp within an ulp, the product rounded
    assert (np.abs(z - zh_).astype(np.float64) <= tolz).all()
    # x = A z + n2: the draws' errors through |A|, the noise normal's, and the expression's own rounding
    tolx = S.stencil_abs(tolz, w).astype(np.float64) + gen + R.rounding(cx)
    assert (np.abs(x - xh).astype(np.float64) <= tolx).all()
    zz = 0.7 * z + 0.1
    f, gz = prob.logLike_and_grad_z_logLike(x, zz, theta)
    fh, gh, cf, cg = S.objective(x, zz, theta, w)
    assert abs(-f - fh) <= R.rounding(cf)
    assert (np.abs(-gz - gh) <= R.rounding(cg)).all()
    s, cs = S.score(x, zz, theta)
    assert (np.abs(prob.grad_theta_logLike(x, zz, theta) - s) <= R.rounding(cs)).all()
    zs, _ = prob.zhat_at_theta(x, np.zeros(N), theta, 1e-6)
    _, g1, _, cg1 = S.objective(x, zs, theta, w)
    assert np.abs(g1).max() <= 1e-6 + float(R.rounding(cg1).max())
    prob.close()
    # batched maps, data element included: cold, from the truth, warm at a tighter tolerance
    xdata = _data(M, N, theta, w)
    prob = M.HipMuseProblem(xdata, model="smooth", ntheta=nth, stencil=w)
    nsims = 3 if N > 20000 else 6
    xs = [xdata] + [prob.sample_x_z(M.SimRng(42, sim), theta)[0] for sim in range(3, 3 + nsims)]
    for z0_mode, th, atol in ((M.Z0_ZERO, theta, 1e-4), (M.Z0_TRUE, theta, 1e-4), (M.Z0_WARM, theta + 0.05, 1e-7)):
        if th is not theta:
            xs = [xdata] + [prob.sample_x_z(M.SimRng(42, sim), th)[0] for sim in range(3, 3 + nsims)]
        g, info = prob.map_and_score_batch(42, 3, 3 + nsims, th, include_data=True, atol=atol, z0_mode=z0_mode)
        _check_records(w, xs, th, prob.get_zhat(0, nsims + 1), g, info, atol, (w, N, nth, z0_mode))
    # several maps in one launch (nth <= 8: the big tier carries one map per launch)
    if nth <= M._capi.MAX_THETA:
        thetas = np.stack([theta, theta + 0.3])
        n = prob.map_and_score_multi_async(9, 0, nsims, thetas, atol=1e-5)
        g, info = prob.batch_wait(n, 0)
        zh = prob.get_zhat(0, n)
        for m, th in enumerate(thetas):
            rows = slice(m * nsims, (m + 1) * nsims)
            _check_records(w, [prob.sample_x_z(M.SimRng(9, sim), th)[0] for sim in range(nsims)], th, zh[rows], g[rows], info[rows], 1e-5, ("multi", m))
    prob.close()


@pytest.mark.parametrize("w", [(0.7, 0.15), (0.6, -0.2)])
def test_results_do_not_depend_on_the_batch_or_the_grid(gpu, M, w):
    """"A result does not depend on placement or element split, bitwise, as for the built-in" -- read as what the built-in model
    guarantees (include/muse_hip.h, muse_set_element_split; test_element_split_vs_oracle_and_invariances): an element's result is a
    function of (seed, sim, theta, N, split), bitwise independent of which launch, how many problems or which workgroup carried it
    (single workgroups, clusters with the direction in LDS, clusters without) and of the storage policy asked for (the stencil
    model streams whatever is asked); the split changes the summation tree, so across splits the scores agree to rtol 1e-12, and
    set_element_split(0) afterwards restores the unsplit bits."""
    for N, nth in ((4097, 3), (100000, 2)):
        theta = _lin(nth)
        prob = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=w)
        g_all, i_all = prob.map_and_score_batch(3, 0, 12, theta, atol=1e-5)
        z_all = prob.get_zhat(0, 12)
        for lo, hi in ((0, 5), (5, 12), (7, 8)):
            g, i = prob.map_and_score_batch(3, lo, hi, theta, atol=1e-5)
            assert g.tobytes() == g_all[lo:hi].tobytes() and i.tobytes() == i_all[lo:hi].tobytes()
            assert prob.get_zhat(0, hi - lo).tobytes() == z_all[lo:hi].tobytes()
        prob.set_placement(0)       # streaming asked for explicitly: the same launches
        g, i = prob.map_and_score_batch(3, 0, 12, theta, atol=1e-5)
        assert g.tobytes() == g_all.tobytes() and i.tobytes() == i_all.tobytes()
        prob.set_placement(-1)
        for split in (2, 8):
            prob.set_element_split(split)
            gs, is_ = prob.map_and_score_batch(3, 0, 12, theta, atol=1e-5)
            prob.set_element_split(0)
            # (the built-in's test: elements whose solve took the same path -- the same iteration and evaluation counts)
            same = (is_["iterations"] == i_all["iterations"]) & (is_["f_calls"] == i_all["f_calls"])
            assert same.mean() >= 0.5, (split, same)
            np.testing.assert_allclose(gs[same], g_all[same], rtol=1e-12)
        g, i = prob.map_and_score_batch(3, 0, 12, theta, atol=1e-5)      # ... and the unsplit bits are back
        assert g.tobytes() == g_all.tobytes() and i.tobytes() == i_all.tobytes()
        prob.close()
    # a split of 8 at N = 10^5 leaves no room for the search direction in LDS: the other cluster kernel, the same property
    prob = M.HipMuseProblem(None, model="smooth", ntheta=2, N=100000, stencil=w)
    prob.set_element_split(8)
    assert not prob.placement_info()["direction_in_lds"]
    g_all, _ = prob.map_and_score_batch(3, 0, 6, _lin(2), atol=1e-5)
    g, _ = prob.map_and_score_batch(3, 2, 5, _lin(2), atol=1e-5)
    assert g.tobytes() == g_all[2:5].tobytes()
    prob.close()


# ------------------------------------------------------------------------------------------------ 7. (1, 0) is the funnel
@pytest.mark.parametrize("N,nth", [(400, 3), (4097, 1), (100000, 4)])
def test_identity_weights_are_the_funnel(gpu, M, N, nth):
    """x = z + n: the same model, other operation order (the stencil's r = x - fma(0, zl + zr, 1 z), g = iv z - fma(0, ., 1 r)).
    Both MAPs are within (atol + rounding) / min_k e^-theta_k of z* = x / (1 + e^-theta) (the bound of the maps against the reference
    above), the scores within the resulting |d score| <= iv (|z| dz + dz^2 / 2) summed over the block, plus their rounding bounds."""
    theta, atol = np.asarray(_lin(nth)), 1e-8
    ps = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=(1.0, 0.0))
    pf = M.HipMuseProblem(None, model="funnel", ntheta=nth, N=N)
    nsims = 4
    gs, infs = ps.map_and_score_batch(21, 0, nsims, theta, atol=atol)
    gf, inff = pf.map_and_score_batch(21, 0, nsims, theta, atol=atol)
    zs, zf = ps.get_zhat(0, nsims), pf.get_zhat(0, nsims)
    k, iv, lam = R.blocks(N, nth), np.exp(-theta), float(np.exp(-np.max(theta)))
    for e in range(nsims):
        xs_, zt = ps.sample_x_z(M.SimRng(21, e), theta)
        xf_, _ = pf.sample_x_z(M.SimRng(21, e), theta)
        assert np.abs(xs_ - xf_).max() <= 4 * R.U * np.abs(xf_).max()       # z + n2 against fma(0, ., 1 z) + n2: the same sum
        _, _, _, cg = S.objective(xs_, zs[e], theta, (1.0, 0.0))
        dz = 2 * (atol + float(R.rounding(cg).max())) / lam       # both MAPs within half of this of z*
        assert np.abs(zs[e] - zf[e]).max() <= dz, (e, np.abs(zs[e] - zf[e]).max(), dz)
        _, cs = S.score(xs_, zs[e], theta)
        ds = np.array([iv[b] * (np.abs(zf[e][k == b]).sum() * dz + 0.5 * (k == b).sum() * dz * dz) for b in range(nth)])
        assert (np.abs(gs[e] - gf[e]) <= ds + 2 * R.rounding(cs)).all(), (e, gs[e], gf[e])
    ps.close()
    pf.close()


# ------------------------------------------------------------------------------------------------ 8. the whole path
def exact_stencil(x, w):
    """test_exact_marginal.exact_smooth with a_q = w0 + 2 w1 cos(2 pi q / N)."""
    N = x.size
    a2 = (w[0] + 2 * w[1] * np.cos(2 * np.pi * np.arange(N) / N)) ** 2
    p = np.abs(np.fft.fft(x)) ** 2 / N
    f = lambda t: 0.5 * np.sum(np.exp(t) * a2 * (p - (1 + np.exp(t) * a2)) / (1 + np.exp(t) * a2) ** 2) - t / PRIOR_SIGMA ** 2
    mode = brentq(f, -8.0, 8.0, xtol=1e-13)
    u = np.exp(mode) * a2 / (1 + np.exp(mode) * a2)
    return np.array([mode]), np.array([1.0 / np.sqrt(0.5 * np.sum(u ** 2) + 1.0 / PRIOR_SIGMA ** 2)])


def _check_marginal(M, prob, x, w, nsims, atol, native):
    mode, sigma = exact_stencil(x, w)
    res = M.muse(prob, [0.0], rng=20240, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=atol, alpha=1.0,
                 get_covariance=True, native=native)
    dev = np.abs(np.asarray(res.theta) - mode) / (sigma / np.sqrt(nsims))
    print("exact marginal", w, x.size, native, "theta", res.theta, "mode", mode, "dev", dev)
    assert np.all(dev < 4.0), (res.theta, mode, dev)            # test_exact_marginal.check's first criterion
    got = np.sqrt(np.diag(np.atleast_2d(res.Sigma)))
    print("  sigma", got, sigma)
    assert np.all(np.abs(got / sigma - 1.0) < 5.0 * 0.5 * np.sqrt(2.0 / (nsims - 1)) + 0.02), (got, sigma)     # ... and its second
    return res


@pytest.mark.parametrize("w", [(0.7, 0.15), (0.6, -0.2)])
@pytest.mark.parametrize("N,truth,nsims", [(4096, [1.0], 256), (100000, [2.0], 64)])
def test_muse_against_the_exact_marginal_posterior(gpu, M, w, N, truth, nsims):
    x = _data(M, N, truth, w, seed=99)
    prob = M.HipMuseProblem(x, model="smooth", ntheta=1, prior=M.GaussianPrior(0.0, PRIOR_SIGMA), stencil=w)
    res = _check_marginal(M, prob, x, w, nsims, 1e-7, True)
    res2 = _check_marginal(M, prob, x, w, nsims, 1e-7, False)
    np.testing.assert_allclose(res2.theta, res.theta, rtol=1e-9, atol=1e-12)
    prob.close()


# ------------------------------------------------------------------------------------------------ 9. both get_H! branches
@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("N,theta", [(64, [0.3]), (257, [0.4, -0.1, 1.0]), (400, _lin(12, -0.5, 1.0))])
def test_get_H_branches_against_the_dense_H(gpu, M, w, N, theta):
    """Per simulation, against H_dense (stencil_reference.implicit_H at the exact MAP).

    Implicit: H_ij = -sum_{block i} iv_i zhat v_j.  (a) CG stops at |r| <= sqrt(eps) |b|, so |v - v*|_2 <= |Hess^-1|_2 |r| <=
    kappa sqrt(eps) |v*|_2 with kappa = lambda_max / lambda_min, lambda_max <= max_q a_q^2 + max_k e^-theta_k, lambda_min >= min_q
    a_q^2 + min_k e^-theta_k (Weyl); (b) zhat is within dz = sqrt(N) (atol + rounding) / lambda_min of the exact MAP (point 6);
    (c) the sum's fp64 rounding, C_ROUND 2^-53 sqrt(n) sum |terms|.  By Cauchy-Schwarz over the block:
        |dH_ij| <= iv_i (|zhat_i|_2 kappa sqrt(eps) |v*_j|_2 + dz |v*_j|_1) (1 + kappa sqrt(eps)) + rounding.
    Finite differences (central, step h): each of the two scores is the reference's at the engine's own MAP within its rounding
    bound, and that MAP within dz of the exact one: |d score_i| <= iv_i (|z*_i|_1 dz + n_i dz^2 / 2); so
        |FD_ij - FD*_ij| <= (2 (d score_i + rounding_i)) / (2 h)
    with FD* the same difference of exact-MAP longdouble scores, whose own distance to H_dense (the truncation, O(h^2)) is
    evaluated from the reference and added."""
    theta = np.asarray(theta, float)
    nth, nsim, atol, h = theta.size, 2, 1e-10, 0.05
    prob = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=w)
    Hi, its = prob.implicit_H_batch(17, 0, nsim, theta, atol=atol, cg_maxiter=1000)
    Hf, _ = prob.fd_jacobian_batch(17, 0, nsim, theta, h * np.ones(nth), atol=atol, fid_mode=0)
    k, iv = R.blocks(N, nth), np.exp(-theta)
    aq2 = S.a_q(N, w).astype(np.float64) ** 2
    lam_min, lam_max = aq2.min() + iv.min(), aq2.max() + iv.max()
    kse = lam_max / lam_min * np.sqrt(np.finfo(float).eps)
    for s in range(nsim):
        Hd = S.implicit_H(N, 17, s, theta, w)
        x, zt, _ = S.sample_x_z(N, 17, s, theta, w)
        L = S.cholesky(S.hessian(N, theta, w))
        zs = S.chol_solve(L, S.stencil(x, w))
        _, _, _, cg = S.objective(x.astype(np.float64), zs.astype(np.float64), theta, w)
        dz = np.sqrt(N) * (atol + float(R.rounding(cg).max())) / lam_min
        for j in range(nth):
            v = np.abs(S.chol_solve(L, S.stencil(S.stencil(R.LD(0.5) * zt * (k == j), w), w))).astype(np.float64)
            for i in range(nth):
                m = k == i
                za = np.abs(zs[m]).astype(np.float64)
                terms = iv[i] * za * v[m]
                bound = iv[i] * (np.linalg.norm(za) * kse * np.linalg.norm(v) + dz * v[m].sum()) * (1 + kse) \
                    + R.C_ROUND * R.U * np.sqrt(m.sum()) * terms.sum()
                assert abs(Hi[s, i, j] - float(Hd[i, j])) <= bound, ("implicit", w, s, i, j, Hi[s, i, j], float(Hd[i, j]), bound)
            # finite differences of column j
            tp, tm = theta.copy(), theta.copy()
            tp[j] += h
            tm[j] -= h
            sp, zp = S.score_at_exact_map(N, 17, s, tp, theta, w)
            sm, zm = S.score_at_exact_map(N, 17, s, tm, theta, w)
            fd_ref = (sp - sm) / R.LD(2 * h)
            for i in range(nth):
                m = k == i
                dsc = sum(iv[i] * (np.abs(zq[m]).astype(np.float64).sum() * dz + 0.5 * m.sum() * dz * dz) for zq in (zp, zm))
                rnd = sum(float(R.rounding(S.score(x.astype(np.float64), zq.astype(np.float64), theta)[1][i])) for zq in (zp, zm))
                bound = (dsc + rnd) / (2 * h) + abs(float(fd_ref[i] - Hd[i, j]))
                assert abs(Hf[s, i, j] - float(Hd[i, j])) <= bound, ("fd", w, s, i, j, Hf[s, i, j], float(Hd[i, j]), bound)
    prob.close()


@pytest.mark.parametrize("w", [(0.7, 0.15), (0.6, -0.2)])
def test_both_get_H_branches_return_the_expected_information(gpu, M, w):
    """At the exact posterior mode, N = 10^4: both branches equal 1/2 sum_q (e^theta a_q^2 / (1 + e^theta a_q^2))^2 to the 1 % of
    test_both_get_H_branches_return_the_exact_information_on_hip."""
    N = 10000
    x = _data(M, N, [1.0], w, seed=99)
    mode, sigma = exact_stencil(x, w)
    F = S.expected_information(N, mode[0], w)
    prob = M.HipMuseProblem(x, model="smooth", ntheta=1, prior=M.GaussianPrior(0.0, PRIOR_SIGMA), stencil=w)
    for kw in (dict(step=0.1 * sigma), dict(implicit_diff=True)):
        res = M.MuseResult()
        res.theta = mode.copy()
        M.get_H_(res, prob, mode, rng=7, nsims=64, grad_z_logLike_atol=1e-6, **kw)
        print("expected information", w, kw, np.atleast_2d(res.H), F)
        np.testing.assert_allclose(np.diag(np.atleast_2d(res.H)), [F], rtol=1e-2, err_msg=str(kw))
    prob.close()


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_leave_the_context_usable(gpu, M):
    for model in ("funnel", "noise"):
        p = M.HipMuseProblem(None, model=model, ntheta=1, N=64)
        g0, _ = p.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
        with pytest.raises(M.MuseError):
            p.set_stencil((0.7, 0.15))
        with pytest.raises(M.MuseError):
            p.set_stencil(None)
        with pytest.raises(M.MuseError):
            p.get_stencil()
        g1, _ = p.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
        assert g0.tobytes() == g1.tobytes()
        p.close()
    with pytest.raises(M.MuseError):
        M.HipMuseProblem(None, model="funnel", ntheta=1, N=64, stencil=(0.7, 0.15))
    u = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("cubic"), ntheta=1, N=64)
    g0, _ = u.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
    with pytest.raises(M.MuseError):
        u.set_stencil((0.7, 0.15))
    g1, _ = u.map_and_score_batch(1, 0, 2, [0.3], atol=1e-6)
    assert g0.tobytes() == g1.tobytes()
    u.close()
    p = M.HipMuseProblem(None, model="smooth", ntheta=2, N=64, stencil=(0.7, 0.15))
    g0, _ = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    for bad in ((np.nan, 0.2), (0.5, np.inf), (-np.inf, 0.0)):
        with pytest.raises(M.MuseError):
            p.set_stencil(bad)
        assert p.get_stencil() == ((0.7, 0.15), True)       # the context keeps the operator it had
    g1, _ = p.map_and_score_batch(1, 0, 2, [0.3, 0.1], atol=1e-6)
    assert g0.tobytes() == g1.tobytes()
    p.close()
