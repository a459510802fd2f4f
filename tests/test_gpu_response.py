"""-m gpu: a response behind the stencil operator stated by a user's header (include/muse_model.h, MUSE_MODEL_RESPONSE;
csrc/models.hpp, UserResponseModel) -- the two packaged libraries, which build() compiles: nothing is compiled here.

1. The header seam costs nothing: models/poly_response.h restates the built-in cubic link in the built-in's expressions, and a
   context of its library gives the BYTES of the product library's context with set_link on the same data -- every operator, map,
   finite-difference entry and muse() trajectory test_gpu_link's _everything / _trajectory collect -- at link_cases.LINK and at
   (0, 0), where they are also the bytes of the context with the noise map and no link.  models/saturating_response.h at p0 = 0 is
   the identity and gives the noise context's bytes.
2. models/saturating_response.h at response_cases.P0 against the longdouble reference tests/response_reference.py (no oracle): the
   sampler, logLike / grad_z with NaN and inf in masked x, maps with their invariances, the theta = 0 case.
3. The finite-difference get_H!: the raw values are the reference's scores at the exact MAP, the entries agree bytewise.
4. The implicit-differentiation get_H!, which the built-in link context refuses (tests/test_gpu_link.py, unchanged): at (0, 0) the
   noise context's H bytes and CG counts; at LINK and at P0 within response_reference.implicit_H_bound; the keywords.

Shapes, noise, mask and theta are the twins' (tests/test_gpu_noise_weights.py)."""
import numpy as np
import pytest

import hp_reference as R
import link_cases as C
import response_cases as RC
import response_reference as RR
import stencil_reference as S
from test_gpu_link import _everything, _trajectory
from test_gpu_noise_weights import SHAPES, STENCILS, VARIANTS, _same, noise_of, theta_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

ATOL = RC.ATOL
LINK = C.LINK
SAT = RC.SAT


def make(M, name, N, nth, split=0, w=None, x=None, p=None, noise=True, prior=None):
    """A context of the packaged response library `name` -- or, name None, of the product library's "smooth" -- with the twins' noise."""
    model = "smooth" if name is None else M.ResponseModel.packaged(name)
    prob = M.HipMuseProblem(x, model=model, ntheta=nth, N=None if x is not None else N, stencil=w, prior=prior)
    if split:
        prob.set_element_split(split)
    info = prob.placement_info()
    sd, mask, marked = noise_of(N, nth, info["threads"], info["workgroups_per_element"])
    if noise:
        prob.set_noise(sd, mask)
    if p is not None:
        prob.set_link(p)
    return prob, sd, mask, marked


def _floor(x, zs, zh, theta, wr, om, resp):
    lam = min(RR.hessian_floor(x, zs, theta, wr, om, resp), RR.hessian_floor(x, zh, theta, wr, om, resp))
    assert lam > 0, lam
    return lam


# ------------------------------------------------------------------------------------------------ 1. the same bits as the built-in
@pytest.mark.parametrize("p", [LINK, (0.0, 0.0)])
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_poly_response_gives_the_bytes_of_the_builtin_link(gpu, M, N, nth, split, w, p):
    theta = theta_of(nth)
    draw, _, _, _ = make(M, None, N, nth, w=w, p=p)
    x = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    draw.close()
    nsims = 2 if N > 20000 else 4
    traj = N <= 7001 and nth <= M._capi.MAX_THETA
    out = {}
    for name in (None, "poly_response"):
        prob, _, _, _ = make(M, name, N, nth, split=split, w=w, x=x, p=p)
        assert prob.get_link() == (tuple(p), True) and prob.get_noise()[2] and prob.get_stencil()[1] == (w is not None)
        if name is not None:
            with pytest.raises(M.MuseError):
                prob.set_placement(1)
            assert prob.placement_info() == out["info"]
        else:
            out["info"] = prob.placement_info()
        out[name] = _everything(M, prob, theta, nsims) + (_trajectory(M, prob, nth) if traj else [])
        prob.close()
    _same(out["poly_response"], out[None], ("poly_response against set_link", p))
    if p == (0.0, 0.0):                                   # ... which at (0, 0) are the bytes of the context without a link
        prob, _, _, _ = make(M, None, N, nth, split=split, w=w, x=x)
        assert prob.get_link() == ((0.0, 0.0), False)
        base = _everything(M, prob, theta, nsims)
        _same(out["poly_response"][:len(base)], base, "the noise context")
        prob.close()


@pytest.mark.parametrize("N,nth,split", [(301, 1, 0), (70001, 4, 0), (70001, 4, 4)])
def test_saturating_response_at_zero_is_the_noise_context(gpu, M, N, nth, split):
    theta = theta_of(nth)
    draw, _, _, _ = make(M, None, N, nth)
    x = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    draw.close()
    nsims = 2 if N > 20000 else 4
    out = []
    for name, p in ((None, None), ("saturating_response", None), ("saturating_response", (0.0, 7.0))):   # (p1 is not read)
        prob, _, _, _ = make(M, name, N, nth, split=split, x=x, p=p)
        if name is not None:
            assert prob.get_link() == ((0.0, 0.0) if p is None else p, True)     # NULL means (0, 0); run-time always
        out.append(_everything(M, prob, theta, nsims))
        prob.close()
    _same(out[1], out[0], "saturating_response, link never set")
    _same(out[2], out[0], "saturating_response at p0 = 0")


# ------------------------------------------------------------------------------------------------ 2. the saturating response
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth", SHAPES)
def test_saturating_sampler_and_operators_against_the_reference(gpu, M, N, nth, w):
    from test_hp_reference import K_GEN
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    resp = RR.saturating(RC.P0)
    plain, sd, mask, _ = make(M, None, N, nth, w=w)
    x_plain, z_plain = plain.sample_x_z(M.SimRng(5, 1), theta)
    plain.close()
    prob, _, _, _ = make(M, "saturating_response", N, nth, w=w, p=SAT)
    om, s = RR.weights(N, sd, mask)
    x, z = prob.sample_x_z(M.SimRng(5, 1), theta)
    assert z.tobytes() == z_plain.tobytes()                           # the response does not enter z
    assert x.tobytes() != x_plain.tobytes()
    assert np.all(x[~mask] == 0.0) and not np.signbit(x[~mask]).any() and np.all(x[mask] != 0.0)
    xh, zh, cx = RR.sample_x_z(N, 5, 1, theta, wr, s, resp)
    rn = R.normals(5, 1, N)[2].astype(np.float64)
    gen = K_GEN * 2.0 ** -52 * np.maximum(1.0, rn)
    tolz = gen * np.exp(0.5 * theta)[R.blocks(N, nth)] + 4 * R.U * np.abs(zh).astype(np.float64)
    assert (np.abs(z - zh).astype(np.float64) <= tolz).all()
    slope = resp.dpa(S.stencil_abs(np.abs(zh) + tolz, wr)).astype(np.float64)          # phi' carried through the twin's bound
    tolx = slope * S.stencil_abs(tolz, wr).astype(np.float64) + s.astype(np.float64) * gen + RR.rounding(cx, resp)
    err = np.abs(x - xh).astype(np.float64)
    print("x: largest error / bound", float((err[mask] / tolx[mask]).max()))
    assert (err <= tolx).all()
    zz = 0.7 * z + 0.1
    xj = x.copy()
    xj[~mask] = np.resize([np.nan, np.inf, -np.inf, 1e30], int((~mask).sum()))
    f, gz = prob.logLike_and_grad_z_logLike(xj, zz, theta)
    fh, gh, cf, cg = RR.objective(x, zz, theta, wr, om, resp)
    gmax = float(np.abs(gh).max())
    print("logLike rel", abs(-f - float(fh)) / abs(float(fh)), "grad rel", float(np.abs(-gz - gh).max() / gmax),
          "bounds rel", float(RR.rounding(cf, resp)) / abs(float(fh)), float(RR.rounding(cg, resp).max()) / gmax)
    assert abs(-f - fh) <= max(1e-12 * abs(float(fh)), float(RR.rounding(cf, resp)))
    assert (np.abs(-gz - gh).astype(np.float64) <= np.maximum(1e-13 * gmax, RR.rounding(cg, resp))).all()
    sc, cs = RR.score(x, zz, theta)
    assert (np.abs(prob.grad_theta_logLike(xj, zz, theta) - sc) <= R.rounding(cs)).all()
    prob.close()


def _check_records(wr, om, xs, theta, zh, g, info, ctx, resp):
    for e in range(len(info)):
        c = (ctx, e, int(info["status"][e]))
        assert info["status"][e] == 0, c
        f, gz, cf, cg = RR.objective(xs[e], zh[e], theta, wr, om, resp)
        gi, gb = np.abs(gz).astype(np.float64), float(RR.rounding(cg, resp).max())
        assert gi.max() <= ATOL + gb, (c, gi.max())
        assert abs(info["gnorm"][e] - gi.max()) <= gb, c
        assert abs(info["f_min"][e] - f) <= RR.rounding(cf, resp), c
        sc, cs = RR.score(xs[e], zh[e], theta)
        assert (np.abs(g[e] - sc) <= R.rounding(cs)).all(), (c, g[e], sc.astype(np.float64))
        zs = RR.exact_map(xs[e], theta, wr, om, resp, z_start=zh[e])
        lam = _floor(xs[e], zs, zh[e], theta, wr, om, resp)
        dz = np.abs(zh[e] - zs).astype(np.float64).max()
        assert dz <= 2 * ATOL / lam, (c, dz, 2 * ATOL / lam)


@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_saturating_maps_against_the_reference_and_their_invariances(gpu, M, N, nth, split, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    resp = RR.saturating(RC.P0)
    draw, sd, mask, _ = make(M, "saturating_response", N, nth, split=split, w=w, p=SAT)
    om, _ = RR.weights(N, sd, mask)
    xdata = draw.sample_x_z(M.SimRng(77, M.DATA_SIM), theta)[0]
    nsims = 3
    xs = [xdata] + [draw.sample_x_z(M.SimRng(42, sim), theta)[0] for sim in range(3, 3 + nsims)]
    draw.close()
    prob, _, _, _ = make(M, "saturating_response", N, nth, split=split, w=w, x=xdata, p=SAT)
    info_p = prob.placement_info()
    if N == 70001:
        assert info_p["workgroups_per_element"] > 1 and info_p["direction_in_lds"] == (split == 0), info_p
    g, info = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=ATOL)
    zh = prob.get_zhat(0, nsims + 1)
    _check_records(wr, om, xs, theta, zh, g, info, (N, nth, split, w), resp)
    prob.set_link(None)                                                # the response is applied: p = (0, 0) gives other scores
    g0, _ = prob.map_and_score_batch(42, 3, 3 + nsims, theta, include_data=True, atol=ATOL)
    assert g0.tobytes() != g.tobytes()
    prob.set_link(SAT)
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
    # refusals of such a library: constants, and the reason
    with pytest.raises(M.MuseError) as e:
        prob.set_constants(0, np.ones(N))
    assert "noise vectors" in str(e.value)
    prob.close()


def test_theta_zero_case_takes_more_evaluations_than_the_noise_twin(gpu, M):
    case = RC.HARD
    N, theta, p = case["N"], np.asarray(case["theta"], float), case["p"]
    x, sd, mask, om, s, wr = RC.hard_data(case)
    resp = RR.saturating(p[0])
    prob = M.HipMuseProblem(None, model=M.ResponseModel.packaged("saturating_response"), ntheta=1, N=N, noise_sd=sd, mask=mask)
    _, rq = prob.zhat_at_theta(x, np.zeros(N), theta, ATOL)                # p = (0, 0): the noise twin's quadratic solve
    prob.set_link(p)
    zh, rec = prob.zhat_at_theta(x, np.zeros(N), theta, ATOL)
    prob.close()
    print("saturating", int(rec["iterations"]), int(rec["f_calls"]), "noise twin", int(rq["iterations"]), int(rq["f_calls"]))
    assert rec["status"] == 0 and rq["status"] == 0
    assert rec["f_calls"] > rq["f_calls"]
    zs = RR.exact_map(x, theta, wr, om, resp, z_start=zh)
    ev = min(np.linalg.eigvalsh(RR.hessian(x, v, theta, wr, om, resp).astype(np.float64)).min() for v in (zs, zh))
    assert ev > 0
    assert np.abs(zh - zs).astype(np.float64).max() <= 2 * ATOL / ev


# ------------------------------------------------------------------------------------------------ 3. finite-difference get_H!
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth", [(301, 1), (7001, 4)])
def test_saturating_get_H_by_finite_differences(gpu, M, N, nth, w):
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    resp = RR.saturating(RC.P0)
    prob, sd, mask, _ = make(M, "saturating_response", N, nth, w=w, p=SAT)
    om, s = RR.weights(N, sd, mask)
    nsim = 2
    step = 0.02 * (1.0 + np.arange(nth) / (nth + 1.0))
    n = nsim * nth
    Fpm, fi = prob.fd_values_columns(9, 3, 0, n, theta, np.stack([step, -step], axis=1), atol=ATOL)
    assert np.all(fi["status"] == 0)
    want = (-0.5 * Fpm[:, 1] + 0.5 * Fpm[:, 0]) / step[np.arange(n) % nth][:, None]
    cols, ci = prob.fd_jacobian_columns(9, 3, 0, n, theta, step, atol=ATOL)
    assert np.all(ci["status"] == 0) and np.array_equal(cols, want)
    Hs, hi = prob.fd_jacobian_batch(9, 3, 3 + nsim, theta, step, atol=ATOL)
    assert np.all(hi["status"] == 0) and np.array_equal(Hs, want.reshape(nsim, nth, nth).transpose(0, 2, 1))
    k, iv = R.blocks(N, nth), np.exp(-theta)
    for j in range(min(nth, 2)):
        for gpt, sign in ((0, 1.0), (1, -1.0)):
            tp = theta.copy()
            tp[j] += sign * step[j]
            xq = RR.sample_x_z(N, 9, 3, tp, wr, s, resp)[0].astype(np.float64)
            sc, zs = RR.score_at_exact_map(xq, theta, wr, om, resp)
            lam = RR.hessian_floor(xq, zs, theta, wr, om, resp)
            assert lam > 0
            dz = 2 * ATOL / lam
            _, cs = RR.score(xq, zs.astype(np.float64), theta)
            dsc = np.array([iv[b] * (np.abs(zs[k == b]).astype(np.float64).sum() * dz + 0.5 * (k == b).sum() * dz * dz) for b in range(nth)])
            assert (np.abs(Fpm[j, gpt] - sc).astype(np.float64) <= dsc + 4 * R.rounding(cs)).all(), (j, gpt, Fpm[j, gpt], sc.astype(np.float64))
    prob.close()


# ------------------------------------------------------------------------------------------------ 4. implicit-differentiation get_H!
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth,split", VARIANTS)
def test_implicit_H_of_poly_response_at_zero_is_the_noise_context(gpu, M, N, nth, split, w):
    theta = theta_of(nth)
    nsim = 2
    out = []
    for name in (None, "poly_response"):
        prob, _, _, _ = make(M, name, N, nth, split=split, w=w, p=None if name is None else (0.0, 0.0))
        assert prob.has_second_derivatives
        before = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)
        Hb, ib = prob.implicit_H_batch(9, 3, 3 + nsim, theta)
        Hc, ic = prob.implicit_H_columns(9, 3, 0, nsim * nth, theta)
        assert np.array_equal(Hc.reshape(nsim, nth, nth).transpose(0, 2, 1), Hb) and np.array_equal(ic.reshape(nsim, nth), ib)
        assert np.all(ib > 0)
        after = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)      # a map afterwards: the bytes before
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        out.append([Hb, ib, Hc, ic])
        prob.close()
    _same(out[1], out[0], "implicit H, poly_response at (0, 0) against the noise context")


RESPONSES = [("poly_response", LINK), ("saturating_response", SAT)]


@pytest.mark.parametrize("name,p", RESPONSES)
@pytest.mark.parametrize("w", STENCILS)
@pytest.mark.parametrize("N,nth", [(301, 1), (7001, 4)])
def test_implicit_H_against_the_reference_and_its_keywords(gpu, M, N, nth, w, name, p):
    """S256 and S512: two simulations, both tolerances, both entry points, every keyword, get_H_."""
    _implicit_against_the_reference(M, N, nth, w, name, p)


@pytest.mark.parametrize("name,p", RESPONSES)
@pytest.mark.parametrize("N,nth", [(70001, 4), (1500, 12)])
def test_implicit_H_in_clusters_and_in_the_big_tier_against_the_reference(gpu, M, N, nth, name, p):
    """70001 x 4 (clusters: d and e are formed from A zhat and A z_true across workgroups, which a response with phi' = 1 could not
    show) and 1500 x 12 (the big tier): one simulation against the reference at both tolerances, and the two entry points against
    each other; on the built-in stencil (the reference solves every column three times in longdouble)."""
    _implicit_against_the_reference(M, N, nth, None, name, p)


def _implicit_against_the_reference(M, N, nth, w, name, p):
    small = N <= 7001
    theta = theta_of(nth)
    wr = S.BUILTIN if w is None else w
    resp = RR.cubic(p) if name == "poly_response" else RR.saturating(p[0])
    prob, sd, mask, _ = make(M, name, N, nth, w=w, p=p)
    if N == 70001:
        assert prob.placement_info()["workgroups_per_element"] > 1
    om, s = RR.weights(N, sd, mask)
    nsim, atol = (2 if small else 1), RC.ATOL_H
    Hd, its_d = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_maxiter=400)
    Ht, its_t = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_maxiter=400, cg_reltol=1e-12)
    print("CG iterations", its_d.tolist(), "at 1e-12", its_t.tolist())
    assert np.all(its_d > 0) and np.all(its_t >= its_d)
    for Hg, reltol in ((Hd, RC.CG_RELTOL), (Ht, 1e-12)):
        for e in range(nsim):
            Href, bound, lam = RR.implicit_H_bound(N, 9, 3 + e, theta, wr, om, s, resp, atol, reltol)
            err = np.abs(Hg[e] - Href).astype(np.float64)
            print("implicit H: reltol", reltol, "largest error / bound", float((err / bound).max()), "lambda", lam)
            assert (err <= bound).all(), (e, reltol, Hg[e], Href.astype(np.float64), bound)
    cols, ic = prob.implicit_H_columns(9, 3, 0, nsim * nth, theta, atol=atol, cg_maxiter=400)
    assert np.array_equal(cols.reshape(nsim, nth, nth).transpose(0, 2, 1), Hd) and np.array_equal(ic.reshape(nsim, nth), its_d)
    if not small:
        prob.close()
        return
    # keywords
    _, i1 = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_maxiter=1)
    assert np.all(i1 == 1)
    H0, i0 = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_maxiter=0)
    assert np.all(i0 == 0) and np.all(H0 == 0.0)
    _, il = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_maxiter=400, cg_reltol=1e-3)
    assert np.all(il <= its_d) and np.all(il > 0)
    Hz, iz = prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_maxiter=400, H1_is_zero=True)
    assert Hz.tobytes() == Hd.tobytes() and iz.tobytes() == its_d.tobytes()
    with pytest.raises(M.MuseError) as e:
        prob.implicit_H_batch(9, 3, 3 + nsim, theta, atol=atol, cg_Pl="jacobi")
    assert "MUSE_IMPLICIT_PL_JACOBI is for the elementwise models" in str(e.value)
    # through get_H_
    res = M.MuseResult()
    res.theta = theta.copy()
    M.get_H_(res, prob, theta, rng=9, nsims=2, implicit_diff=True)
    Hr, _ = prob.implicit_H_batch(9, 0, 2, theta, atol=1e-1)
    assert np.asarray(res.Hs).tobytes() == Hr.tobytes()
    prob.close()


def test_a_library_without_second_derivatives_refuses_the_implicit_branch(gpu, M):
    """The header of tests/test_response_reference.py that states no phi'' (build() compiled it): the implicit entries refuse it with
    the engine's sentence, and everything else of the family works."""
    from test_response_reference import no_second_model
    sentence = "the implicit-differentiation H needs second derivatives, which this model's header does not supply"
    N, nth, p = 301, 2, (2.0, 0.0)
    theta = theta_of(nth)
    sd, mask, _ = noise_of(N, nth)
    prob = M.HipMuseProblem(None, model=no_second_model(M), ntheta=nth, N=N, noise_sd=sd, mask=mask, link=p)
    assert not prob.has_second_derivatives and prob.get_link() == (p, True)
    before = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)
    assert np.all(before[1]["status"] == 0)
    for call in (lambda: prob.implicit_H_batch(9, 3, 5, theta), lambda: prob.implicit_H_columns(9, 3, 0, 2 * nth, theta),
                 lambda: prob.implicit_H_batch(9, 3, 5, theta, cg_maxiter=0, cg_reltol=1e-3)):
        with pytest.raises(M.MuseError) as e:
            call()
        assert sentence in str(e.value) and "MUSE_MODEL_RESPONSE_SECOND" in str(e.value)
    res = M.MuseResult()
    res.theta = theta.copy()
    with pytest.raises(M.MuseError) as e:
        M.get_H_(res, prob, theta, rng=9, nsims=2, implicit_diff=True)
    assert sentence in str(e.value)
    # the finite-difference get_H! works, and a map afterwards gives the bytes it gave before
    step = 0.02 * np.ones(nth)
    Hs, hi = prob.fd_jacobian_batch(9, 3, 5, theta, step, atol=ATOL)
    assert np.all(hi["status"] == 0) and np.all(np.isfinite(Hs)) and np.all(np.diag(Hs[0]) != 0.0)
    M.get_H_(res, prob, theta, rng=9, nsims=2, step=step)
    assert len(res.Hs) == 2
    after = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # numbers at which the header is not finite at u = 0 (its gain's pole, p1 = 1) are refused; the context keeps what it had
    with pytest.raises(M.MuseError) as e:
        prob.set_link((2.0, 1.0))
    assert "not finite at u = 0" in str(e.value) and prob.get_link() == (p, True)
    again = prob.map_and_score_batch(42, 3, 5, theta, include_data=False, atol=ATOL)
    assert again[0].tobytes() == before[0].tobytes()
    prob.close()
