"""-m gpu: MUSE_IMPLICIT_PL_JACOBI (include/muse_hip.h) -- CG preconditioned by the Hessian's diagonal in the implicit-differentiation
get_H! of the elementwise models -- and the CG keywords the kernels of the built-in and one-parameter models honour with it (a header
of the one-parameter family without it as well).

The reference is longdouble: the exact diagonal solve of tests/hp_reference.py (funnel, noise, cubic) and tests/pair_implicit_reference.py
(offset_noise), and the preconditioned recurrence of tests/jacobi_reference.py.  The bounds are those the existing default-CG tests
hold each model to: rtol = atol / max|H| = 1e-6 of tests/test_gpu_highprec.py (test_implicit_H_against_the_reference: CG's stopping
rule at sqrt(eps) times cond(A)) for the one-parameter models, tests/test_pair_implicit.py's `within` (twice the reference's own
bound) for the two-parameter family.  Shapes: N = 1001 (odd: the pad element is live; a block boundary inside a wave), 3 simulations
(one H column per workgroup); 2 simulations with 8 components; the big tier; clusters at N = 65 536; 300 simulations (all columns
of a simulation in one workgroup).

`cubic` is the packaged models/cubic.h.  It declares no run-time constant vectors (no packaged header with second derivatives does,
and no header is compiled here), so "per-element constants" are not what varies: its d2 o / dz2 differs from element to element
through the MAP, which is what CG's iteration count depends on.  Model::second reading a context's constant vectors is not exercised
through the preconditioned instantiations."""
import numpy as np
import pytest

import hp_reference as R
import jacobi_reference as J
import pair_implicit_reference as P
from test_pair_implicit import theta_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

LD = R.LD
SEED, ATOL = 17, 1e-10
HP_RTOL = 1e-6          # tests/test_gpu_highprec.py, test_implicit_H_against_the_reference / _of_the_cubic_header


def hp_bound(Hh):
    """The entrywise bound of np.testing.assert_allclose(H, Hh, rtol=1e-6, atol=1e-6 max|Hh|) of tests/test_gpu_highprec.py."""
    return HP_RTOL * np.abs(Hh) + HP_RTOL * np.abs(Hh).max()


def problem(M, model, N, nth):
    m = M.ElementwiseModel.packaged(model) if model in ("cubic", "offset_noise") else model
    return M.HipMuseProblem(None, model=m, ntheta=nth, N=N)


def _terms(model, x, zt, iv, zh):
    """(d, b1, dFz) of funnel / cubic at zh: A = diag(d), dFdtheta1 = b1 on the column's block, dFdtheta = dFz on the row's."""
    if model == "funnel":
        return -(LD(1) + iv), LD(0.5) * zt, iv * zh
    hpz, hpt = LD(1) + LD(3) * zh * zh / LD(10), LD(1) + LD(3) * zt * zt / LD(10)
    d = -(iv + hpz * hpz - (x - (zh + zh ** 3 / LD(10))) * (LD(6) * zh / LD(10)))
    return d, hpz * (LD(0.5) * hpt * zt), iv * zh


def operands(prob, M, model, N, sim, theta):
    """Longdouble operands of one simulation of a one-parameter model at the exact MAP: (d, b [nth, N], dF [nth, N], H1, mapt): A =
    diag(d), b[j] = dFdtheta1[:, j], H = H1 - sum_i dF[i2] (A^-1 b[j]) -- the terms of hp_reference.implicit_H, kept apart -- and
    mapt [N] = |d term_i / d zhat_i| / |A_ii|: times the MAP's atol (|grad_i| <= atol, so |zhat_i - z*_i| <= atol / |A_ii|) it bounds
    what the MAP's own tolerance puts into a diagonal entry of H, in the manner of pair_implicit_reference's bound_H1."""
    th = np.asarray(theta, dtype=np.float64)
    B = th.size
    x, zt = R.sample_x_z(model, N, SEED, sim, th)
    k, iv = R._coefs(model, N, th)[:2]
    H1 = np.zeros((B, B), LD)
    if model == "noise":
        zh = iv * x / (LD(1) + iv)
        dx = LD(0.5) * (x - zt)
        H1[0, 0] = iv[0] * np.sum((x - zh) * dx)
        # H = sum iv / (1 + iv) (x - zhat) dx: d term / d zhat = -iv / (1 + iv) dx; H1 alone: -iv dx
        return (-(iv + LD(1)), (iv * dx)[None], (-iv * (x - zh))[None], H1, iv * np.abs(dx) / (LD(1) + iv) ** 2,
                iv * np.abs(dx) / (LD(1) + iv))
    if model == "funnel":
        zh = x / (LD(1) + iv)
    else:
        xs, _ = prob.sample_x_z(M.SimRng(SEED, sim), th)
        z0, _ = prob.zhat_at_theta(xs, np.zeros(N), th, ATOL)
        zh = R._cubic_polish(x, iv, z0.astype(LD))
    d, b1, dFz = _terms(model, x, zt, iv, zh)
    h = LD(1e-5)       # central difference of term_i = dFz_i b1_i / d_i in zhat_i (longdouble: its error is ~1e-10 of the derivative)
    tp, tm = _terms(model, x, zt, iv, zh + h), _terms(model, x, zt, iv, zh - h)
    mapt = np.abs(tp[2] * tp[1] / tp[0] - tm[2] * tm[1] / tm[0]) / (LD(2) * h) / np.abs(d)
    masks = [(k == j).astype(LD) for j in range(B)]
    return d, np.array([b1 * m for m in masks]), np.array([dFz * m for m in masks]), H1, LD(1.0001) * mapt, None


def H_from(d, b, dF, H1, solve):
    B = b.shape[0]
    H = H1.copy()
    for j in range(B):
        v = solve(d, b[j])
        for i2 in range(dF.shape[0]):
            H[i2, j] -= np.sum(dF[i2] * v)
    return H.astype(np.float64)


def reference(prob, M, model, N, sim, theta):
    """dict(H exact, bound, round, sum_round, ops).  round: the rounding term of `bound`, i.e. its part that does not scale with CG's
    tolerance -- for the one-parameter models the absolute term of tests/test_gpu_highprec.py's assert_allclose (1e-6 max |H|), for
    the two-parameter family pair_implicit_reference's bound at reltol = 0 (the existing bound itself is doubled, as `within` does).
    The default call and the preconditioned one run the same MAP solve, and their distances from the EXACT MAP's H both contain that
    solve's stopping error, which the absolute term covers and the rounding of the sums alone does not: a solve may end f_converged
    with |grad|_inf above atol (solver.hpp, MUSE_STATUS_F_CONVERGED; cubic at N = 1001: distances of 2e-8 to 1.3e-7 on entries of
    ~3e2 from either call, of either sign).  sum_round: the rounding of an entry's sums (hp_reference.rounding of sqrt(n) sum |terms|)
    plus atol carried through a g_converged MAP (operands: mapt) -- used for noise's H1, whose quadratic solve ends there."""
    if model == "offset_noise":
        ref = P.implicit_H(model, N, SEED, sim, theta)
        return dict(H=ref["H"], H1=ref["H1"], bound=2.0 * ref["bound"](), round=ref["bound"](0.0), sum_round=None, ops=None)
    d, b, dF, H1, mapt, h1t = operands(prob, M, model, N, sim, theta)
    H = H_from(d, b, dF, H1, lambda dd, bb: J.apply_pl(bb, dd))
    cond, mapb = np.zeros(H.shape, LD), np.zeros(H.shape, LD)
    for j in range(b.shape[0]):
        for i2 in range(dF.shape[0]):
            cond[i2, j] = np.sqrt(LD(N)) * np.sum(np.abs(dF[i2] * b[j] / d))
            mapb[i2, j] = LD(ATOL) * np.sum(mapt * (dF[i2] != 0) * (b[j] != 0))
    if model == "noise":    # H1's terms iv (x - zhat) dx/dtheta = -dF b / iv
        cond[0, 0] += np.sqrt(LD(N)) * np.sum(np.abs(b[0] * dF[0]) / R._coefs(model, N, np.asarray(theta, dtype=np.float64))[1])
    return dict(H=H, H1=H1.astype(np.float64), bound=hp_bound(H), round=HP_RTOL * np.abs(H).max(),
                sum_round=R.rounding(cond.astype(np.float64)) + mapb.astype(np.float64), ops=(d, b, dF, H1), h1_map=h1t)


def check_against(got, ref, what):
    err = np.abs(got - ref["H"])
    print(what, "max |err| / bound =", float(np.max(err / np.maximum(ref["bound"], 1e-300))), "max |err| =", float(err.max()))
    assert np.all(err <= ref["bound"]), (what, err, ref["bound"])
    return err


#         model           N      theta                                           nsims  cluster
CASES = [("funnel",       1001,  [0.3, -0.5, 1.0],                               3,     False),
         ("noise",        1001,  [-0.2],                                         3,     False),
         ("cubic",        1001,  [0.5, -0.3],                                    3,     False),
         ("offset_noise", 1001,  None,                                           3,     False),
         ("funnel",       1001,  [0.3, -0.5, 1.0, 0.2, -0.1, 0.4, 0.0, -0.3],    2,     False),      # imp_split == ntheta, 8 components
         ("funnel",       4096,  [0.3, -0.5, 1.0, 0.2, -0.1, 0.4, 0.0, -0.3, 0.6], 3,   False),      # the big tier
         ("funnel",       65536, [0.3, -0.5],                                    1,     True),
         ("noise",        65536, [0.4],                                          1,     True),
         ("cubic",        65536, [0.5],                                          1,     True),
         ("offset_noise", 65536, None,                                           1,     True)]


@pytest.mark.parametrize("model,N,theta,nsims,cluster", CASES)
def test_one_iteration_and_the_exact_solve(gpu, M, model, N, theta, nsims, cluster):
    """1. cg_iters_out is 1 for every column with a right-hand side and 0 otherwise; 2. H within the model's default-CG bound of the
    exact longdouble solve, the default call within it too, and the preconditioned result no further from exact than the default one
    plus the bound's rounding term; 4. the _ex entry at the defaults gives the legacy entry's bits."""
    theta = theta_of(model, 4) if theta is None else np.asarray(theta, dtype=np.float64)
    nth = theta.size
    prob = problem(M, model, N, nth)
    assert (prob.placement_info()["workgroups_per_element"] > 1) == cluster      # (the implicit entry: clusters exactly when the maps are)
    Hd, itd = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL, cg_maxiter=1000)
    Hj, itj = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL, cg_maxiter=1000, cg_Pl="jacobi")
    print(model, N, "CG iterations: default", itd.tolist(), "jacobi", itj.tolist())
    for s in range(nsims):
        ref = reference(prob, M, model, N, s, theta)
        if ref["ops"] is not None:
            nonzero = np.array([bool(np.any(bj != 0)) for bj in ref["ops"][1]])
        else:
            nonzero = np.ones(nth, dtype=bool)
        assert np.array_equal(itj[s], nonzero.astype(np.int32)), (s, itj[s])
        ed = check_against(Hd[s], ref, f"{model} N={N} default sim {s}")
        ej = check_against(Hj[s], ref, f"{model} N={N} jacobi sim {s}")
        assert np.all(ej <= ed + ref["round"]), (s, ej, ed, ref["round"])
    Hl, il = np.empty_like(Hd), np.zeros_like(itd)
    th = M._capi.f8(theta, nth)
    prob._check(prob._lib.muse_implicit_H_batch(prob._ctx, SEED, 0, nsims, M._capi.ptr(th), ATOL, 1000, M._capi.ptr(Hl), M._capi.ptr(il)))
    assert np.array_equal(Hl, Hd) and np.array_equal(il, itd)
    prob.close()


@pytest.mark.parametrize("model,theta", [("funnel", [0.3, -0.5, 1.0]), ("cubic", [0.5, -0.3]), ("offset_noise", None)])
def test_all_columns_in_one_workgroup_equal_the_columns_entry(gpu, M, model, theta):
    """300 simulations: more than half the launch's slots, so a workgroup runs all columns of its simulation (imp_split == 1); the
    columns entry always runs one column per workgroup.  The same bits and counts, all ones."""
    N, many = 1001, 300
    theta = theta_of(model, 4) if theta is None else np.asarray(theta, dtype=np.float64)
    nth = theta.size
    prob = problem(M, model, N, nth)
    big, ib = prob.implicit_H_batch(SEED, 0, many, theta, cg_Pl="jacobi")
    cols, ic = prob.implicit_H_columns(SEED, 0, 0, many * nth, theta, cg_Pl="jacobi")
    assert np.array_equal(cols.reshape(many, nth, nth).transpose(0, 2, 1), big) and np.array_equal(ic.reshape(many, nth), ib)
    assert np.all(ib == 1)
    few, _ = prob.implicit_H_batch(SEED, 2, 5, theta, cg_Pl="jacobi")
    assert np.array_equal(few, big[2:5])
    prob.close()


@pytest.mark.parametrize("model,theta", [("funnel", [0.3, -0.5, 1.0]), ("noise", [-0.2]), ("cubic", [0.5, -0.3])])
def test_keywords_the_elementwise_kernels_now_honour(gpu, M, model, theta):
    """cg_maxiter = 0: H = H1 (exactly 0 for funnel and cubic, whose H1 is zero); H1-is-zero: H + H1 = the default H.  With the
    preconditioner on every model; without it on the header of the one-parameter family, whose library routes the keywords alone to
    the same kernels (Pl off) -- the built-in library without the bit keeps its refusal (tests/test_pair_implicit.py,
    test_other_models_refuse_what_their_kernels_do_not_honour)."""
    N, nsims = 1001, 3
    theta = np.asarray(theta, dtype=np.float64)
    prob = problem(M, model, N, theta.size)
    Hd, itd = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL)
    for pl in ((None, "jacobi") if model == "cubic" else ("jacobi",)):
        H0, it0 = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL, cg_maxiter=0, cg_Pl=pl)
        Hz, itz = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL, H1_is_zero=True, cg_Pl=pl)
        assert np.all(it0 == 0)
        assert np.all(np.abs(itz - itd) <= 1) if pl is None else np.all(itz <= 1)     # (Pl off: the recurrence is plain CG)
        for s in range(nsims):
            ref = reference(prob, M, model, N, s, theta)
            if model == "noise":
                # H1 = iv sum (x - zhat) dx/dtheta: the rounding of its sum and the MAP's tolerance carried through (|dH1/dzhat_i| atol / A_ii)
                h1b = ref["sum_round"] + ATOL * float(np.sum(ref["h1_map"]))
                assert np.all(np.abs(H0[s] - ref["H1"]) <= h1b), (s, H0[s], ref["H1"], h1b)
            else:
                assert not H0[s].any()
            assert np.all(np.abs(Hz[s] + ref["H1"] - Hd[s]) <= ref["bound"]), (pl, s, Hz[s], ref["H1"], Hd[s])
    prob.close()


def test_a_loose_tolerance_on_the_cubic_header(gpu, M):
    """cg_reltol = 1e-3 on models/cubic.h: fewer iterations than the default, and H is that of the longdouble run of the same loop with
    the same keyword (tests/jacobi_reference.py, Pl off) within the bound; cg_abstol above every |b| stops at once."""
    N, nsims, theta = 1001, 3, np.array([0.5, -0.3])
    prob = problem(M, "cubic", N, 2)
    Hd, itd = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL)
    Hl, itl = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL, cg_reltol=1e-3)
    print("CG iterations: default", itd.tolist(), "reltol 1e-3", itl.tolist())
    assert np.all(itl < itd) and np.all(itl >= 1)
    for s in range(nsims):
        ref = reference(prob, M, "cubic", N, s, theta)
        d, b, dF, H1 = ref["ops"]
        its = []
        def loose(dd, bb):
            x, _, it = J.solve(dd, bb, jacobi=False, reltol=1e-3)
            its.append(it)
            return x
        Hr = H_from(d, b, dF, H1, loose)
        assert np.array_equal(itl[s], its), (s, itl[s], its)
        assert np.all(np.abs(Hl[s] - Hr) <= hp_bound(Hr)), (s, Hl[s], Hr)
    H0, it0 = prob.implicit_H_batch(SEED, 0, nsims, theta, atol=ATOL, cg_abstol=1e9)
    assert np.all(it0 == 0) and not H0.any()
    for bad in (dict(cg_reltol=-1.0), dict(cg_abstol=float("nan")), dict(cg_maxiter=-1)):
        with pytest.raises(M.MuseError):
            prob.implicit_H_batch(SEED, 0, 1, theta, **bad)
    prob.close()


@pytest.mark.parametrize("variant", ["plain", "stencil", "noise"])
def test_the_stencil_model_refuses_the_bit(gpu, M, variant):
    """MUSE_ERR_INVALID with the reason -- the operator -- in muse_last_error(); the context stays usable: the default call before and
    after gives the same bits."""
    N, theta = 1001, [1.0, 0.5]
    prob = M.HipMuseProblem(None, model="smooth", ntheta=2, N=N)
    if variant == "stencil":
        prob.set_stencil((0.6, 0.2))
    if variant == "noise":
        rng = np.random.default_rng(1)
        prob.set_noise(10.0 ** rng.uniform(-1, 0, N), rng.uniform(size=N) > 0.2)
    H, its = prob.implicit_H_batch(SEED, 0, 2, theta)
    with pytest.raises(M.MuseError, match="operator") as e:
        prob.implicit_H_batch(SEED, 0, 2, theta, cg_Pl="jacobi")
    assert e.value.args and "MUSE_IMPLICIT_PL_JACOBI" in str(e.value)
    with pytest.raises(M.MuseError, match="operator"):
        prob.implicit_H_columns(SEED, 0, 0, 4, theta, cg_Pl="jacobi")
    H2, its2 = prob.implicit_H_batch(SEED, 0, 2, theta)
    assert np.array_equal(H2, H) and np.array_equal(its2, its)
    prob.close()


def test_get_H_with_pl_jacobi_end_to_end(gpu, M):
    """get_H(implicit_diff=True, implicit_diff_cg_kwargs={"Pl": "jacobi"}) on models/offset_noise.h through muse.py, at the shape of
    tests/test_pair_implicit.py's test_muse_on_offset_noise_against_the_exact_posterior (N = 10^4, K = 1, 512 simulations): the CG
    histories are ones (zeros where a column has no right-hand side); sigma is the default call's within the tolerance that test
    allows between its implicit and finite-difference routes (its formula, at its nsims); and, since the two calls run the same
    simulations and MAPs and differ in the CG loop alone, H agrees entry by entry to CG's level -- rtol 1e-6 of max |H|, what
    tests/test_gpu_highprec.py holds the implicit H to -- and Sigma = (H' J^-1 H + H_prior)^-1 to that times 2 cond(H) (first order:
    dSigma = -Sigma (dH' J^-1 H + H' J^-1 dH) Sigma, |dH| <= 1e-6 |H|)."""
    from test_pair_model import PRIOR_SIGMA
    N, K, nsims, truth = 10000, 1, 512, [0.8, 0.5]
    model = M.ElementwiseModel.packaged("offset_noise")
    tmp = M.HipMuseProblem(None, model=model, ntheta=2 * K, N=N)
    x, _ = tmp.sample_x_z(M.SimRng(99, M.DATA_SIM), truth)
    tmp.close()
    prob = M.HipMuseProblem(x, model=model, ntheta=2 * K, prior=M.GaussianPrior(0.0, PRIOR_SIGMA))
    res = M.muse(prob, [0.0] * (2 * K), rng=20240, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-6, alpha=1.0,
                 get_covariance=False)
    M.get_J_(res, prob, nsims=nsims)
    tol = 5.0 * 0.5 * np.sqrt(2.0 / (nsims - 1)) + 0.03          # (test_muse_on_offset_noise_against_the_exact_posterior)
    got = {}
    for how, kw in (("default", {}), ("jacobi", dict(implicit_diff_cg_kwargs={"Pl": "jacobi"}))):
        res.Hs, res.H = [], None
        res.metadata.pop("implicit_diff_cg_hists", None)
        M.get_H_(res, prob, nsims=nsims, implicit_diff=True, **kw)
        Sigma = np.atleast_2d(res.Sigma).copy()
        got[how] = (np.sqrt(np.diag(Sigma)), np.array(res.metadata["implicit_diff_cg_hists"]), np.array(res.H), Sigma)
    (sd, itd, Hd, Sd), (sj, itj, Hj, Sj) = got["default"], got["jacobi"]
    print("sigma jacobi / default", sj / sd, "default CG", itd.min(), itd.max(), "max |dH| / max |H|", np.abs(Hj - Hd).max() / np.abs(Hd).max(),
          "max |dSigma| / max |Sigma|", np.abs(Sj - Sd).max() / np.abs(Sd).max())
    assert itj.shape == (nsims, 2 * K) and np.all((itj == 1) | (itj == 0)) and itj.any()
    assert np.all(np.abs(sj / sd - 1.0) < tol)
    assert np.all(np.abs(Hj - Hd) <= HP_RTOL * np.abs(Hd).max()), (Hj, Hd)
    assert np.all(np.abs(Sj - Sd) <= 2.0 * np.linalg.cond(Hd) * HP_RTOL * np.abs(Sd).max()), (Sj, Sd)
    prob.close()
