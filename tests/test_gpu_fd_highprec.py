"""-m gpu: get_H!'s finite-difference map on the HIP path (muse_fd_values_columns, muse_fd_jacobian_columns, muse_fd_jacobian_batch and
the BATCH_FD flavour of the solver kernel behind them) against the extended-precision reference alone -- no oracle in any assertion.

Every value f(eps) = grad_theta logLike(x(theta0 + eps e_j), zhat(x; theta0), theta0) the engine returns is held, entry by entry,
against hp_reference.fd_value (the draw at the perturbed theta, the EXACT MAP and the score at theta0, in longdouble) within
hp_reference.fd_bound, which is derived in fd_value's docstring from atol and the fp64 rounding bounds and from nothing measured.
The oracle restates the engine's recipe; the reference shares no formula with either, so a mistake both of them share -- the solve
or the score at the perturbed theta, the sampling entry of the wrong block, a plus/minus swap, a transposed Hs[s][i][j], a wrong sd
among the big tier's entries, the pair family's [block][2] repacking -- shows here.  tests/test_hp_reference.py holds the oracle
to the same bound and feeds the checker a wrong recipe (the negative control).

No unit is left out: every record must say status == 0 at atol = 1e-8 (test_hp_reference.fd_mismatches asserts it).  The routes
of fd_values_impl (csrc/muse_engine.cpp) each get a case at the smallest N that takes them: the placements of choose_place
(N <= 512, <= 4096, <= 10000 resident; streaming above and for the stencil model; clusters from 65536), the forced streaming
placement and the element split; ntheta 1, 2, 3, 4, 8 and the big tier (12, 33); the two-parameter family at 2, 4 and 8; sampling
entries in the kernel-argument block (ntheta G <= sizeof(MapTheta) kMaxMaps / sizeof(SampleSd) = 26) and uploaded; per-unit
offsets; ranges that begin and end inside a Jacobian from a simulation > 0; and at N = 10000 the normals cache filled by the call,
held (the fiducial's normals from their own kernel), debug bits 21 and 20, after set_normals_cache(False), both fid_modes and
another fid_sim.  cubic stays with the oracle (fd_value's docstring).
"""
import numpy as np
import pytest

import hp_reference as R
from test_hp_reference import fd_mismatches, fd_reference

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

ATOL, SEED, S0, NSIMS = 1e-8, 9, 3, 2


def theta_of(model, nth):
    """Distinct components (a wrong block shows), in a range where every solve reaches atol."""
    t = np.round(np.linspace(-0.4, 0.9, nth) + 0.013 * np.cos(3.0 * np.arange(nth)), 4)
    if model in ("normal_mean_var", "offset_noise"):     # (mu_0 .., tau_0 ..)
        t[: nth // 2] = np.round(np.linspace(0.6, -0.5, nth // 2) + 0.021 * np.arange(nth // 2), 4)
    if model == "smooth":
        # A solve of the stencil model approaches atol = 1e-8 where the objective (|f| ~ N) no longer changes in fp64: a step at
        # |g|_inf ~ 1e-8 lowers f by ~N g^2 / lambda, below ulp(f) from N ~ 10^4 on, and two such steps in a row end the solve
        # f_converged.  It must get from above that region to below atol in one step, which it does when the Hessian
        # A^T A + diag e^-theta is close to a multiple of the identity: theta in [-3.04, -2.91], e^-theta in [18, 21], cond <= 1.2
        # (L-BFGS then gains more than a factor 20 per iteration).  The components stay distinct.
        t = np.round(0.1 * t - 3.0, 4)
    return t


def steps_of(nth):
    """A different step for every column: a transposition or a column's step taken from another cannot cancel."""
    return 0.02 * (1.0 + np.arange(nth) / (nth + 1.0))


def offsets_of(rows, G, salt):
    """Mixed signs up to 0.05, and zeros: every third row has one."""
    off = np.random.default_rng(1000 + salt).uniform(-0.05, 0.05, size=(rows, G))
    off[::3, G // 2] = 0.0
    return off


def make(M, model, N, nth, placement=-1, split=0):
    lib = M.ElementwiseModel.packaged(model) if model in ("normal_mean_var", "offset_noise") else model
    prob = M.HipMuseProblem(None, model=lib, ntheta=nth, N=N)
    if placement >= 0:
        prob.set_placement(placement)
    if split:
        prob.set_element_split(split)
    return prob


def rng_of(nth):
    """A column range that begins inside the first simulation's Jacobian and ends inside the last one's (ntheta > 1)."""
    return (1, NSIMS * nth - 1) if nth > 1 else (0, NSIMS)


def hold_values(prob, model, N, theta0, G, *, fid_mode=0, per_unit=False, fid_sim=None, ctx=""):
    nth = theta0.size
    lo, hi = rng_of(nth)
    off = offsets_of(hi - lo if per_unit else nth, G, N + nth + G)
    kw = {} if fid_sim is None else dict(fid_sim=fid_sim)
    F, info = prob.fd_values_columns(SEED, S0, lo, hi, theta0, off, per_unit=per_unit, atol=ATOL, fid_mode=fid_mode, **kw)
    bad = fd_mismatches(model, N, SEED, S0, lo, hi, theta0, off, per_unit, F, info, ATOL, ctx)
    assert not bad, "\n".join(bad)
    return F


def hold_jacobians(prob, model, N, theta0, *, fid_mode=0, ctx=""):
    """The central_fdm(3, 1) entries are (-1/2 f_- + 1/2 f_+) / step_j of the values, bit for bit -- whole Jacobians and a column
    range -- and those values are the reference's within the bound."""
    nth = theta0.size
    step = steps_of(nth)
    n = NSIMS * nth
    Fpm, info = prob.fd_values_columns(SEED, S0, 0, n, theta0, np.stack([step, -step], axis=1), atol=ATOL, fid_mode=fid_mode)
    bad = fd_mismatches(model, N, SEED, S0, 0, n, theta0, np.stack([step, -step], axis=1), False, Fpm, info, ATOL, ctx + " +-step")
    assert not bad, "\n".join(bad)
    want = (-0.5 * Fpm[:, 1] + 0.5 * Fpm[:, 0]) / step[np.arange(n) % nth][:, None]        # [unit (sim, j)][i]
    lo, hi = rng_of(nth)
    cols, ci = prob.fd_jacobian_columns(SEED, S0, lo, hi, theta0, step, atol=ATOL, fid_mode=fid_mode)
    assert np.all(ci["status"] == 0) and np.array_equal(cols, want[lo:hi]), ctx
    Hs, hi_ = prob.fd_jacobian_batch(SEED, S0, S0 + NSIMS, theta0, step, atol=ATOL, fid_mode=fid_mode)
    assert np.all(hi_["status"] == 0) and np.array_equal(Hs, want.reshape(NSIMS, nth, nth).transpose(0, 2, 1)), ctx   # Hs[s][i][j]
    return Hs


# (model, N, ntheta, G, placement, split, per_unit)   -- fid_mode alternates along the list
CASES = [
    # R256x1: N <= 512
    ("funnel", 1, 1, 2, -1, 0, False), ("funnel", 5, 2, 5, -1, 0, False), ("funnel", 257, 3, 1, -1, 0, False),
    ("funnel", 511, 4, 2, -1, 0, True), ("funnel", 512, 1, 5, -1, 0, False), ("noise", 257, 1, 2, -1, 0, False),
    # R512x4: 512 < N <= 4096
    ("funnel", 513, 2, 2, -1, 0, False), ("funnel", 4096, 8, 1, -1, 0, False), ("noise", 4096, 1, 5, -1, 0, True),
    # R512x10: 4096 < N <= 10000; sampling entries in the kernel arguments (4 x 2 <= 26) and uploaded (8 x 5 > 26, per unit)
    ("funnel", 4097, 3, 5, -1, 0, False), ("funnel", 9999, 1, 2, -1, 0, False), ("funnel", 10000, 4, 2, -1, 0, False),
    ("funnel", 10000, 8, 5, -1, 0, False), ("funnel", 10000, 4, 2, -1, 0, True), ("noise", 9999, 1, 1, -1, 0, False),
    # streaming: N > 10000 (one component: the small tier's kernel; more: the big tier's), forced at 3000; clusters; the element split
    ("funnel", 10001, 1, 2, -1, 0, False), ("funnel", 10001, 2, 5, -1, 0, False), ("noise", 10001, 1, 1, -1, 0, False),
    ("funnel", 3000, 3, 2, 0, 0, False), ("funnel", 3000, 1, 1, 0, 0, True), ("funnel", 66001, 2, 1, -1, 0, False),
    ("funnel", 10000, 4, 2, -1, 4, False),
    # the stencil model (N >= 5)
    ("smooth", 5, 1, 2, -1, 0, False), ("smooth", 601, 4, 2, -1, 0, False), ("smooth", 601, 3, 5, -1, 0, True),
    ("smooth", 66001, 2, 1, -1, 0, False),
    # the big tier: ntheta > 8
    ("funnel", 6000, 12, 2, -1, 0, False), ("funnel", 6000, 33, 1, -1, 0, True), ("smooth", 2500, 12, 1, -1, 0, False),
    ("smooth", 2500, 33, 2, -1, 0, False),
    # the two-parameter family's libraries
    ("normal_mean_var", 257, 2, 5, -1, 0, False), ("normal_mean_var", 4097, 4, 2, -1, 0, True), ("normal_mean_var", 10000, 8, 5, -1, 0, False),
    ("normal_mean_var", 10001, 4, 1, -1, 0, False), ("offset_noise", 513, 2, 2, -1, 0, False), ("offset_noise", 4096, 8, 1, -1, 0, False),
    ("offset_noise", 10000, 4, 5, -1, 0, True), ("offset_noise", 66001, 2, 1, -1, 0, False),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=["-".join(str(v) for v in c) for c in CASES])
def test_fd_values_and_jacobians_against_the_reference(gpu, M, k):
    model, N, nth, G, placement, split, per_unit = CASES[k]
    theta0 = theta_of(model, nth)
    prob = make(M, model, N, nth, placement, split)
    hold_values(prob, model, N, theta0, G, fid_mode=k % 2, per_unit=per_unit, ctx=str(CASES[k]))
    hold_jacobians(prob, model, N, theta0, fid_mode=k % 2, ctx=str(CASES[k]))
    prob.close()


@pytest.mark.parametrize("model,nth,G", [("funnel", 4, 2), ("funnel", 8, 5), ("offset_noise", 4, 2)])
def test_cache_and_fiducial_routes_at_10000(gpu, M, model, nth, G):
    """N = 10000 (R512x10, where the normals cache applies): each route of the call against the reference, not against the others --
    and then, since they are documented to change no bit, against each other."""
    N, theta0 = 10000, theta_of(model, nth)
    prob = make(M, model, N, nth)
    seen = {"fills the cache": hold_values(prob, model, N, theta0, G, ctx="fills the cache")}
    seen["cache held"] = hold_values(prob, model, N, theta0, G, ctx="cache held")           # the fiducial's normals from their kernel
    prob.debug_flags(1 << 21)
    seen["own normals"] = hold_values(prob, model, N, theta0, G, ctx="bit 21")              # ... drawn by the fiducial problem itself
    prob.debug_flags(1 << 20)
    seen["folded"] = hold_values(prob, model, N, theta0, G, ctx="bit 20")                   # the one launch that carries its fiducial
    prob.debug_flags(0)
    prob.set_normals_cache(False)
    seen["after set_normals_cache(False)"] = hold_values(prob, model, N, theta0, G, ctx="set_normals_cache(False)")
    prob.set_normals_cache(True)
    for name, F in seen.items():
        assert np.array_equal(F, seen["fills the cache"]), name
    hold_values(prob, model, N, theta0, G, per_unit=True, ctx="cache held, per unit")
    hold_values(prob, model, N, theta0, G, fid_mode=1, ctx="cache held, fid_mode 1")
    hold_values(prob, model, N, theta0, G, fid_sim=7, ctx="cache held, fid_sim 7")          # the values hold whatever the fiducial
    hold_jacobians(prob, model, N, theta0, ctx="cache held")
    prob.close()
    fresh = make(M, model, N, nth)                                                          # nothing cached: fid_mode 1 fills it
    hold_values(fresh, model, N, theta0, G, fid_mode=1, ctx="fresh, fid_mode 1")
    fresh.close()
    fresh = make(M, model, N, nth)
    hold_values(fresh, model, N, theta0, G, fid_sim=7, ctx="fresh, fid_sim 7")
    fresh.debug_flags(1 << 20)
    hold_values(fresh, model, N, theta0, G, fid_sim=7, ctx="folded, fid_sim 7")
    fresh.close()


@pytest.mark.parametrize("model,N,nth", [("smooth", 601, 3), ("offset_noise", 513, 4)])
def test_jacobian_layout_against_the_longdouble_central_difference(gpu, M, model, N, nth):
    """Hs[s][i][j] = d g_i / d theta_j of models whose H is neither diagonal nor symmetric, against the central difference of the
    reference's values within (bound_+ + bound_-) / (2 step_j), a different step for every column."""
    theta0, step = theta_of(model, nth), steps_of(nth)
    prob = make(M, model, N, nth)
    Hs, info = prob.fd_jacobian_batch(SEED, S0, S0 + NSIMS, theta0, step, atol=ATOL)
    cols, ci = prob.fd_jacobian_columns(SEED, S0, 0, NSIMS * nth, theta0, step, atol=ATOL)
    prob.close()
    assert Hs.shape == (NSIMS, nth, nth) and info.shape == (NSIMS, nth, 2) and np.all(info["status"] == 0) and np.all(ci["status"] == 0)
    ref, bmax = np.empty((NSIMS, nth, nth)), 0.0
    for s in range(NSIMS):
        for j in range(nth):
            (fp, ap), (fm, am) = (fd_reference(model, N, SEED, S0 + s, theta0, j, e) for e in (step[j], -step[j]))
            want = (fp - fm) / R.LD(2.0 * step[j])
            ref[s, :, j] = want.astype(np.float64)
            bound = (R.fd_bound(ap, ATOL) + R.fd_bound(am, ATOL)) / (2.0 * step[j])
            bmax = max(bmax, float(bound.max()))
            for got, what in ((Hs[s, :, j], "Hs[s][:, j]"), (cols[s * nth + j], "cols[s ntheta + j]")):
                err = np.abs(got - want).astype(np.float64)
                assert (err <= bound).all(), (what, s, j, got, want.astype(np.float64), err, bound)
    # the case tells a transposed layout from the right one: H is far from symmetric on the scale of the bound
    assert np.abs(ref - ref.transpose(0, 2, 1)).max() > 100 * bmax
