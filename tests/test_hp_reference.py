"""The extended-precision reference (tests/hp_reference.py) validated before any GPU time is spent, and the CPU oracle held to it:
Philox known answers, the oracle's normals within the committed generator bound K, the oracle's per-sim operators, MAPs and
implicit H within the reference's stated bounds at the edge sizes."""
import os

import numpy as np
import pytest

import hp_reference as R

pytestmark = pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)

# The generator bound: |n - n_hp| <= K_GEN 2^-52 max(1, r), r = sqrt(-2 log u1), for every normal of the stream (oracle and
# device are bit-equal).  Measured maximum over the 1.2e7 elements of test_oracle_normals_within_K: 1.47 (log_unit's and
# sincospi_02's few-ulp polynomials, times r).  test_oracle's accuracy test admits errors up to 5e-15, about 22 such units: a
# Lg*/S*/C* coefficient changed as far as that test still accepts moves some element past K.  Smaller changes can stay below K
# (Lg1 off by 1e-14 relative does).
K_GEN = 2

EDGE_N = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257)


def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 10 rounds (the vectors of tests/test_oracle.py)
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        w = R.philox4x32_10(*[np.array([c], dtype=np.uint64) for c in ctr], *key)
        assert [int(v[0]) for v in w] == want


def test_box_muller_against_mpmath():
    """Spot check of the longdouble Box-Muller against 40-digit arithmetic."""
    import mpmath
    mpmath.mp.dps = 40
    n1, n2, _ = R.normals(3, 2**40 + 7, 64)
    u1, u2 = R.uniforms(3, 2**40 + 7, np.arange(64, dtype=np.uint64))
    for j in range(0, 64, 7):
        a, b = mpmath.mpf(int(u1[j] * R.LD(2) ** 53)) / 2**53, mpmath.mpf(int(u2[j] * R.LD(2) ** 53)) / 2**53
        r = mpmath.sqrt(-2 * mpmath.log(a))
        for got, want in ((n1[j], r * mpmath.cos(2 * mpmath.pi * b)), (n2[j], r * mpmath.sin(2 * mpmath.pi * b))):
            assert abs(mpmath.mpf(float(got)) - want) <= 2.0**-52 * max(1.0, float(r))     # fp64 rounding of the longdouble
            assert abs(float(mpmath.mpf(np.format_float_positional(got, unique=True)) - want)) <= 2.0**-60 * max(1.0, float(r))


@pytest.mark.parametrize("seed,sim", [(0, 0), (11, 3), (1234, 2**40 + 7), (2**33 + 5, (1 << 32) - 1), (42, 17), (7, 2**62 - 1)])
def test_oracle_normals_within_K(O, seed, sim):
    """2e6 elements per stream, 1.2e7 in all."""
    N = 2_000_000
    n1, n2 = O.normals(seed, sim, N)
    h1, h2, r = R.normals(seed, sim, N)
    tol = K_GEN * 2.0**-52 * np.maximum(1.0, r.astype(np.float64))
    for n, h in ((n1, h1), (n2, h2)):
        err = np.abs(n - h).astype(np.float64)
        assert (err <= tol).all(), f"max {np.max(err / tol) * K_GEN:.2f} units of 2^-52 max(1, r)"


def test_blocks_partition():
    for N in (1, 2, 3, 5, 64, 65, 4097):
        for B in (1, 2, 3, 8):
            k = R.blocks(N, B)
            assert k[0] == 0 and np.all(np.diff(k) >= 0) and k.max() < B
            if N >= B:
                assert k[-1] == B - 1
            # block b = [ceil(b N / B), ceil((b + 1) N / B)): the n_k of the constant 1/2 sum_k n_k theta_k
            lo = [-(-b * N // B) for b in range(B + 1)]
            assert [int(v) for v in R.block_sizes(N, B)] == [lo[b + 1] - lo[b] for b in range(B)]


def _cases():
    out = []
    for N in EDGE_N:
        out.append(("funnel", N, [0.4]))
        out.append(("noise", N, [-0.3]))
        out.append(("smooth", N, [1.0]))
        if N >= 3:
            out.append(("funnel", N, [0.4, -0.7, 1.3]))
            out.append(("smooth", N, [1.0, 2.0, -0.5]))
    out += [("funnel", 4097, [0.1 * k for k in range(8)]), ("smooth", 4097, [1.0, 2.0, 3.0, 0.5])]
    return out


@pytest.mark.parametrize("model,N,theta", _cases())
def test_oracle_operators_within_bounds(O, model, N, theta):
    x, z = O.sample_x_z(model, N, 5, 1, theta)
    zz = 0.7 * z + 0.1
    fo, go = O.logLike_and_grad_z(model, x, zz, theta)
    f, g, cf, cg = R.objective(model, x, zz, theta)
    assert abs(-fo - f) <= R.rounding(cf)                      # the engine's convention: f = -logLike, 1/2 sum n_k theta_k
    assert (np.abs(-go - g) <= R.rounding(cg)).all()
    s, cs = R.score(model, x, zz, theta)
    assert (np.abs(O.grad_theta(model, x, zz, theta) - s) <= R.rounding(cs)).all()
    # the draw itself: x, z from the reference's normals (the oracle's exp is within an ulp of the longdouble one)
    xh, zh = R.sample_x_z(model, N, 5, 1, theta)
    _, _, r = R.normals(5, 1, N)
    sd = np.exp(0.5 * np.max(np.abs(theta)))
    gen = K_GEN * 2.0**-52 * np.maximum(1.0, r.astype(np.float64)) * sd
    assert (np.abs(z - zh) <= gen + 4 * R.U * np.abs(zh)).all()
    assert (np.abs(x - xh) <= 2 * gen + R.rounding(np.abs(xh) + 2 * np.abs(zh))).all()


@pytest.mark.parametrize("model,N,theta", [c for c in _cases() if c[1] <= 257] + [("funnel", 4097, [0.3, 1.0])])
def test_oracle_map_within_bounds(O, model, N, theta):
    """f_min / gnorm of the oracle's record against f_hp / |g_hp|_inf at its own zhat, zhat against the exact MAP.  (atol 1e-9
    on smooth ends some solves f_converged: the record must describe zhat whatever the status.)"""
    x, _ = O.sample_x_z(model, N, 9, 4, theta)
    for atol in (1e-3, 1e-9):
        zh, info = O.zhat_at_theta(model, x, np.zeros(N), theta, atol)
        f, g, cf, cg = R.objective(model, x, zh, theta)
        gi = np.abs(g).astype(np.float64)
        gb = R.rounding(cg).max()
        if info["status"] == 0:
            assert gi.max() <= atol + gb
        assert abs(info["gnorm"] - gi.max()) <= gb
        assert abs(info["f_min"] - f) <= R.rounding(cf)
        zs = R.exact_map(model, x, theta)
        if model == "smooth":       # |dz|_2 <= |g|_2 / lambda_min, lambda_min >= e^{-theta_max}
            assert np.linalg.norm((zh - zs).astype(np.float64)) <= (np.linalg.norm(gi) + np.sqrt(N) * gb) * np.exp(np.max(theta))
        else:                       # diagonal: z - z* = g_i / H_ii exactly
            H = R.diag_hessian(model, x, zh, theta).astype(np.float64)
            assert (np.abs((zh - zs).astype(np.float64)) <= (gi + gb) / H).all()


def test_oracle_cubic_within_bounds(O):
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "museinference.jl_amd", "models", "cubic.h")
    with O.user_model(header, "cubic"):
        for N, theta in ((1, [0.3]), (5, [0.3, -0.4]), (257, [1.0, 0.2, -1.0]), (4097, [0.5])):
            x, z = O.sample_x_z("user", N, 3, 2, theta)
            zz = 0.7 * z + 0.1
            fo, go = O.logLike_and_grad_z("user", x, zz, theta)
            f, g, cf, cg = R.objective("cubic", x, zz, theta)
            assert abs(-fo - f) <= R.rounding(cf) and (np.abs(-go - g) <= R.rounding(cg)).all()
            s, cs = R.score("cubic", x, zz, theta)
            assert (np.abs(O.grad_theta("user", x, zz, theta) - s) <= R.rounding(cs)).all()
            zh, info = O.zhat_at_theta("user", x, np.zeros(N), theta, 1e-9)
            f, g, cf, cg = R.objective("cubic", x, zh, theta)
            assert abs(info["f_min"] - f) <= R.rounding(cf)
            assert abs(info["gnorm"] - np.abs(g).max()) <= R.rounding(cg).max()
            if N <= 257:
                H, _ = O.implicit_H("user", N, 3, 2, theta, atol=1e-10, cg_maxiter=200)
                Hh = R.implicit_H("cubic", N, 3, 2, theta, zhat_start=zh).astype(np.float64)
                np.testing.assert_allclose(H, Hh, rtol=1e-6, atol=1e-6 * np.abs(Hh).max())


def test_oracle_pair_model_within_bounds(O):
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "museinference.jl_amd", "models",
                          "normal_mean_var.h")
    with O.user_model(header, "normal_mean_var"):
        for N, theta in ((1, [0.3, -0.2]), (5, [0.3, -0.4, 1.0, 0.2]), (257, [1.0, 0.2, -1.0, 0.5, 0.0, 0.3])):
            x, z = O.sample_x_z("user", N, 3, 2, theta)
            zz = 0.7 * z + 0.1
            fo, go = O.logLike_and_grad_z("user", x, zz, theta)
            f, g, cf, cg = R.objective("normal_mean_var", x, zz, theta)
            assert abs(-fo - f) <= R.rounding(cf) and (np.abs(-go - g) <= R.rounding(cg)).all()
            s, cs = R.score("normal_mean_var", x, zz, theta)
            assert (np.abs(O.grad_theta("user", x, zz, theta) - s) <= R.rounding(cs)).all()
            zh, info = O.zhat_at_theta("user", x, np.zeros(N), theta, 1e-9)
            f, g, cf, cg = R.objective("normal_mean_var", x, zh, theta)
            gi, gb = np.abs(g).astype(np.float64), R.rounding(cg).max()
            assert abs(info["f_min"] - f) <= R.rounding(cf) and abs(info["gnorm"] - gi.max()) <= gb
            zs = R.exact_map("normal_mean_var", x, theta)
            assert (np.abs((zh - zs).astype(np.float64)) <= (gi + gb) / R.diag_hessian("normal_mean_var", x, zh, theta).astype(float)).all()


# implicit H: rtol 1e-6 -- CG stops at |r| <= sqrt(eps) |b| (src/muse.jl's cg defaults), i.e. a relative residual of 1.5e-8
# times cond(A) <= (1 + e^{-theta_min}) / e^{-theta_max} ~ 50 here: ~1e-6, not rounding.
@pytest.mark.parametrize("model,N,theta", [("funnel", 65, [0.3]), ("funnel", 257, [0.3, -0.5, 1.0]), ("noise", 64, [0.4]),
                                           ("noise", 4097, [-0.2]), ("smooth", 63, [1.0, 0.5]), ("smooth", 257, [1.0, 2.0, -0.5, 0.3]),
                                           ("smooth", 3, [1.0])])
def test_oracle_implicit_H(O, model, N, theta):
    H, _ = O.implicit_H(model, N, 17, 2, theta, atol=1e-10, cg_maxiter=1000)
    Hh = R.implicit_H(model, N, 17, 2, theta).astype(np.float64)
    np.testing.assert_allclose(H, Hh, rtol=1e-6, atol=1e-6 * np.abs(Hh).max())


# ------------------------------------------------------------------------------------------------ finite-difference get_H! values
MODELS_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "museinference.jl_amd", "models")
_FD_REFERENCE = {}      # (model, N, seed, sim, theta0, j, theta0[j] + eps) -> (f, aux): computed once, shared by the tests, never changed


def fd_reference(model, N, seed, sim, theta0, j, eps):
    th = np.atleast_1d(np.asarray(theta0, dtype=np.float64))
    key = (model, N, seed, sim, th.tobytes(), j, float(th[j] + np.float64(eps)))
    if key not in _FD_REFERENCE:
        _FD_REFERENCE[key] = R.fd_value(model, N, seed, sim, th, j, eps)
    return _FD_REFERENCE[key]


def fd_mismatches(model, N, seed, sim_begin, lo, hi, theta0, offsets, per_unit, F, info, atol, ctx=""):
    """Every entry of F [hi - lo, G, ntheta] (the units [lo, hi) of the list (sim_begin, column 0), (sim_begin, column 1), ...)
    against hp_reference.fd_value within fd_bound: the entries outside it, each naming its unit, simulation, column, grid point,
    offset and score component.  No unit is left out: every record must say status == 0, which is what the bound is derived for."""
    theta0, offsets = np.atleast_1d(np.asarray(theta0, np.float64)), np.asarray(offsets, np.float64)
    nth, G = theta0.size, offsets.shape[1]
    assert F.shape == (hi - lo, G, nth) and info.shape == (hi - lo, G), (ctx, F.shape, info.shape)
    assert np.all(info["status"] == 0), (ctx, "status", info["status"])
    bad = []
    for u in range(hi - lo):
        sim, j = sim_begin + (lo + u) // nth, (lo + u) % nth
        for g in range(G):
            eps = offsets[u if per_unit else j, g]
            f, aux = fd_reference(model, N, seed, sim, theta0, j, eps)
            err, bound = np.abs(F[u, g] - f).astype(np.float64), R.fd_bound(aux, atol)
            for i in np.nonzero(~(err <= bound))[0]:
                bad.append(f"{ctx} unit {lo + u} sim {sim} column {j} grid {g} offset {eps:+.4g} component {i}: got {F[u, g, i]!r} "
                           f"want {float(f[i])!r} err {err[i]:.3e} bound {bound[i]:.3e}")
    return bad


FD_CPU_CASES = [("funnel", 257, [0.4, -0.3, 0.9]), ("noise", 300, [-0.25]), ("smooth", 129, [-3.0, -2.93]),
                ("normal_mean_var", 257, [0.3, -0.2, 0.5, -0.4]), ("offset_noise", 257, [0.3, -0.2, 0.5, -0.4])]


def _fd_oracle(O, model):
    """(context manager, the oracle's model name) for one of hp_reference.FD_MODELS."""
    import contextlib
    if model in ("normal_mean_var", "offset_noise"):
        return O.user_model(os.path.join(MODELS_DIR, model + ".h"), model), "user"
    return contextlib.nullcontext(), model


@pytest.mark.parametrize("model,N,theta0", FD_CPU_CASES)
def test_oracle_fd_values_within_the_derived_bound(O, model, N, theta0):
    """The oracle's finite-difference values against hp_reference.fd_value within fd_bound (derived in fd_value's docstring), without
    any kernel: both fiducial modes, offsets shared by the simulations and one row per unit, an offset of 0, a column range that
    begins and ends inside a Jacobian -- and every record g_converged at atol = 1e-8, the condition of the GPU test."""
    from oracle_problem import OracleBatchedProblem
    nth, nsims, G, atol, seed, s0 = len(theta0), 3, 3, 1e-8, 9, 4
    lo, hi = 1, nsims * nth - (1 if nth > 1 else 0)
    rng = np.random.default_rng(N)
    cm, name = _fd_oracle(O, model)
    with cm:
        orc = OracleBatchedProblem(None, name, nth, N=N, nthreads=1)
        for fid_mode in (0, 1):
            shared = rng.uniform(-0.05, 0.05, size=(nth, G))
            shared[:, 1] = 0.0
            F, info = orc.fd_values_columns(seed, s0, lo, hi, theta0, shared, atol=atol, fid_mode=fid_mode)
            assert not fd_mismatches(model, N, seed, s0, lo, hi, theta0, shared, False, F, info, atol, f"shared fid_mode {fid_mode}")
            per = rng.uniform(-0.05, 0.05, size=(hi - lo, G))
            F, info = orc.fd_values_columns(seed, s0, lo, hi, theta0, per, per_unit=True, atol=atol, fid_mode=fid_mode)
            assert not fd_mismatches(model, N, seed, s0, lo, hi, theta0, per, True, F, info, atol, f"per unit fid_mode {fid_mode}")


@pytest.mark.parametrize("model,N,theta0", FD_CPU_CASES)
def test_fd_bound_rejects_a_score_taken_at_the_perturbed_theta(O, model, N, theta0):
    """The negative control: the same draw and the same MAP at theta0, but the score evaluated at theta0 + eps e_j -- a recipe that
    two implementations can share.  The checker must refuse it (an offset of 0 aside, where the two recipes coincide)."""
    nth, atol, seed, s0 = len(theta0), 1e-8, 9, 4
    th = np.asarray(theta0, np.float64)
    off = np.tile([0.03, 0.0, -0.02], (nth, 1))
    cm, name = _fd_oracle(O, model)
    F = np.empty((nth, 3, nth))
    info = np.zeros((nth, 3), dtype=[("status", np.int32)])
    with cm:
        zfid = O.map_and_score_batch(name, N, seed, 2**40, 2**40 + 1, th, atol=atol, z0_mode=0)[1][0]
        for j in range(nth):
            for g in range(3):
                t = th.copy()
                t[j] = th[j] + off[j, g]
                x, _ = O.sample_x_z(name, N, seed, s0, t)
                zh, inf = O.zhat_at_theta(name, x, zfid, th, atol)
                assert inf["status"] == 0
                F[j, g] = O.grad_theta(name, x, zh, t)          # wrong on purpose: theta0 is what get_H! scores at
    bad = fd_mismatches(model, N, seed, s0, 0, nth, th, off, False, F, info, atol)
    assert bad and not [b for b in bad if " grid 1 " in b], bad
    assert all(any(f" column {j} grid {g} " in b for b in bad) for j in range(nth) for g in (0, 2)), bad
