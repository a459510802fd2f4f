"""An extended-precision reference of the engine's operators, restated from their documented definitions (the model comments of
csrc/models.hpp, models/cubic.h and models/normal_mean_var.h; the stream definition of csrc/rng.hpp and oracle/muse_oracle.c's
header).  It imports neither the oracle nor the package: what the oracle and the kernels share (the generator sequence, the fixed
exp, fma placement) is not shared here, so a wrong formula or constant on both of them shows up against it.

Arithmetic is numpy `longdouble` (x87 extended: 64-bit significand, u_ld = 2^-64); `log`, `cos`, `sin` and `exp` are the C
library's long-double functions.  Everything fp64 is rounded from an exact (to ~2^-63) value, so the reference's own error is
below 1/1000 of every bound written in 2^-53 below.

Rounding bounds.  Every operator returns, next to its value, a condition sum `cond` such that the fp64 evaluation of the same
formula is within C_ROUND * 2^-53 * cond of the value:
- an elementwise output (a gradient component) evaluated in k <= 8 fp64 operations, the 1-ulp exponential among them, is within
  k u (the expression evaluated on absolute values) of the exact one (Higham, "Accuracy and Stability", 3.1): cond is that
  absolute-value evaluation, and c = 8 would do;
- a reduced output (f, a score component) sums n such terms in any order: the per-term errors are bounded as above and the n
  roundings of the sum by lambda sqrt(n) u sum|t| except with probability 2 exp(-lambda^2 / 2) (Higham & Mary, SISC 41 (2019),
  the probabilistic bound); cond = sqrt(n) sum|t| (plus the absolute value of what is added after the sum), and lambda = 8
  gives a failure probability below 3e-14 per output.
So C_ROUND = 16 = 8 (per-term operations) + 8 (lambda) covers both.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                  # the fp64 unit roundoff
C_ROUND = 16                    # see the module docstring
PI = LD("3.14159265358979323846264338327950288419716939937510582")
HAVE_LD = np.finfo(LD).nmant >= 63
SKIP_REASON = "numpy longdouble has fewer than 64 significand bits on this platform (the reference needs x87 extended)"

MASK32 = np.uint64(0xFFFFFFFF)

PAIR_MODELS = ("normal_mean_var",)
MODELS = ("funnel", "noise", "smooth", "cubic", "normal_mean_var")


# ------------------------------------------------------------------------------------------------ the generator
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words: returns the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0 = M0 * c[0]
        p1 = M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK32, p1 & MASK32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK32, p0 & MASK32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK32
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK32
    return c


def uniforms(seed, sim, i):
    """(u1, u2) of elements i of simulation `sim`: key = (seed lo, seed hi), counter = (i lo, i hi, sim lo, sim hi),
    u = (k + 1/2) 2^-52 with k = the 52 bits (w_a << 20) | (w_b >> 12).  Exact in longdouble."""
    i = np.asarray(i, dtype=np.uint64)
    seed, sim = int(seed), int(sim)
    w = philox4x32_10(i & MASK32, i >> np.uint64(32), np.full(i.shape, sim & 0xFFFFFFFF, np.uint64),
                      np.full(i.shape, sim >> 32, np.uint64), seed & 0xFFFFFFFF, seed >> 32)
    k1 = (w[0] << np.uint64(20)) | (w[1] >> np.uint64(12))
    k2 = (w[2] << np.uint64(20)) | (w[3] >> np.uint64(12))
    scale = LD(2.0) ** -52
    return (k1.astype(LD) + LD(0.5)) * scale, (k2.astype(LD) + LD(0.5)) * scale


def normals(seed, sim, N, start=0):
    """(n1, n2, r) in longdouble: Box-Muller r = sqrt(-2 log u1), n1 = r cos(2 pi u2), n2 = r sin(2 pi u2)."""
    u1, u2 = uniforms(seed, sim, np.arange(start, start + N, dtype=np.uint64))
    r = np.sqrt(LD(-2) * np.log(u1))
    a = LD(2) * PI * u2
    return r * np.cos(a), r * np.sin(a), r


# ------------------------------------------------------------------------------------------------ blocks
def blocks(N, B):
    """Block of element i: floor(i B / N).  (An engine that pairs elements pads odd N with one element, and fills phantom slots
    of its last workgroup; neither is an element: they contribute nothing to any output.)"""
    return (np.arange(N, dtype=np.int64) * B) // N


def block_sizes(N, B):
    return np.bincount(blocks(N, B), minlength=B).astype(np.int64)


def _bsum(v, k, B):
    """Per-block sums of a longdouble vector (exact enough: longdouble accumulation)."""
    out = np.zeros(B, dtype=LD)
    np.add.at(out, k, v)
    return out


# ------------------------------------------------------------------------------------------------ models
def _stencil(v):
    """A v for the periodic (1/4, 1/2, 1/4) stencil (symmetric); np.roll makes N = 1, 2 wrap onto themselves."""
    return LD(0.25) * (np.roll(v, 1) + np.roll(v, -1)) + LD(0.5) * v


def _coefs(model, N, theta):
    """Per-element coefficients: (k, iv[k], mu[k] or 0, B, n_k, the constant's terms)."""
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    if model in PAIR_MODELS:
        K = th.size // 2
        k = blocks(N, K)
        n = block_sizes(N, K)
        return k, np.exp(-th[K:])[k], th[:K][k], K, n, n.astype(LD) * th[K:]
    B = 1 if model == "noise" else th.size
    k = blocks(N, B)
    n = block_sizes(N, B)
    if model == "noise":
        return k, np.full(N, np.exp(-th[0])), np.zeros(N, LD), 1, n, np.array([LD(N) * th[0]])
    return k, np.exp(-th)[k], np.zeros(N, LD), B, n, n.astype(LD) * th


def objective(model, x, z, theta):
    """f = -logLike (the engine's constant: 1/2 sum_k n_k theta_k, no 2 pi) and g = grad_z f, in longdouble, with cond_f (a
    scalar) and cond_g (per element).  x, z: fp64 arrays."""
    x, z = np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD)
    N = x.size
    k, iv, mu, B, n, cst = _coefs(model, N, theta)
    ax, az = np.abs(x), np.abs(z)
    if model == "noise":            # z ~ N(0,1), x ~ N(z, e^theta)
        r = x - z
        terms, tabs = z * z + iv * r * r, z * z + iv * r * r       # (r = x - z is one rounding of an exact difference)
        g = z - iv * r
        gabs = az + iv * np.abs(r)
    elif model == "smooth":         # z ~ N(0, e^theta_k), x = A z + n
        Az, Aaz = _stencil(z), _stencil(az)
        r = x - Az
        rabs = ax + Aaz
        terms, tabs = r * r + iv * z * z, rabs * rabs + iv * z * z
        g = iv * z - _stencil(r)
        gabs = iv * az + _stencil(rabs)
    elif model == "cubic":          # z ~ N(0, e^theta_k), x ~ N(h(z), 1), h = z + z^3/10
        h, hp = z + z ** 3 / LD(10), LD(1) + LD(3) * z * z / LD(10)
        r = x - h
        rabs = ax + az + az ** 3 / LD(10)
        terms, tabs = r * r + iv * z * z, rabs * rabs + iv * z * z
        g = iv * z - r * hp
        gabs = iv * az + rabs * hp
    else:                           # funnel: z ~ N(0, e^theta_k), x ~ N(z, 1); normal_mean_var: z ~ N(mu_k, e^tau_k), x ~ N(z, 1)
        r, d = x - z, z - mu
        dabs = az + np.abs(mu)
        terms, tabs = r * r + iv * d * d, r * r + iv * dabs * dabs
        g = iv * d - r
        gabs = iv * dabs + np.abs(r)
    f = LD(0.5) * (terms.sum() + cst.sum())
    cond_f = LD(0.5) * (np.sqrt(LD(N)) * tabs.sum() + np.abs(cst).sum())
    return f, g, cond_f, gabs


def score(model, x, z, theta):
    """grad_theta logLike at (x, z, theta) and its per-component cond.  x, z: fp64 arrays."""
    return _score_ld(model, np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD), theta)


def _score_ld(model, x, z, theta):
    """score on longdouble x, z as they are (fd_value's exact MAP is not an fp64 vector)."""
    N = x.size
    k, iv, mu, B, n, _ = _coefs(model, N, theta)
    nL, sq = n.astype(LD), np.sqrt(n.astype(LD))
    if model in PAIR_MODELS:        # d/dmu_k = iv_k sum (z - mu);  d/dtau_k = 1/2 (iv_k sum (z - mu)^2 - n_k)
        d, dabs = z - mu, np.abs(z) + np.abs(mu)
        ivk = _bsum(iv, k, B) / nL
        s = np.concatenate([ivk * _bsum(d, k, B), LD(0.5) * (ivk * _bsum(d * d, k, B) - nL)])
        c = np.concatenate([ivk * sq * _bsum(dabs, k, B), LD(0.5) * (ivk * sq * _bsum(dabs * dabs, k, B) + nL)])
        return s, c
    if model == "noise":
        r = x - z
        S = _bsum(r * r, k, 1)
    else:
        S = _bsum(z * z, k, B)
    ivk = _bsum(iv, k, B) / nL
    return LD(0.5) * (ivk * S - nL), LD(0.5) * (ivk * sq * S + nL)


def rounding(cond):
    """The stated bound on an fp64 evaluation of an output whose condition sum is `cond`."""
    return C_ROUND * U * np.asarray(cond, dtype=np.float64)


def diag_hessian(model, x, z, theta):
    """The diagonal of grad_z^2 f (longdouble)."""
    x, z = np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD)
    _, iv, _, _, _, _ = _coefs(model, x.size, theta)
    if model == "cubic":
        h, hp = z + z ** 3 / LD(10), LD(1) + LD(3) * z * z / LD(10)
        return iv + hp * hp - (x - h) * (LD(6) * z / LD(10))
    if model == "smooth":
        return iv + LD(0.375) if x.size >= 3 else iv + np.diag(_dense_A(x.size) @ _dense_A(x.size))
    return iv + LD(1)


def _dense_A(N):
    A = np.zeros((N, N), LD)
    for i in range(N):
        for o, w in ((-1, 0.25), (1, 0.25), (0, 0.5)):
            A[i, (i + o) % N] += LD(w)
    return A


# ------------------------------------------------------------------------------------------------ exact MAPs
def _smooth_solve(iv, b):
    """(A^T A + diag iv) v = b (A the periodic stencil, symmetric) to ~longdouble accuracy: a sparse fp64 LU and three steps of
    iterative refinement on longdouble residuals."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    N = b.size
    if N <= 4:
        A = _dense_A(N).astype(np.float64)
        Mat = sp.csc_matrix(A @ A + np.diag(iv.astype(np.float64)))
    else:
        e = np.ones(N)
        A = sp.diags([0.25 * e[:-1], 0.5 * e, 0.25 * e[:-1]], [-1, 0, 1], format="lil")
        A[0, N - 1] = 0.25
        A[N - 1, 0] = 0.25
        A = A.tocsc()
        Mat = (A @ A + sp.diags(iv.astype(np.float64))).tocsc()
    lu = spl.splu(Mat)
    v = lu.solve(b.astype(np.float64)).astype(LD)
    for _ in range(3):
        res = b - (_stencil(_stencil(v)) + iv * v)
        v = v + lu.solve(res.astype(np.float64)).astype(LD)
    return v


def exact_map(model, x, theta, z_start=None):
    """The MAP argmin_z f (longdouble): closed forms for the diagonal Gaussian models, a refined solve for smooth, and Newton
    steps from z_start (per element, longdouble) for cubic."""
    return _exact_map_ld(model, np.asarray(x, np.float64).astype(LD), theta, z_start)


def _exact_map_ld(model, x, theta, z_start=None):
    N = x.size
    _, iv, mu, _, _, _ = _coefs(model, N, theta)
    if model == "funnel":
        return x / (LD(1) + iv)
    if model == "noise":
        return iv * x / (LD(1) + iv)
    if model in PAIR_MODELS:
        return (x + iv * mu) / (LD(1) + iv)
    if model == "smooth":
        return _smooth_solve(iv, _stencil(x))
    assert model == "cubic" and z_start is not None
    return _cubic_polish(x, iv, np.asarray(z_start, np.float64).astype(LD))


def sample_x_z(model, N, seed, sim, theta):
    """(x, z) in longdouble from the reference's normals (the definitions of the models' draws)."""
    n1, n2, _ = normals(seed, sim, N)
    k, iv, mu, _, _, _ = _coefs(model, N, theta)
    sd = LD(1) / np.sqrt(iv)      # e^{theta/2}
    if model == "noise":
        return n1 + sd * n2, n1
    z = mu + sd * n1
    if model == "smooth":
        return _stencil(z) + n2, z
    if model == "cubic":
        return z + z ** 3 / LD(10) + n2, z
    return z + n2, z


# ------------------------------------------------------------------------------------------------ implicit-differentiation H
def implicit_H(model, N, seed, sim, theta0, zhat_start=None):
    """get_H!'s implicit-differentiation H of one simulation at the exact MAP (Newton-polished from zhat_start for cubic):
    H = H1 - dFdth^T A^{-1} dFdth1 with A = grad_z^2 logLike(x, zhat, theta0), dFdth = d/dtheta grad_z logLike(x, zhat, theta),
    dFdth1 = d/dtheta grad_z logLike(x(theta), zhat, theta0) and H1 = d/dtheta score(x(theta), zhat, theta0), x(theta) drawn at
    fixed normals.  Only the ntheta right-hand sides are solved for (A is diagonal, or the stencil's A^T A + diag iv)."""
    th = np.asarray(theta0, dtype=np.float64)
    B = th.size
    x, zt = sample_x_z(model, N, seed, sim, th)
    k, iv, _, _, _, _ = _coefs(model, N, th)
    if model == "cubic":   # Newton on the longdouble x itself
        zh = _cubic_polish(x, iv, np.asarray(zhat_start, np.float64).astype(LD))
    elif model == "smooth":
        zh = _smooth_solve(iv, _stencil(x))
    elif model == "funnel":
        zh = x / (LD(1) + iv)
    else:
        zh = iv * x / (LD(1) + iv)
    H = np.zeros((B, B), LD)
    if model == "noise":
        dxdth = LD(0.5) * (x - zt)
        d = x - zh
        H1 = iv[0] * np.sum(d * dxdth)
        dF = -iv * d                       # dFdth (one column)
        dF1 = iv * dxdth                   # dFdth1
        Ainv_dF1 = -dF1 / (iv + LD(1))
        H[0, 0] = H1 - np.sum(dF * Ainv_dF1)
        return H
    for j in range(B):
        m = (k == j).astype(LD)
        if model == "funnel":
            dF1 = LD(0.5) * zt * m
            v = -dF1 / (LD(1) + iv)
        elif model == "smooth":
            dF1 = _stencil(_stencil(LD(0.5) * zt * m))
            v = -_smooth_solve(iv, dF1)
        else:   # cubic: dx/dtheta_k = 1/2 h'(z_true) z_true on block k; d/dx grad_z logLike = h'(zhat)
            hpz = LD(1) + LD(3) * zh * zh / LD(10)
            hpt = LD(1) + LD(3) * zt * zt / LD(10)
            dF1 = hpz * (LD(0.5) * hpt * zt) * m
            h = zh + zh ** 3 / LD(10)
            v = -dF1 / (iv + hpz * hpz - (x - h) * (LD(6) * zh / LD(10)))
        for i2 in range(B):
            dF = iv * zh * (k == i2)           # d/dtheta_i2 (-iv z) = iv z on block i2
            H[i2, j] = -np.sum(dF * v)
    return H


def _cubic_polish(x, iv, z):
    for _ in range(8):
        h, hp = z + z ** 3 / LD(10), LD(1) + LD(3) * z * z / LD(10)
        g = iv * z - (x - h) * hp
        z = z - g / (iv + hp * hp - (x - h) * (LD(6) * z / LD(10)))
    return z


# ------------------------------------------------------------------------------------------------ finite-difference get_H! values
FD_MODELS = ("funnel", "noise", "smooth", "normal_mean_var", "offset_noise")


def fd_value(model, N, seed, sim, theta0, j, eps):
    """One value of get_H!'s finite-difference map (src/muse.jl:426-432) and what its bound needs: returns (f, aux) with

        f(eps) = grad_theta logLike( x(theta0 + eps e_j; the simulation's normals), z*(x; theta0), theta0 )          (longdouble [ntheta])

    x drawn at the perturbed theta from the normals of (seed, sim), z* the EXACT MAP at theta0 of that draw (closed form; the
    refined solve for smooth), the score at theta0.  The perturbed component is the fp64 sum theta0[j] + eps -- the engine forms
    that sum in fp64, so it is the input -- converted to longdouble afterwards; everything else is longdouble (x and z* are not
    rounded to fp64 on the way).  Models: FD_MODELS, the Gaussian ones; offset_noise (models/offset_noise.h) draws and solves through
    tests/pair_implicit_reference.py.  cubic is left with the oracle: the finite-difference entry returns no MAP to polish from, and
    without one the cubic model has no exact MAP here (exact_map needs a z_start inside the right basin).

    fd_bound(aux, atol) bounds |engine's value - f| per component for a unit whose record says status == 0 (g_converged).  It is
    derived, not fitted, after points (b) and (c) of test_gpu_stencil.test_get_H_branches_against_the_dense_H:

    1. The kernel stops on its own fp64 gradient, |g_fp64|_inf <= atol, and that is within gb = rounding(cond_g).max() of the true
       gradient at its MAP zhat: |grad f(zhat)|_inf <= atol + gb.  (cond_g is evaluated at z*; at zhat it differs by O(dz) of it.)
    2. f is quadratic in z with Hessian Hz, so zhat - z* = Hz^-1 grad f(zhat).  Diagonal models: per element
       dz_i <= (atol + gb) / H_ii, H_ii = 1 + iv_i (diag_hessian).  smooth: |dz|_2 <= sqrt(N) (atol + gb) / lambda_min with
       lambda_min >= e^{-max theta0} (A^T A is positive semi-definite).
    3. Every score component is a quadratic in z, so its change over dz is bounded exactly.  With q_i the absolute value of the
       quadratic's argument at z* (|z*_i| for funnel and smooth, |x_i - z*_i| for noise, |z*_i - mu_k| for normal_mean_var,
       |x_i - z*_i - mu_k| for offset_noise) a component 1/2 (iv_k sum q^2 - n_k) moves by at most
           iv_k (sum_i q_i dz_i + 1/2 sum_i dz_i^2)                 -- for smooth by Cauchy-Schwarz  iv_k (|q_k|_2 D + 1/2 D^2), D = |dz|_2,
       and the pair models' linear component iv_k sum (+-)(argument) by at most iv_k sum_i dz_i.
    4. The kernel's fp64 evaluation of the score at zhat is within rounding(cond_score) of the exact one, cond evaluated on
       |z*| + dz (on |q_k|_2 + D for smooth), which covers zhat.
    The bound is the sum of 3 and 4: no other slack, no constant from running a kernel.  (Not in it: the engine's draw differs from
    the reference's by the generator's K_GEN 2^-52 max(1, r) per normal and one ulp of exp(theta/2), some 1e-7 of atol at the
    atol = 1e-8 the tests use; a solve reports g_converged at |g|_inf <= atol, not within 1e-15 of it.)"""
    assert model in FD_MODELS
    th0 = np.atleast_1d(np.asarray(theta0, dtype=np.float64))
    thp = th0.copy()
    thp[j] = th0[j] + np.float64(eps)                  # the fp64 sum: the input
    if model == "offset_noise":
        import pair_implicit_reference as P
        x, zt, _, _ = P.sample(model, N, seed, sim, thp)
        zs = P.exact_map(model, x, zt, N, th0)
        th = th0.astype(LD)
        K = th.size // 2
        k, n = blocks(N, K), block_sizes(N, K)
        mu, iv = th[:K][k], np.exp(-th[K:])[k]
        r = x - zs - mu
        f = np.concatenate([_bsum(iv * r, k, K), LD(0.5) * (_bsum(iv * r * r, k, K) - n.astype(LD))])
        q, qa = np.abs(r), np.abs(x) + np.abs(zs) + np.abs(mu)
        gabs = np.abs(zs) + iv * qa                    # grad_z (1/2 o) = z - iv r on absolute values
        hdiag = LD(1) + iv
        pair = True
    else:
        x, _ = sample_x_z(model, N, seed, sim, thp)
        zs = _exact_map_ld(model, x, th0)
        f, _ = _score_ld(model, x, zs, th0)
        k, iv, mu, K, n, _ = _coefs(model, N, th0)
        gabs = objective(model, x, zs, th0)[3]
        hdiag = None if model == "smooth" else iv + LD(1)
        pair = model in PAIR_MODELS
        if model == "noise":
            q = qa = np.abs(x - zs)
        elif pair:
            q, qa = np.abs(zs - mu), np.abs(zs) + np.abs(mu)
        else:
            q = qa = np.abs(zs)
    f64 = lambda v: np.asarray(v, dtype=np.float64)
    aux = dict(model=model, N=N, K=K, k=k, n=f64(n), iv=f64(_bsum(iv, k, K)) / f64(n), q=f64(q), qa=f64(qa), gabs=f64(gabs),
               hdiag=None if hdiag is None else f64(hdiag), pair=pair, lam_min=float(np.exp(-np.max(th0))), x=x, zs=zs)
    return f, aux


def fd_bound(aux, atol):
    """|engine's fd value - fd_value's f| per component for a status == 0 unit: points 1-4 of fd_value's docstring."""
    k, K, n, iv, q, qa = aux["k"], aux["K"], aux["n"], aux["iv"], aux["q"], aux["qa"]
    ga = atol + float(rounding(aux["gabs"]).max())                    # 1.
    bs = lambda v: np.bincount(k, weights=v, minlength=K)
    if aux["model"] == "smooth":                                      # 2., 3. (Cauchy-Schwarz), 4. on |q_k|_2 + D
        D = np.sqrt(aux["N"]) * ga / aux["lam_min"]
        q2 = np.sqrt(bs(q * q))
        return iv * (q2 * D + 0.5 * D * D) + rounding(0.5 * (iv * np.sqrt(n) * (q2 + D) ** 2 + n))
    dz = ga / aux["hdiag"]                                            # 2.
    quad = iv * (bs(q * dz) + 0.5 * bs(dz * dz)) + rounding(0.5 * (iv * np.sqrt(n) * bs((qa + dz) ** 2) + n))
    if not aux["pair"]:
        return quad
    lin = iv * bs(dz) + rounding(iv * np.sqrt(n) * bs(qa + dz))
    return np.concatenate([lin, quad])
