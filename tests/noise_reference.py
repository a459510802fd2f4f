"""An extended-precision reference of the stencil model with a noise variance per element and a mask (muse_set_noise), restated
from its definition:

    z_i ~ N(0, e^{theta_k(i)}),   x_i = (A z)_i + s_i n2_i,   (A z)_i = w1 (z_{i-1} + z_{i+1}) + w0 z_i  (periodic)
    s_i = sd_i where observed, 0 where masked;   omega_i = 1 / (sd_i sd_i) where observed, 0 where masked
    f = -logLike = 1/2 sum_i omega_i r_i^2 + 1/2 sum_i e^{-theta_k} z_i^2 + 1/2 sum_k n_k theta_k,   r = x - A z
    grad_z f = e^{-theta} z - A^T (omega r),   Hessian_z f = A^T Omega A + diag(e^{-theta})
    score_k = 1/2 (e^{-theta_k} sum_{i in k} z_i^2 - n_k)          (unchanged: the noise does not depend on theta)

Built on tests/stencil_reference.py (the operator, the dense longdouble Cholesky) and tests/hp_reference.py (the generator, the block
map, the rounding-bound scheme); it imports neither the oracle nor the package.  The oracle knows nothing of Omega: this module is
the checker, and at sd = 1 without a mask it must equal stencil_reference exactly (tests/test_noise_reference.py).

omega is formed as the engine's host code forms it -- fp64 sd, the fp64 product sd sd, the fp64 quotient 1 / (sd sd): two rounded
operations -- and then taken as an exact number: the model the kernels are held to is the one with THAT omega, so the two roundings
are part of the statement of the model, not of the error budget.

Bounds, derived from atol and the fp64 rounding alone:

* Rounding.  hp_reference's scheme: every operator returns a condition sum `cond` with |fp64 - exact| <= C_ROUND 2^-53 cond.
  The weighted expressions have ONE more multiply per term than stencil_reference's (omega r), still below the 8 operations per
  term that C_ROUND = 16 allows for: cond_g = e^{-theta} |z| + |A| (omega (|x| + |A| |z|)), cond_f = 1/2 (sqrt(N) sum_i (omega_i
  rabs_i^2 + e^{-theta} z_i^2) + |sum_k n_k theta_k|).
* The draw.  x_i = fma(s_i, n2_i, (A z)_i): cond_x = |A| |z| + s |n2|; a masked element's x is EXACTLY 0.
* The MAP.  A solve that ends g_converged at tolerance atol leaves |g(zhat)|_inf <= atol + rounding(cond_g), and
  zhat - z* = H^-1 g(zhat) with H = A^T Omega A + diag(e^{-theta}).  A^T Omega A is positive semi-definite (omega >= 0), so
  lambda_min(H) >= min_k e^{-theta_k} (Weyl) whatever the mask hides, and |zhat - z*|_inf <= |zhat - z*|_2 <= |g|_2 / lambda_min.
  The GPU tests assert |zhat - z*|_inf <= 2 atol / lambda_min: atol carried through lambda_min, the factor 2 the room for
  rounding(cond_g) next to atol (below 1e-3 atol at atol = 1e-8 and the tests' sizes) and for |H^-1|_inf against |H^-1|_2 of a
  banded, diagonally weighted H.  z* is exact_map: the dense longdouble Cholesky for N <= 400 and, matrix-free, longdouble
  conjugate gradients to a residual of 1e-16 |b| beyond (|z*_cg - z*|_2 <= 1e-16 |A^T Omega x|_2 / lambda_min, below 1e-5 atol);
  tests/test_noise_reference.py holds the two against each other.
* Scores at the engine's MAP: hp_reference.score's rounding bound (the score's formula is unchanged).  Scores at the EXACT MAP
  differ from those at zhat by at most e^{-theta_k} (|z*|_1 dz + n_k dz^2 / 2) over the block, dz the max-norm distance above.
* implicit_H: column j is -dFdth^T v_j, v_j = -H^-1 A^T Omega A (1/2 z_true 1_j), dFdth_i = e^{-theta_i} zhat 1_i.  CG stops at
  |r| <= sqrt(eps) |b|: |v - v*|_2 <= kappa sqrt(eps) |v*|_2, kappa = lambda_max / lambda_min with lambda_max <= max omega max_q
  a_q^2 + max_k e^{-theta_k} and lambda_min >= min_k e^{-theta_k}; with zhat within dz of the exact MAP and the sum's rounding:
      |dH_ij| <= e^{-theta_i} (|zhat_i|_2 kappa sqrt(eps) |v*_j|_2 + dz |v*_j|_1) (1 + kappa sqrt(eps)) + C_ROUND 2^-53 sqrt(n_i) sum |terms|
  (implicit_H_bound below evaluates it).
* The marginal posterior (the model is jointly Gaussian): over the OBSERVED elements x_o ~ N(0, C), C = A_o diag(e^theta) A_o^T +
  diag(sd_o^2); d log p / d theta_k = 1/2 (y^T D_k y - tr(C^-1 D_k)), y = C^-1 x_o, D_k = e^{theta_k} A_o 1_k A_o^T.  With the
  identity y = Omega_o (x_o - A_o z*) and A^T Omega r = e^{-theta} z* at the MAP this is 1/2 (e^{-theta_k} sum_k z*^2 - e^{theta_k}
  tr_k(A^T (Omega - Omega A H'^-1 A^T Omega) A)), evaluated densely here (N <= 400) and, for the sizes muse() runs at, by the
  expectation's Monte-Carlo estimate with its own error (marginal_gradient_mc)."""
import numpy as np

import hp_reference as R
import stencil_reference as S

LD = R.LD
BUILTIN = S.BUILTIN


def weights(N, sd=None, mask=None):
    """(omega, s) in longdouble as the engine's host code forms them from fp64 sd and the mask: omega = 1.0 / (sd * sd), two
    rounded fp64 operations, s = sd; both 0 where masked."""
    sd = np.ones(N) if sd is None else np.broadcast_to(np.asarray(sd, np.float64), (N,)).copy()
    m = np.ones(N, bool) if mask is None else np.asarray(mask).astype(bool)
    assert sd.shape == (N,) and m.shape == (N,) and np.all(np.isfinite(sd)) and np.all(sd > 0)
    var = sd * sd                                   # fp64, rounded
    om = np.where(m, 1.0 / var, 0.0)                # fp64, rounded
    return om.astype(LD), np.where(m, sd, 0.0).astype(LD)


def objective(x, z, theta, w, omega):
    """f = -logLike, g = grad_z f, cond_f, cond_g -- as stencil_reference.objective, the residual weighted."""
    x, z = np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD)
    # (a masked element's x enters nothing: whatever it holds -- 1e30, inf, nan -- is dropped before any arithmetic)
    x = np.where(omega != 0, x, LD(0))
    N = x.size
    k, iv, B, n, cst = S._coefs(N, theta)
    ax, az = np.abs(x), np.abs(z)
    r = x - S.stencil(z, w)
    rabs = ax + S.stencil_abs(az, w)
    q, qabs = omega * r, omega * rabs
    terms, tabs = q * r + iv * z * z, qabs * rabs + iv * z * z
    g = iv * z - S.stencil(q, w)
    gabs = iv * az + S.stencil_abs(qabs, w)
    f = LD(0.5) * (terms.sum() + cst.sum())
    cond_f = LD(0.5) * (np.sqrt(LD(N)) * tabs.sum() + np.abs(cst).sum())
    return f, g, cond_f, gabs


def score(x, z, theta):
    return S.score(x, z, theta)


def sample_x_z(N, seed, sim, theta, w, s):
    """(x, z, cond_x): x = A z + s n2, exactly 0 where masked (s = 0); cond_x = |A| |z| + s |n2|."""
    n1, n2, _ = R.normals(seed, sim, N)
    k, iv, _, _, _ = S._coefs(N, theta)
    z = (LD(1) / np.sqrt(iv)) * n1
    x = np.where(s != 0, S.stencil(z, w) + s * n2, LD(0))
    return x, z, S.stencil_abs(np.abs(z), w) + s * np.abs(n2)


def hessian(N, theta, w, omega):
    """A^T Omega A + diag(e^{-theta}): smallest eigenvalue >= min_k e^{-theta_k}."""
    A = S.dense_A(N, w)
    _, iv, _, _, _ = S._coefs(N, theta)
    return A.T @ (omega[:, None] * A) + np.diag(iv)


def hess_apply(v, iv, w, omega):
    return S.stencil(omega * S.stencil(v, w), w) + iv * v


def cg_solve(iv, w, omega, b, rtol=LD(1e-16), maxiter=5000):
    """H v = b by longdouble conjugate gradients, matrix-free (any N): stops at |r|_2 <= rtol |b|_2 (the longdouble unit roundoff is
    5e-20: the recurrence's residual is the true one to ~1e-18 |b| kappa), so |v - v*|_2 <= rtol |b|_2 / lambda_min."""
    tol = rtol * np.sqrt(np.dot(b, b))
    v = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr = np.dot(r, r)
    for _ in range(maxiter):
        if np.sqrt(rr) <= tol:
            break
        Ap = hess_apply(p, iv, w, omega)
        al = rr / np.dot(p, Ap)
        v = v + al * p
        r = r - al * Ap
        rn = np.dot(r, r)
        p = r + (rn / rr) * p
        rr = rn
    assert np.sqrt(rr) <= tol, float(np.sqrt(rr))
    return v


def exact_map(x, theta, w, omega, dense=None):
    """z* = H^-1 A^T Omega x: the dense longdouble Cholesky for N <= 400, longdouble conjugate gradients (residual 1e-16 |b|) beyond."""
    x = np.where(omega != 0, np.asarray(x, np.float64).astype(LD), LD(0))
    N = x.size
    b = S.stencil(omega * x, w)
    if dense is None:
        dense = N <= 400
    if dense:
        return S.chol_solve(S.cholesky(hessian(N, theta, w, omega)), b)
    _, iv, _, _, _ = S._coefs(N, theta)
    return cg_solve(iv, w, omega, b)


def score_at_exact_map(x, theta, w, omega):
    """(score(z*), z*) in longdouble."""
    zs = exact_map(x, theta, w, omega)
    k, iv, B, n, _ = S._coefs(zs.size, theta)
    return LD(0.5) * (np.exp(-np.asarray(theta, np.float64).astype(LD)) * R._bsum(zs * zs, k, B) - n.astype(LD)), zs


def implicit_H(N, seed, sim, theta0, w, omega, s, zhat=None, dense=None):
    """get_H!'s per-simulation H: column j is -dFdth^T v_j with v_j = -H^-1 A^T Omega A (1/2 z_true 1_j), dFdth_i = iv zhat 1_i;
    zhat = the exact MAP unless given.  Returns (H, |v_j| for the bound)."""
    th = np.asarray(theta0, dtype=np.float64)
    B = th.size
    x, zt, _ = sample_x_z(N, seed, sim, th, w, s)
    k, iv, _, _, _ = S._coefs(N, th)
    if dense is None:
        dense = N <= 400
    if dense:
        L = S.cholesky(hessian(N, th, w, omega))
        solve = lambda b: S.chol_solve(L, b)
    else:
        solve = lambda b: cg_solve(iv, w, omega, b)
    zh = solve(S.stencil(omega * x, w)) if zhat is None else np.asarray(zhat, np.float64).astype(LD)
    H = np.zeros((B, B), LD)
    vs = []
    for j in range(B):
        v = -solve(S.stencil(omega * S.stencil(LD(0.5) * zt * (k == j), w), w))
        vs.append(np.abs(v))
        for i in range(B):
            H[i, j] = -np.sum(iv * zh * (k == i) * v)
    return H, vs, zh


def implicit_H_bound(theta, w, omega, zh, vs, dz):
    """The bound of the module docstring, entry by entry [i, j]."""
    th = np.asarray(theta, np.float64)
    N, B = zh.size, th.size
    k, iv = R.blocks(N, B), np.exp(-th)
    aq2 = float((S.a_q(N, w) ** 2).max())
    kse = (float(omega.max()) * aq2 + iv.max()) / iv.min() * np.sqrt(np.finfo(float).eps)
    out = np.zeros((B, B))
    for j in range(B):
        v = vs[j].astype(np.float64)
        for i in range(B):
            m = k == i
            za = np.abs(zh[m]).astype(np.float64)
            out[i, j] = iv[i] * (np.linalg.norm(za) * kse * np.linalg.norm(v) + dz * v[m].sum()) * (1 + kse) \
                + R.C_ROUND * R.U * np.sqrt(m.sum()) * (iv[i] * za * v[m]).sum()
    return out


def expected_information(N, theta, w, omega):
    """E[score score^T] of the marginal likelihood = 1/2 tr(C^-1 D_i C^-1 D_j) over the observed elements (dense, N <= 400)."""
    th = np.asarray(theta, np.float64).astype(LD)
    B = th.size
    k = R.blocks(N, B)
    obs = np.asarray(omega != 0)
    A = S.dense_A(N, w)[obs]
    Cm = A @ (np.exp(th)[k][:, None] * A.T) + np.diag(LD(1) / omega[obs])
    L = S.cholesky(Cm)
    Ms = []
    for j in range(B):
        D = A @ ((np.exp(th[j]) * (k == j))[:, None] * A.T)
        Ms.append(np.stack([S.chol_solve(L, D[:, c]) for c in range(D.shape[1])], axis=1))
    return np.array([[float(LD(0.5) * np.trace(Ms[i] @ Ms[j])) for j in range(B)] for i in range(B)])


def marginal_gradient(x, theta, w, omega):
    """d log p(x | theta) / d theta, exact (dense longdouble, N <= 400): 1/2 (y^T D_k y - tr(C^-1 D_k)) over the observed elements."""
    th = np.asarray(theta, np.float64).astype(LD)
    B = th.size
    N = np.asarray(x).size
    k = R.blocks(N, B)
    obs = np.asarray(omega != 0)
    xo = np.asarray(x, np.float64).astype(LD)[obs]
    A = S.dense_A(N, w)[obs]
    Cm = A @ (np.exp(th)[k][:, None] * A.T) + np.diag(LD(1) / omega[obs])
    L = S.cholesky(Cm)
    y = S.chol_solve(L, xo)
    out = np.zeros(B, LD)
    for j in range(B):
        D = A @ ((np.exp(th[j]) * (k == j))[:, None] * A.T)
        tr = sum(S.chol_solve(L, D[:, c])[c] for c in range(D.shape[1]))
        out[j] = LD(0.5) * (np.dot(y, D @ y) - tr)
    return out


def marginal_gradient_mc(x, theta, w, omega, s, seed, nsims):
    """The same gradient at any N as MUSE's own identity in exact arithmetic: score(z*(x)) - E_sims[score(z*(x_sim))], the
    expectation by `nsims` longdouble simulations (for a jointly Gaussian model the MUSE score IS the marginal score); returns
    (estimate, its Monte-Carlo standard error per component)."""
    th = np.asarray(theta, np.float64)
    N = np.asarray(x).size
    sd, _ = score_at_exact_map(x, th, w, omega)
    sims = np.array([score_at_exact_map(sample_x_z(N, seed, i, th, w, s)[0].astype(np.float64), th, w, omega)[0].astype(np.float64)
                     for i in range(nsims)])
    return sd.astype(np.float64) - sims.mean(axis=0), sims.std(axis=0, ddof=1) / np.sqrt(nsims)


def marginal_gradient_latent(x, theta, w, omega):
    """The same gradient in fp64 at the sizes muse() runs at (N up to ~10^4), from the latent side: E[z z^T | x] = z* z*^T + H^-1, so
    d log p(x | theta) / d theta_k = 1/2 (e^{-theta_k} (sum_{i in k} z*_i^2 + tr_k H^-1) - n_k); H is the periodic pentadiagonal
    Hessian, factorised sparsely.  (fp64: for mode finding against a Monte-Carlo error, not for rounding bounds;
    tests/test_noise_reference.py holds it to the dense longdouble marginal_gradient.)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    th = np.asarray(theta, np.float64)
    x = np.asarray(x, np.float64)
    N, B = x.size, th.size
    k = R.blocks(N, B)
    om = np.asarray(omega, np.float64)
    x = np.where(om != 0, x, 0.0)
    i = np.arange(N)
    A = sp.csc_matrix((np.concatenate([np.full(N, float(w[0])), np.full(N, float(w[1])), np.full(N, float(w[1]))]),
                       (np.concatenate([i, i, i]), np.concatenate([i, (i - 1) % N, (i + 1) % N]))), shape=(N, N))
    H = (A.T @ sp.diags(om) @ A + sp.diags(np.exp(-th)[k])).tocsc()
    zs = spl.splu(H).solve(A.T @ (om * x))
    dH = _diag_of_inverse(H)
    n = R.block_sizes(N, B).astype(np.float64)
    return 0.5 * (np.exp(-th) * np.array([np.sum((zs * zs + dH)[k == b]) for b in range(B)]) - n)


def _diag_of_inverse(H):
    """diag(H^-1) of a symmetric positive definite matrix with cyclic bandwidth 2 (N >= 8), in O(N): the last two indices are a
    border, the rest is banded -- H = [[Bm, U], [U^T, D]], (H^-1)_II = Bm^-1 + (Bm^-1 U) S^-1 (Bm^-1 U)^T, (H^-1)_bb = S^-1,
    S = D - U^T Bm^-1 U -- with LAPACK's banded Cholesky of Bm."""
    from scipy.linalg import cholesky_banded, cho_solve_banded
    N = H.shape[0]
    n = N - 2
    Hi = H[:n, :n]
    ab = np.zeros((3, n))
    for d in range(3):
        ab[2 - d, d:] = Hi.diagonal(d)
    cb = cholesky_banded(ab)
    U = H[:n, n:].toarray()
    D = H[n:, n:].toarray()
    BU = cho_solve_banded((cb, False), U)
    Sinv = np.linalg.inv(D - U.T @ BU)
    # diag(Bm^-1) by the Takahashi recurrence on Bm = R^T R (R upper, bandwidth 2): R Z = R^-T is lower triangular with diagonal
    # 1 / R_ii, so for j >= i: Z_ij = (delta_ij / R_ii - sum_{k > i} R_ik Z_kj) / R_ii -- the band of Z from the last row upwards
    r0, r1, r2 = cb[2], np.append(cb[1][1:], [0.0]), np.append(cb[0][2:], [0.0, 0.0])      # R_ii, R_i,i+1, R_i,i+2
    z0, z1, z2 = np.zeros(n + 2), np.zeros(n + 2), np.zeros(n + 2)                          # Z_ii, Z_i,i+1, Z_i,i+2
    for i in range(n - 1, -1, -1):
        z1[i] = -(r1[i] * z0[i + 1] + r2[i] * z1[i + 1]) / r0[i]
        z2[i] = -(r1[i] * z1[i + 1] + r2[i] * z0[i + 2]) / r0[i]
        z0[i] = (1.0 / r0[i] - r1[i] * z1[i] - r2[i] * z2[i]) / r0[i]
    out = np.empty(N)
    out[:n] = z0[:n]
    out[:n] += np.einsum("ia,ab,ib->i", BU, Sinv, BU)
    out[n:] = np.diag(Sinv)
    return out


def posterior_mode(x, w, omega, B, prior_sigma):
    """(mode, sigma) of the exact marginal posterior with the prior theta_k ~ N(0, prior_sigma^2): the root of marginal_gradient_latent
    - theta / prior_sigma^2 (scipy's hybrid Powell), sigma = sqrt(diag(-Hessian^-1)) by central differences of the gradient there."""
    from scipy.optimize import root
    f = lambda t: marginal_gradient_latent(x, t, w, omega) - np.asarray(t) / prior_sigma ** 2
    sol = root(f, np.zeros(B), tol=1e-10)
    assert sol.success, sol.message
    mode, h = sol.x, 1e-4
    J = np.empty((B, B))
    for j in range(B):
        e = np.zeros(B)
        e[j] = h
        J[:, j] = (f(mode + e) - f(mode - e)) / (2 * h)
    return mode, np.sqrt(np.diag(np.linalg.inv(-0.5 * (J + J.T))))
