"""An extended-precision reference of the stencil model with run-time weights (muse_set_stencil), restated from its definition:

    z_i ~ N(0, e^{theta_k(i)}),   x = A z + n,   (A z)_i = w1 (z_{i-1} + z_{i+1}) + w0 z_i  (periodic),   n_i ~ N(0, 1)
    score_k = 1/2 (e^{-theta_k} sum_{i in k} z_i^2 - n_k)

Built on tests/hp_reference.py's generator, block map and rounding-bound scheme (C_ROUND 2^-53 cond: its docstring derives the
constant); it imports neither the oracle nor the package.  The oracle's own stencil is fixed at (1/4, 1/2, 1/4): this module is the
checker for every other pair, and at that pair it must equal hp_reference's `smooth` operators (tests/test_stencil_reference.py).

Dense algebra (N <= 400) is longdouble throughout: a Cholesky factorisation written out here, since numpy's LAPACK front end is
fp64.  The per-term operation count of a stencil expression with two weights is the built-in's plus two multiplies that were
exact scalings by powers of two -- still below the 8 operations per term that C_ROUND = 16 allows for."""
import numpy as np

import hp_reference as R

LD = R.LD
BUILTIN = (0.5, 0.25)


def _w(w):
    return LD(float(w[0])), LD(float(w[1]))          # the engine's weights are fp64 numbers


def stencil(v, w):
    """A v (A is symmetric); np.roll makes the wrap."""
    w0, w1 = _w(w)
    return w1 * (np.roll(v, 1) + np.roll(v, -1)) + w0 * v


def stencil_abs(v, w):
    """|A| |v|: the condition sum of A v."""
    w0, w1 = _w(w)
    return np.abs(w1) * (np.roll(v, 1) + np.roll(v, -1)) + np.abs(w0) * v


def dense_A(N, w):
    w0, w1 = _w(w)
    A = np.zeros((N, N), LD)
    for i in range(N):
        A[i, i] += w0
        A[i, (i - 1) % N] += w1
        A[i, (i + 1) % N] += w1
    return A


def _coefs(N, theta):
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    k = R.blocks(N, th.size)
    n = R.block_sizes(N, th.size)
    return k, np.exp(-th)[k], th.size, n, n.astype(LD) * th


def objective(x, z, theta, w):
    """f = -logLike (constant 1/2 sum_k n_k theta_k), g = grad_z f, cond_f, cond_g -- as hp_reference.objective."""
    x, z = np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD)
    N = x.size
    k, iv, B, n, cst = _coefs(N, theta)
    ax, az = np.abs(x), np.abs(z)
    r = x - stencil(z, w)
    rabs = ax + stencil_abs(az, w)
    terms, tabs = r * r + iv * z * z, rabs * rabs + iv * z * z
    g = iv * z - stencil(r, w)
    gabs = iv * az + stencil_abs(rabs, w)
    f = LD(0.5) * (terms.sum() + cst.sum())
    cond_f = LD(0.5) * (np.sqrt(LD(N)) * tabs.sum() + np.abs(cst).sum())
    return f, g, cond_f, gabs


def score(x, z, theta):
    """grad_theta logLike and its cond: the weights do not enter (hp_reference's `smooth` score)."""
    return R.score("smooth", x, z, theta)


def sample_x_z(N, seed, sim, theta, w):
    """(x, z, cond_x) in longdouble from hp_reference's normals; cond_x = |A| |z| + |n2| bounds the fp64 evaluation of x."""
    n1, n2, _ = R.normals(seed, sim, N)
    k, iv, _, _, _ = _coefs(N, theta)
    z = (LD(1) / np.sqrt(iv)) * n1      # e^{theta/2} n1
    return stencil(z, w) + n2, z, stencil_abs(np.abs(z), w) + np.abs(n2)


# ------------------------------------------------------------------------------------------------ dense algebra in longdouble
def cholesky(Mat):
    """Lower Cholesky factor of a symmetric positive definite longdouble matrix (row by row, vectorised inner products)."""
    n = Mat.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = Mat[j, j] - np.dot(L[j, :j], L[j, :j])
        assert d > 0
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (Mat[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def chol_solve(L, b):
    n = b.shape[0]
    y = np.zeros_like(b, dtype=LD)
    for i in range(n):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    v = np.zeros_like(y)
    for i in range(n - 1, -1, -1):
        v[i] = (y[i] - np.dot(L[i + 1:, i], v[i + 1:])) / L[i, i]
    return v


def hessian(N, theta, w):
    """grad_z^2 f = A^T A + diag(e^{-theta}): symmetric, smallest eigenvalue >= min_k e^{-theta_k} (A^T A is positive semi-definite)."""
    A = dense_A(N, w)
    _, iv, _, _, _ = _coefs(N, theta)
    return A.T @ A + np.diag(iv)


def exact_map(x, theta, w):
    """z* = (A^T A + diag e^{-theta})^-1 A^T x by a dense longdouble solve (N <= 400)."""
    x = np.asarray(x).astype(LD)
    assert x.size <= 400
    L = cholesky(hessian(x.size, theta, w))
    return chol_solve(L, stencil(x, w))


def a_q(N, w):
    """Eigenvalues of the circulant A: w0 + 2 w1 cos(2 pi q / N)."""
    w0, w1 = _w(w)
    return w0 + LD(2) * w1 * np.cos(LD(2) * R.PI * np.arange(N).astype(LD) / LD(N))


def marginal_dense(x, theta, w):
    """log p(x | theta) + N/2 log 2 pi for ONE theta: x ~ N(0, C), C = e^theta A A^T + I -- dense longdouble."""
    x = np.asarray(x).astype(LD)
    N = x.size
    A = dense_A(N, w)
    Cm = np.exp(LD(float(theta))) * (A @ A.T) + np.eye(N, dtype=LD)
    L = cholesky(Cm)
    y = chol_solve(L, x)
    return -LD(0.5) * np.dot(x, y) - np.log(np.diag(L)).sum()


def marginal_fft(x, theta, w):
    """The same number mode by mode: -1/2 sum_q |xhat_q|^2 / (N (1 + e^theta a_q^2)) - 1/2 sum_q log(1 + e^theta a_q^2); the
    transform is an explicit longdouble DFT (N <= 400)."""
    x = np.asarray(x).astype(LD)
    N = x.size
    ang = LD(2) * R.PI * np.outer(np.arange(N), np.arange(N)).astype(LD) / LD(N)
    p = ((np.cos(ang) @ x) ** 2 + (np.sin(ang) @ x) ** 2) / LD(N)
    v = LD(1) + np.exp(LD(float(theta))) * a_q(N, w) ** 2
    return -LD(0.5) * (p / v).sum() - LD(0.5) * np.log(v).sum()


def implicit_H(N, seed, sim, theta0, w, zhat=None):
    """get_H!'s per-simulation H (hp_reference.implicit_H's definition) for the weights w, by dense longdouble solves: column j is
    -dFdth^T v_j with v_j = -(A^T A + diag iv)^-1 A^T A (1/2 z_true 1_j) and dFdth_i = iv zhat 1_i; zhat = the exact MAP unless given."""
    th = np.asarray(theta0, dtype=np.float64)
    B = th.size
    x, zt, _ = sample_x_z(N, seed, sim, th, w)
    k, iv, _, _, _ = _coefs(N, th)
    L = cholesky(hessian(N, th, w))
    zh = chol_solve(L, stencil(x, w)) if zhat is None else np.asarray(zhat, np.float64).astype(LD)
    H = np.zeros((B, B), LD)
    for j in range(B):
        v = -chol_solve(L, stencil(stencil(LD(0.5) * zt * (k == j), w), w))
        for i in range(B):
            H[i, j] = -np.sum(iv * zh * (k == i) * v)
    return H


def score_at_exact_map(N, seed, sim, theta_draw, theta0, w):
    """score(zhat*(x(theta_draw)), theta0) in longdouble: what get_H!'s finite differences difference."""
    x, _, _ = sample_x_z(N, seed, sim, theta_draw, w)
    zs = chol_solve(cholesky(hessian(N, theta0, w)), stencil(x, w))
    k, iv, B, n, _ = _coefs(N, theta0)
    return LD(0.5) * (np.exp(-np.asarray(theta0, np.float64).astype(LD)) * R._bsum(zs * zs, k, B) - n.astype(LD)), zs


def expected_information(N, theta, w):
    """1/2 sum_q (e^theta a_q^2 / (1 + e^theta a_q^2))^2 for one theta."""
    u = np.exp(LD(float(theta))) * a_q(N, w) ** 2
    return float(LD(0.5) * ((u / (LD(1) + u)) ** 2).sum())
