"""An extended-precision reference of the stencil model with a pointwise response behind the operator (muse_set_link), restated
from its definition:

    z_i ~ N(0, e^{theta_k(i)}),   u = A z,   (A z)_i = w1 (z_{i-1} + z_{i+1}) + w0 z_i  (periodic)
    x_i = phi(u_i) + s_i n2_i,    phi(u) = u + a2 u^2 + a3 u^3,   phi'(u) = 1 + 2 a2 u + 3 a3 u^2,   phi''(u) = 2 a2 + 6 a3 u
    s_i = sd_i where observed, 0 where masked;   omega_i = 1 / (sd_i sd_i) where observed, 0 where masked
    f = -logLike = 1/2 sum_i omega_i r_i^2 + 1/2 sum_i e^{-theta_k} z_i^2 + 1/2 sum_k n_k theta_k,   r = x - phi(A z)
    grad_z f = e^{-theta} z - A^T (omega phi'(u) r)
    Hessian_z f = A^T diag(omega (phi'(u)^2 - r phi''(u))) A + diag(e^{-theta})
    score_k = 1/2 (e^{-theta_k} sum_{i in k} z_i^2 - n_k)          (unchanged: phi does not depend on theta)

Built on tests/noise_reference.py (omega and s as the engine's host code forms them, the matrix-free longdouble CG),
tests/stencil_reference.py (the operator, the dense longdouble Cholesky) and tests/hp_reference.py (the generator R.normals, the
block map R.blocks); it imports neither the oracle nor the package.  The oracle knows nothing of phi: this module is the checker,
and at (a2, a3) = (0, 0) every function must equal noise_reference's exactly (tests/test_link_reference.py).

Bounds, derived anew from the fp64 rounding and atol alone (U = 2^-53, every |.| elementwise):

* u.  The kernel forms u_i = fma(w1, zl + zr, w0 z0): three rounded operations on terms whose absolute sum is ua = |A| |z|:
  |du| <= 3 U ua.
* phi(u) = fma(u h, u, u), h = fma(a3, u, a2): three rounded operations on terms bounded by pa = |u| + |a2| u^2 + |a3| |u|^3, and
  the error of u enters as phi'(u) du.  With dpa(t) = 1 + 2 |a2| t + 3 |a3| t^2 >= |phi'| on [-t, t] and pa <= dpa(ua) ua:
      |d phi| <= (3 + 3) U cphi,   cphi = dpa(ua) ua.
* r = x - phi(u): one more operation; rabs = |x| + cphi, |dr| <= 7 U rabs.  q = omega r: |dq| <= 8 U qabs, qabs = omega rabs.
  The objective's term q r: (8 + 7 + 1) U qabs rabs -- the 16 of hp_reference.C_ROUND is used up by the term alone, before the
  prior's term and the sum.
* phi'(u) = fma(u, fma(3 a3, u, 2 a2), 1): four rounded operations (3 a3 is rounded; 2 a2 is exact) on terms bounded by dpa(ua),
  and du enters through phi'': |d phi'| <= 4 U dpa(ua) + ddpa(ua) 3 U ua <= 7 U cslope, cslope = dpa(ua) + ddpa(ua) ua,
  ddpa(t) = 2 |a2| + 6 |a3| t.
* rho = q phi'(u): |d rho| <= (8 + 7 + 1) U qabs cslope = 16 U rhoabs.  The gradient e^-theta z - A^T rho adds the stencil's three
  operations, the product e^-theta z and the subtraction: 21 operations on cond_g = e^-theta |z| + |A| rhoabs.
  A term therefore takes MORE operations than C_ROUND = 16 covers, and this module states its own constant, C_LINK = 24: the
  21 above and room for the second-order products of the first-order errors (each below 2^-40 of its term at the tests' sizes).
  rounding(cond) = C_LINK U cond is what the tests use for f, g and x of the linked model.  (The score's formula is unchanged
  and keeps hp_reference's bound.)
* The draw.  x_i = fma(s_i, n2_i, phi(u_i)): cond_x = cphi + s |n2| (seven operations); a masked element's x is EXACTLY 0.  An
  error dz of the drawn z (the generator's) enters x as dpa(ua) |A| dz: the GPU test carries phi' through the twin's bound so.
* The MAP.  A solve that ends g_converged at atol leaves |g(zhat)|_inf <= atol + rounding(cond_g).  With lambda a lower bound of
  the Hessian's smallest eigenvalue on the segment between zhat and z*, |zhat - z*|_2 <= |g(zhat)|_2 / lambda.  The Hessian is
  A^T diag(c) A + diag(e^-theta), c = omega (phi'^2 - r phi''), and c may be negative: by Weyl
      lambda_min >= min_k e^{-theta_k} - |A|_2^2 max_i max(0, -c_i)                                   (hessian_floor)
  with |A|_2 = max_q |a_q| the circulant's largest eigenvalue.  The GPU tests evaluate it at z* and at zhat, assert it positive (a
  condition on the inputs: link, sd and theta are chosen so that it holds with room) and assert |zhat - z*|_inf <= 2 atol / lambda.
  z* is exact_map: Newton from a given start -- the dense longdouble Cholesky for N <= 400, matrix-free Newton-CG beyond -- to
  |g|_inf <= 1e-16 max(cond_g); tests/test_link_reference.py holds the two against each other.  A step whose Hessian is not
  positive definite (far from the MAP only) falls back to the Gauss-Newton matrix A^T diag(omega phi'^2) A + diag(e^-theta), and
  every step is halved until the objective decreases: the iteration ends at a stationary point with the full Hessian's quadratic
  convergence.
* Scores at the EXACT MAP differ from those at zhat by at most e^{-theta_k} (|z*|_1 dz + n_k dz^2 / 2) over the block."""
import numpy as np

import hp_reference as R
import noise_reference as Q
import stencil_reference as S

LD = R.LD
BUILTIN = S.BUILTIN
U = R.U
C_LINK = 24                     # see the module docstring: 21 operations per term of the gradient, and room
normals = R.normals
blocks = R.blocks
weights = Q.weights


def rounding(cond):
    """|fp64 - exact| <= C_LINK 2^-53 cond for f, g and x of the linked model."""
    return C_LINK * U * np.asarray(cond, dtype=np.float64)


def _a(link):
    a2, a3 = (0.0, 0.0) if link is None else link
    return LD(np.float64(a2)), LD(np.float64(a3))


def phi(u, link):
    a2, a3 = _a(link)
    return u + u * u * (a2 + a3 * u)


def dphi(u, link):
    a2, a3 = _a(link)
    return LD(1) + u * (LD(2) * a2 + LD(3) * a3 * u)


def ddphi(u, link):
    a2, a3 = _a(link)
    return LD(2) * a2 + LD(6) * a3 * u


def _dpa(t, link):
    a2, a3 = _a(link)
    return LD(1) + LD(2) * abs(a2) * t + LD(3) * abs(a3) * t * t


def _ddpa(t, link):
    a2, a3 = _a(link)
    return LD(2) * abs(a2) + LD(6) * abs(a3) * t


def objective(x, z, theta, w, omega, link):
    """f = -logLike, g = grad_z f, cond_f, cond_g -- as noise_reference.objective with r = x - phi(A z) and rho = q phi'(u)."""
    x, z = np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD)
    x = np.where(omega != 0, x, LD(0))       # (a masked element's x enters nothing)
    N = x.size
    k, iv, B, n, cst = S._coefs(N, theta)
    ax, az = np.abs(x), np.abs(z)
    u, ua = S.stencil(z, w), S.stencil_abs(az, w)
    r = x - phi(u, link)
    rabs = ax + _dpa(ua, link) * ua
    q, qabs = omega * r, omega * rabs
    rho, rhoabs = q * dphi(u, link), qabs * (_dpa(ua, link) + _ddpa(ua, link) * ua)
    terms, tabs = q * r + iv * z * z, qabs * rabs + iv * z * z
    g = iv * z - S.stencil(rho, w)
    gabs = iv * az + S.stencil_abs(rhoabs, w)
    f = LD(0.5) * (terms.sum() + cst.sum())
    cond_f = LD(0.5) * (np.sqrt(LD(N)) * tabs.sum() + np.abs(cst).sum())
    return f, g, cond_f, gabs


def score(x, z, theta):
    return S.score(x, z, theta)


def sample_x_z(N, seed, sim, theta, w, s, link):
    """(x, z, cond_x): x = phi(A z) + s n2, exactly 0 where masked (s = 0); cond_x = dpa(|A| |z|) |A| |z| + s |n2|."""
    n1, n2, _ = R.normals(seed, sim, N)
    k, iv, _, _, _ = S._coefs(N, theta)
    z = (LD(1) / np.sqrt(iv)) * n1
    ua = S.stencil_abs(np.abs(z), w)
    x = np.where(s != 0, phi(S.stencil(z, w), link) + s * n2, LD(0))
    return x, z, _dpa(ua, link) * ua + s * np.abs(n2)


def curvature(x, z, w, omega, link):
    """c = omega (phi'(u)^2 - r phi''(u)), the diagonal between A^T and A in the Hessian (may be negative)."""
    x = np.where(omega != 0, np.asarray(x, np.float64).astype(LD), LD(0))
    u = S.stencil(np.asarray(z).astype(LD), w)
    d = dphi(u, link)
    return omega * (d * d - (x - phi(u, link)) * ddphi(u, link))


def hessian(x, z, theta, w, omega, link):
    """The full Hessian A^T diag(omega (phi'^2 - r phi'')) A + diag(e^{-theta}), dense longdouble."""
    N = np.asarray(x).size
    A = S.dense_A(N, w)
    _, iv, _, _, _ = S._coefs(N, theta)
    return A.T @ (curvature(x, z, w, omega, link)[:, None] * A) + np.diag(iv)


def hessian_floor(x, z, theta, w, omega, link):
    """min_k e^{-theta_k} - |A|_2^2 max_i max(0, -c_i): a lower bound of the Hessian's smallest eigenvalue at z (Weyl)."""
    N = np.asarray(x).size
    c = curvature(x, z, w, omega, link).astype(np.float64)
    a2 = float((np.asarray(S.a_q(N, w), dtype=np.float64) ** 2).max())
    return float(np.exp(-np.max(np.asarray(theta, np.float64)))) - a2 * float(np.maximum(0.0, -c).max())


def _cg(iv, w, c, b, rtol=LD(1e-17), maxiter=5000):
    """H v = b, H = A^T diag(c) A + diag(iv), by longdouble conjugate gradients; None when a direction of non-positive curvature
    shows (the caller falls back to the Gauss-Newton matrix)."""
    tol = rtol * np.sqrt(np.dot(b, b))
    v = np.zeros_like(b)
    r = b.copy()
    p = r.copy()
    rr = np.dot(r, r)
    for _ in range(maxiter):
        if np.sqrt(rr) <= tol:
            break
        Ap = Q.hess_apply(p, iv, w, c)
        pAp = np.dot(p, Ap)
        if not pAp > 0:
            return None
        al = rr / pAp
        v = v + al * p
        r = r - al * Ap
        rn = np.dot(r, r)
        p = r + (rn / rr) * p
        rr = rn
    return v


def _solve(x, z, theta, iv, w, omega, link, b, dense):
    c = curvature(x, z, w, omega, link)
    d = dphi(S.stencil(z, w), link)
    for cc in (c, omega * d * d):                      # the full Hessian, then Gauss-Newton (positive definite always)
        if dense:
            A = S.dense_A(z.size, w)
            try:
                return S.chol_solve(S.cholesky(A.T @ (cc[:, None] * A) + np.diag(iv)), b)
            except Exception:
                continue
        else:
            v = _cg(iv, w, cc, b)
            if v is not None:
                return v
    raise AssertionError("no descent step")


def exact_map(x, theta, w, omega, link, z_start=None, dense=None, rtol=1e-16, maxiter=100):
    """A stationary point of f by Newton's method from z_start (zero when None), in longdouble: to |g|_inf <= rtol max(cond_g).
    Dense Cholesky for N <= 400, matrix-free Newton-CG beyond."""
    N = np.asarray(x).size
    z = np.zeros(N, LD) if z_start is None else np.asarray(z_start).astype(LD)
    if dense is None:
        dense = N <= 400
    _, iv, _, _, _ = S._coefs(N, theta)
    f, g, _, gabs = objective(x, z, theta, w, omega, link)
    for _ in range(maxiter):
        if np.abs(g).max() <= LD(rtol) * gabs.max():
            return z
        step = _solve(x, z, theta, iv, w, omega, link, -g, dense)
        t = LD(1)
        while True:
            fn, gn, _, gabs_n = objective(x, z + t * step, theta, w, omega, link)
            # (decrease of f, or -- at the resolution of f -- of the gradient: the last steps move f by less than its rounding)
            if fn < f or np.abs(gn).max() < np.abs(g).max():
                break
            t = t / 2
            assert t > LD(2.0) ** -60, "the line search of exact_map found no decrease"
        z, f, g, gabs = z + t * step, fn, gn, gabs_n
    raise AssertionError(("exact_map did not converge", float(np.abs(g).max()), float(gabs.max())))


def _score_ld(z, theta):
    k, iv, B, n, _ = S._coefs(z.size, theta)
    return LD(0.5) * (np.exp(-np.asarray(theta, np.float64).astype(LD)) * R._bsum(z * z, k, B) - n.astype(LD))


def score_at_exact_map(x, theta, w, omega, link, z_start=None):
    """(score(z*), z*) in longdouble."""
    zs = exact_map(x, theta, w, omega, link, z_start)
    return _score_ld(zs, theta), zs


def muse_gradient(x, theta, w, omega, s, link, seed, nsims, starts=None):
    """The MUSE gradient at theta from the engine's own streams (seed, simulations 0 .. nsims - 1), every MAP exact: the data's
    score minus the mean of the simulations' scores, each simulation drawn at theta.  `starts` (a dict the caller keeps) carries the
    MAPs from one call to the next as Newton's starts.  Returns fp64."""
    th = np.asarray(theta, np.float64)
    N = np.asarray(x).size
    starts = {} if starts is None else starts
    sd, starts["data"] = score_at_exact_map(x, th, w, omega, link, starts.get("data"))
    acc = np.zeros(th.size, LD)
    for i in range(nsims):
        xi = sample_x_z(N, seed, i, th, w, s, link)[0].astype(np.float64)
        sc, starts[i] = score_at_exact_map(xi, th, w, omega, link, starts.get(i))
        acc += sc
    return (sd - acc / nsims).astype(np.float64)
