"""An extended-precision reference of the stencil model with ANY pointwise response behind the operator (include/muse_model.h,
MUSE_MODEL_RESPONSE), restated from its definition with phi, phi' and phi'' as callables:

    z_i ~ N(0, e^{theta_k(i)}),   u = A z,   (A z)_i = w1 (z_{i-1} + z_{i+1}) + w0 z_i  (periodic)
    x_i = phi(u_i) + s_i n2_i,    s_i = sd_i where observed, 0 where masked;   omega_i = 1 / (sd_i sd_i) where observed, else 0
    f = -logLike = 1/2 sum_i omega_i r_i^2 + 1/2 sum_i e^{-theta_k} z_i^2 + 1/2 sum_k n_k theta_k,   r = x - phi(A z)
    grad_z f = e^{-theta} z - A^T (omega phi'(u) r)
    Hessian_z f = A^T diag(omega (phi'(u)^2 - r phi''(u))) A + diag(e^{-theta})
    score_k = 1/2 (e^{-theta_k} sum_{i in k} z_i^2 - n_k)
    implicit H[k][j] = (e^{-theta_k} zhat|_k) . Hessian_z f (zhat)^-1 b_j,   b_j = A^T (omega phi'(u) phi'(u_t) A (z_true / 2)|_j),
                       u = A zhat, u_t = A z_true          (get_H!'s implicit-differentiation branch; H1 = 0)

A `Response` carries the three callables (longdouble in, longdouble out), two majorants -- dpa(t) >= |phi'| and ddpa(t) >= |phi''|
on [-t, t] -- and the rounding constant of its fp64 expressions.  tests/link_reference.py is the special case of the cubic: with
`cubic(link)` every function here returns what link_reference returns, array-equal (tests/test_response_reference.py); it is built
on the same pieces (noise_reference's weights and Hessian product, stencil_reference's operator and Cholesky, hp_reference's
generator) and imports neither the oracle nor the package.

Bounds (U = 2^-53).  The structure is link_reference's, whose docstring derives it: a term of f, g or x is a fixed number of rounded
operations on quantities bounded by a condition number, |fp64 - exact| <= C U cond.  The condition numbers are written with dpa and
ddpa and so hold for any response; C counts the response's own operations:

* the cubic: C_LINK = 24 (link_reference).
* the saturating response phi = u / sqrt(q), q = fma(s, s, 1), s = p0 u, phi' = 1 / (q sqrt(q)):
    u: 3 operations (relative 3 U of |A||z|);  s: +1 = 4;  q = 1 + s^2: 2 * 4 U s^2 / q + U <= 9 U;  sqrt(q): 9/2 + 1 <= 6 U;
    phi = u / sqrt(q): 3 + 6 + 1 = 10 U;   r = x - phi: 11;   q_w = omega r: 12;   the objective's term q_w r: 12 + 11 + 1 = 24;
    phi' = 1 / (q sqrt(q)): 9 + 6 + 1 + 1 = 17 U, and du enters through phi'' (inside cslope = dpa + ddpa ua, as for the cubic);
    rho = q_w phi': 12 + 17 + 1 = 30;   the gradient adds the stencil's 3, the product e^-theta z and the subtraction: 35.
  C_SAT = 35 + 5 = 40: the 35 above and room for the second-order products (as C_LINK keeps 3 of 24).
* the implicit H, entry [k][j] (implicit_H_bound).  Conjugate gradients stops at |r|_2 <= reltol |b_j|_2, so its v is within
  reltol |b_j|_2 / lambda of the solution (lambda = hessian_floor > 0) and the entry within |dFdtheta_k|_2 reltol |b_j|_2 / lambda.
  The engine's zhat is within dz = 2 atol / lambda of the exact MAP in the max-norm.  H[k][j] = sum_{i in k} e^-theta_k zhat_i v_i
  depends on zhat through dFdtheta directly -- over the l_inf-ball of radius dz that moves the entry by at most
  e^-theta_k dz sum_{i in k} |v_i| (attained at dz sign(v), whose signs are not sign(z*)'s) -- and through v (d, e and so the
  Hessian and b_j are formed at zhat): for that the reference re-evaluates H with the MAP displaced by +- dz sign(z*) and takes the
  larger change.  Both terms enter.  (The first was missing at first: 1500 x 12 at reltol 1e-12 then showed 3.8 times the bound on
  the GPU, an error of 8e-11 relative where the term allows 1.6e-9.)  Rounding: the final sums are
  C U sqrt(n_k) sum |e^-theta zhat v|, and an fp64 CG's recurrence residual departs from the true one by ~ kappa U |b|
  (kappa = (max omega |A|_2^2 + max e^-theta) / lambda), which enters as C U kappa |dFdtheta_k|_2 |v_j|_2."""
import numpy as np

import hp_reference as R
import link_reference as L
import noise_reference as Q
import stencil_reference as S

LD = R.LD
BUILTIN = S.BUILTIN
U = R.U
C_SAT = 35 + 5                  # see the module docstring: the operation count of the saturating header's gradient term, and room
normals = R.normals
blocks = R.blocks
weights = Q.weights


class Response:
    def __init__(self, name, phi, dphi, ddphi, dpa, ddpa, c_round, params):
        self.name, self.phi, self.dphi, self.ddphi, self.dpa, self.ddpa, self.c_round, self.params = name, phi, dphi, ddphi, dpa, ddpa, c_round, params


def cubic(link):
    """phi(u) = u + a2 u^2 + a3 u^3 -- link_reference's own callables and constant."""
    return Response("cubic", lambda u: L.phi(u, link), lambda u: L.dphi(u, link), lambda u: L.ddphi(u, link),
                    lambda t: L._dpa(t, link), lambda t: L._ddpa(t, link), L.C_LINK, (0.0, 0.0) if link is None else tuple(link))


def saturating(p0):
    """phi(u) = u / sqrt(1 + (p0 u)^2): phi' = q^-3/2 in (0, 1], phi'' = -3 p0^2 u q^-5/2, |phi''| <= 3 p0^2 |u|."""
    p = LD(np.float64(p0))

    def q(u):
        return LD(1) + (p * u) * (p * u)
    return Response("saturating", lambda u: u / np.sqrt(q(u)), lambda u: LD(1) / (q(u) * np.sqrt(q(u))),
                    lambda u: -LD(3) * p * p * u / (q(u) * q(u) * np.sqrt(q(u))),
                    lambda t: LD(1) + LD(0) * t, lambda t: LD(3) * p * p * t, C_SAT, (float(p0), 0.0))


def rounding(cond, resp):
    """|fp64 - exact| <= C 2^-53 cond for f, g and x of the model with this response."""
    return resp.c_round * U * np.asarray(cond, dtype=np.float64)


def objective(x, z, theta, w, omega, resp):
    """f = -logLike, g = grad_z f, cond_f, cond_g."""
    x, z = np.asarray(x, np.float64).astype(LD), np.asarray(z, np.float64).astype(LD)
    x = np.where(omega != 0, x, LD(0))       # (a masked element's x enters nothing)
    N = x.size
    k, iv, B, n, cst = S._coefs(N, theta)
    ax, az = np.abs(x), np.abs(z)
    u, ua = S.stencil(z, w), S.stencil_abs(az, w)
    r = x - resp.phi(u)
    rabs = ax + resp.dpa(ua) * ua
    q, qabs = omega * r, omega * rabs
    rho, rhoabs = q * resp.dphi(u), qabs * (resp.dpa(ua) + resp.ddpa(ua) * ua)
    terms, tabs = q * r + iv * z * z, qabs * rabs + iv * z * z
    g = iv * z - S.stencil(rho, w)
    gabs = iv * az + S.stencil_abs(rhoabs, w)
    f = LD(0.5) * (terms.sum() + cst.sum())
    cond_f = LD(0.5) * (np.sqrt(LD(N)) * tabs.sum() + np.abs(cst).sum())
    return f, g, cond_f, gabs


def score(x, z, theta):
    return S.score(x, z, theta)


def sample_x_z(N, seed, sim, theta, w, s, resp):
    """(x, z, cond_x): x = phi(A z) + s n2, exactly 0 where masked (s = 0); cond_x = dpa(|A| |z|) |A| |z| + s |n2|."""
    n1, n2, _ = R.normals(seed, sim, N)
    k, iv, _, _, _ = S._coefs(N, theta)
    z = (LD(1) / np.sqrt(iv)) * n1
    ua = S.stencil_abs(np.abs(z), w)
    x = np.where(s != 0, resp.phi(S.stencil(z, w)) + s * n2, LD(0))
    return x, z, resp.dpa(ua) * ua + s * np.abs(n2)


def curvature(x, z, w, omega, resp):
    """c = omega (phi'(u)^2 - r phi''(u)), the diagonal between A^T and A in the Hessian (may be negative)."""
    x = np.where(omega != 0, np.asarray(x, np.float64).astype(LD), LD(0))
    u = S.stencil(np.asarray(z).astype(LD), w)
    d = resp.dphi(u)
    return omega * (d * d - (x - resp.phi(u)) * resp.ddphi(u))


def hessian(x, z, theta, w, omega, resp):
    """The full Hessian A^T diag(omega (phi'^2 - r phi'')) A + diag(e^{-theta}), dense longdouble."""
    N = np.asarray(x).size
    A = S.dense_A(N, w)
    _, iv, _, _, _ = S._coefs(N, theta)
    return A.T @ (curvature(x, z, w, omega, resp)[:, None] * A) + np.diag(iv)


def hessian_floor(x, z, theta, w, omega, resp):
    """min_k e^{-theta_k} - |A|_2^2 max_i max(0, -c_i): a lower bound of the Hessian's smallest eigenvalue at z (Weyl)."""
    N = np.asarray(x).size
    c = curvature(x, z, w, omega, resp).astype(np.float64)
    a2 = float((np.asarray(S.a_q(N, w), dtype=np.float64) ** 2).max())
    return float(np.exp(-np.max(np.asarray(theta, np.float64)))) - a2 * float(np.maximum(0.0, -c).max())


def _solve(x, z, theta, iv, w, omega, resp, b, dense):
    c = curvature(x, z, w, omega, resp)
    d = resp.dphi(S.stencil(z, w))
    for cc in (c, omega * d * d):                      # the full Hessian, then Gauss-Newton (positive definite always)
        if dense:
            A = S.dense_A(z.size, w)
            try:
                return S.chol_solve(S.cholesky(A.T @ (cc[:, None] * A) + np.diag(iv)), b)
            except Exception:
                continue
        else:
            v = L._cg(iv, w, cc, b)
            if v is not None:
                return v
    raise AssertionError("no descent step")


def exact_map(x, theta, w, omega, resp, z_start=None, dense=None, rtol=1e-16, maxiter=100):
    """A stationary point of f by Newton's method from z_start (zero when None), in longdouble: to |g|_inf <= rtol max(cond_g).
    Dense Cholesky for N <= 400, matrix-free Newton-CG beyond (link_reference.exact_map, the response as callables)."""
    N = np.asarray(x).size
    z = np.zeros(N, LD) if z_start is None else np.asarray(z_start).astype(LD)
    if dense is None:
        dense = N <= 400
    _, iv, _, _, _ = S._coefs(N, theta)
    f, g, _, gabs = objective(x, z, theta, w, omega, resp)
    for _ in range(maxiter):
        if np.abs(g).max() <= LD(rtol) * gabs.max():
            return z
        step = _solve(x, z, theta, iv, w, omega, resp, -g, dense)
        t = LD(1)
        while True:
            fn, gn, _, gabs_n = objective(x, z + t * step, theta, w, omega, resp)
            if fn < f or np.abs(gn).max() < np.abs(g).max():
                break
            t = t / 2
            assert t > LD(2.0) ** -60, "the line search of exact_map found no decrease"
        z, f, g, gabs = z + t * step, fn, gn, gabs_n
    raise AssertionError(("exact_map did not converge", float(np.abs(g).max()), float(gabs.max())))


def score_at_exact_map(x, theta, w, omega, resp, z_start=None):
    """(score(z*), z*) in longdouble."""
    zs = exact_map(x, theta, w, omega, resp, z_start)
    return L._score_ld(zs, theta), zs


def implicit_rhs(zt, zh, theta, w, omega, resp, j):
    """b_j = A^T (omega phi'(A zhat) phi'(A z_true) A (z_true / 2)|_j), longdouble."""
    k = R.blocks(zt.size, np.asarray(theta).size)
    e = omega * resp.dphi(S.stencil(zh, w)) * resp.dphi(S.stencil(zt, w))
    return S.stencil(e * S.stencil(LD(0.5) * zt * (k == j), w), w)


def implicit_H(N, seed, sim, theta0, w, omega, s, resp, zhat=None, dense=None):
    """get_H!'s per-simulation H by implicit differentiation at zhat (the exact MAP of the simulation's draw unless given):
    (H [B, B], [|v_j|], [|b_j|_2], zhat), v_j = Hessian_z f^-1 b_j."""
    th = np.asarray(theta0, dtype=np.float64)
    B = th.size
    x, zt, _ = sample_x_z(N, seed, sim, th, w, s, resp)
    x = x.astype(np.float64)
    k, iv, _, _, _ = S._coefs(N, th)
    if dense is None:
        dense = N <= 400
    zh = exact_map(x, th, w, omega, resp, dense=dense) if zhat is None else np.asarray(zhat).astype(LD)
    c = curvature(x, zh, w, omega, resp)
    if dense:
        A = S.dense_A(N, w)
        Lc = S.cholesky(A.T @ (c[:, None] * A) + np.diag(iv))
        solve = lambda b: S.chol_solve(Lc, b)
    else:
        def solve(b):
            v = L._cg(iv, w, c, b)
            assert v is not None, "the Hessian at zhat is not positive definite"
            return v
    H = np.zeros((B, B), LD)
    vs, bn = [], []
    for j in range(B):
        b = implicit_rhs(zt, zh, th, w, omega, resp, j)
        v = solve(b)
        vs.append(np.abs(v))
        bn.append(float(np.sqrt(np.dot(b, b))))
        for i in range(B):
            H[i, j] = np.sum(iv * zh * (k == i) * v)
    return H, vs, bn, zh


def implicit_H_bound(N, seed, sim, theta0, w, omega, s, resp, atol, reltol, dense=None):
    """(H at the exact MAP, the bound of the module docstring entry by entry, lambda).  The MAP's displacement enters through
    dFdtheta (e^-theta dz |v|_1 over the block) and through v (H re-evaluated with the MAP displaced by +- 2 atol / lambda sign(z*))."""
    th = np.asarray(theta0, np.float64)
    B = th.size
    H, vs, bn, zs = implicit_H(N, seed, sim, th, w, omega, s, resp, dense=dense)
    x = sample_x_z(N, seed, sim, th, w, s, resp)[0].astype(np.float64)
    lam = hessian_floor(x, zs, th, w, omega, resp)
    assert lam > 0, lam
    dz = 2 * atol / lam
    k, iv = R.blocks(N, B), np.exp(-th)
    sg = np.where(zs >= 0, LD(1), LD(-1))
    moved = np.zeros((B, B))
    for sign in (1.0, -1.0):
        Hm = implicit_H(N, seed, sim, th, w, omega, s, resp, zhat=zs + LD(sign * dz) * sg, dense=dense)[0]
        moved = np.maximum(moved, np.abs(Hm - H).astype(np.float64))
    aq2 = float((np.asarray(S.a_q(N, w), dtype=np.float64) ** 2).max())
    kappa = (float(np.asarray(omega, np.float64).max()) * aq2 + float(iv.max())) / lam
    out = np.zeros((B, B))
    for j in range(B):
        v = vs[j].astype(np.float64)
        for i in range(B):
            m = k == i
            dF = iv[i] * np.abs(zs[m]).astype(np.float64)
            out[i, j] = (np.linalg.norm(dF) * reltol * bn[j] / lam + iv[i] * dz * v[m].sum() + moved[i, j]
                         + resp.c_round * U * (np.sqrt(m.sum()) * (dF * v[m]).sum() + kappa * np.linalg.norm(dF) * np.linalg.norm(v)))
    return H, out, lam


# ---- an fp64 numpy restatement of what the kernels compute (objective, gradient, conjugate gradients): the reference's bounds
#      are held against it on the CPU before a GPU sees them (tests/test_response_reference.py)
def numpy_response(name, p):
    """(phi, phi', phi'') in fp64 numpy, the packaged headers' expressions."""
    p0, p1 = float(p[0]), float(p[1])
    if name == "poly_response":
        return (lambda u: u * (p1 * u + p0) * u + u, lambda u: u * (3.0 * p1 * u + 2.0 * p0) + 1.0, lambda u: 6.0 * p1 * u + 2.0 * p0)
    assert name == "saturating_response"
    q = lambda u: (p0 * u) * (p0 * u) + 1.0
    return (lambda u: u / np.sqrt(q(u)), lambda u: 1.0 / (q(u) * np.sqrt(q(u))), lambda u: -(3.0 * p0 * (p0 * u)) / ((q(u) * q(u)) * np.sqrt(q(u))))


def numpy_objective(x, z, theta, w, omega, fns, total=lambda v: float(np.sum(v))):
    """(f, g) in fp64; `total` forms the objective's sum (link_cases.ORDERS: the order is the kernels' business)."""
    N = x.size
    th = np.asarray(theta, np.float64)
    iv = np.exp(-th)[R.blocks(N, th.size)]
    cst = float(np.sum(R.block_sizes(N, th.size) * th))
    om = np.asarray(omega, np.float64)
    xf = np.where(om != 0, x, 0.0)
    A = lambda v: w[1] * (np.roll(v, 1) + np.roll(v, -1)) + w[0] * v
    u = A(z)
    r = xf - fns[0](u)
    q = om * r
    return 0.5 * (total(q * r + iv * z * z) + cst), iv * z - A(q * fns[1](u))


def numpy_cg(x, zh, zt, theta, w, omega, fns, j, reltol=1.4901161193847656e-08, abstol=0.0, maxiter=200, d=None):
    """The kernel's CG for column j in fp64 (solver.hpp, run_implicit with plain_cg and its guard): returns (v with -Hessian v = b, count); the count
    is -1 - iterations when p.Ap is not finite and negative (an indefinite Hessian).  `d` overrides the curvature vector."""
    N = x.size
    th = np.asarray(theta, np.float64)
    k = R.blocks(N, th.size)
    iv = np.exp(-th)[k]
    om = np.asarray(omega, np.float64)
    A = lambda v: w[1] * (np.roll(v, 1) + np.roll(v, -1)) + w[0] * v
    u, ut = A(zh), A(zt)
    fp = fns[1](u)
    r = np.where(om != 0, x - fns[0](u), 0.0)
    dd = np.where(om != 0, om * (fp * fp - r * fns[2](u)), 0.0) if d is None else d
    ee = (om * fp) * fns[1](ut)
    b = A(ee * A(np.where(k == j, 0.5 * zt, 0.0)))
    v, res, p = np.zeros(N), b.copy(), b.copy()
    rr = float(res @ res)
    tol = max(reltol * np.sqrt(rr), abstol)
    it = 0
    while it < maxiter and not np.sqrt(rr) <= tol:
        Ap = -(A(dd * A(p)) + iv * p)
        pAp = float(p @ Ap)
        if not pAp < 0.0 or np.isinf(pAp):
            return v, -1 - it
        al = rr / pAp
        v = v + al * p
        res = res - al * Ap
        rn = float(res @ res)
        p = res + (rn / rr) * p
        rr = rn
        it += 1
    return v, it
