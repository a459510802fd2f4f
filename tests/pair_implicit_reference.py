"""A numpy-longdouble restatement of the implicit-differentiation get_H! of the two-parameter user-model family
(include/muse_model.h, MUSE_MODEL_PAIR_SECOND), for three models.  It imports neither the package nor the oracle; the normals are
tests/hp_reference.py's.

Block k has parameters a = theta[k], b = theta[K + k]; iv = e^-b, sd = e^(b/2).  Per element, at (x, zhat, theta0):

    ozz = d2(o/2)/dz2, ozx = d2(o/2)/dz dx, gza, gzb = d/da, d/db of d(o/2)/dz, sxa, sxb = d/dx of -1/2 do/da, -1/2 do/db,
    xa, xb = dx/da, dx/db at fixed normals,

    A w = -ozz w,  dFdtheta[:, p] = -gzp (p's block),  dFdtheta1[:, q] = -ozx xq (q's block),  H1[p, q] = sum_{block} sxp xq,
    H[:, q] = H1[:, q] - dFdtheta^T A^{-1} dFdtheta1[:, q]          (the diagonal solve is exact here: no CG)

  normal_mean_var   z ~ N(a, e^b), x ~ N(z, 1):            o = (x - z)^2 + iv (z - a)^2
  offset_noise      z ~ N(0, 1),   x ~ N(z + a, e^b):      o = z^2 + iv (x - z - a)^2
  cubic_mean_var    z ~ N(a, e^b), x ~ N(z + z^3/10, 1):   o = (x - z - z^3/10)^2 + iv (z - a)^2

The MAP is the closed form of the two Gaussian models and per-element Newton steps (from the simulation's true z) for the cubic one.

Bound per entry (implicit_H returns it beside the value).  The engine's CG stops at |r| <= reltol |b_q|, so its solution is within
reltol |b_q|_2 / min ozz of the exact one in the 2-norm, and entry (p, q) within |gzp|_2 reltol |b_q|_2 / min ozz; to that comes the
fp64 rounding of the entry's sums, hp_reference.rounding of their condition sum (sqrt(n) sum |terms|, the terms evaluated on absolute
values).  bound(reltol) is the sum of the two; a test allows twice that, which covers the MAP's own tolerance.  H1 alone (cg_maxiter =
0) involves no solve: its bound is the rounding term plus the MAP's tolerance carried through, atol sum |d(sxp xq)/dz| / ozz.
"""
import numpy as np

import hp_reference as R

LD = R.LD
MODELS = ("normal_mean_var", "offset_noise", "cubic_mean_var")
RELTOL_DEFAULT = float(np.sqrt(np.finfo(np.float64).eps))

# the cubic model generated from its terms (ElementwiseModel.from_pair_expressions); normal_mean_var's terms are
# tests/test_symbolic_model.py's NMV_TERMS
CUBIC_TERMS = dict(coefs=["a", "exp(b/2)", "exp(-b)"], C="b", o="(x - z - z**3/10)**2 + c2*(z - c0)**2", z="c0 + c1*n1",
                   x="z + z**3/10 + n2")


def _per_element(N, theta):
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    K = th.size // 2
    k = R.blocks(N, K)
    return K, k, th[:K][k], np.exp(th[K:] / LD(2))[k], np.exp(-th[K:])[k]


def sample(model, N, seed, sim, theta):
    """(x, z, n1, n2) in longdouble."""
    n1, n2, _ = R.normals(seed, sim, N)
    _, _, a, sd, _ = _per_element(N, theta)
    if model == "offset_noise":
        return n1 + a + sd * n2, n1, n1, n2
    z = a + sd * n1
    if model == "cubic_mean_var":
        return z + z ** 3 / LD(10) + n2, z, n1, n2
    return z + n2, z, n1, n2


def exact_map(model, x, z_true, N, theta):
    _, _, a, _, iv = _per_element(N, theta)
    if model == "normal_mean_var":
        return (x + iv * a) / (LD(1) + iv)
    if model == "offset_noise":
        return iv * (x - a) / (LD(1) + iv)
    z = z_true.copy()
    for _ in range(60):
        h, hp = z + z ** 3 / LD(10), LD(1) + LD(3) * z * z / LD(10)
        g = iv * (z - a) - (x - h) * hp
        z = z - g / (iv + hp * hp - (x - h) * (LD(6) * z / LD(10)))
    h, hp = z + z ** 3 / LD(10), LD(1) + LD(3) * z * z / LD(10)
    assert np.max(np.abs(iv * (z - a) - (x - h) * hp)) < 1e-17, "the Newton polish of the cubic model's MAP has not converged"
    return z


def operands(model, x, z, n1, n2, N, theta):
    """The eight per-element operands at (x, z) and, for the condition sums, their evaluation on absolute values; d(sxa)/dz and
    d(sxb)/dz for the MAP-tolerance term of H1."""
    _, _, a, sd, iv = _per_element(N, theta)
    ax, az, aa = np.abs(x), np.abs(z), np.abs(a)
    one, zero = np.ones(N, LD), np.zeros(N, LD)
    if model == "offset_noise":
        r, rabs = x - z - a, ax + az + aa
        q = dict(ozz=one + iv, ozx=-iv, gza=iv, gzb=iv * r, sxa=iv, sxb=iv * r, xa=one, xb=LD(0.5) * sd * n2)
        qa = dict(q, gzb=iv * rabs, sxb=iv * rabs, ozx=iv, xb=np.abs(q["xb"]))
        return q, qa, dict(sxa=zero, sxb=-iv)
    d, dabs = z - a, az + aa
    if model == "normal_mean_var":
        q = dict(ozz=one + iv, ozx=-one, gza=-iv, gzb=-iv * d, sxa=zero, sxb=zero, xa=one, xb=LD(0.5) * sd * n1)
        qa = dict(q, ozx=one, gza=iv, gzb=iv * dabs, xb=np.abs(q["xb"]))
        return q, qa, dict(sxa=zero, sxb=zero)
    zt = a + sd * n1                                   # the draw's z: x = h(zt) + n2, dx/da = h'(zt), dx/db = h'(zt) sd n1 / 2
    h, hp, hpt = z + z ** 3 / LD(10), LD(1) + LD(3) * z * z / LD(10), LD(1) + LD(3) * zt * zt / LD(10)
    habs = az + az ** 3 / LD(10)
    q = dict(ozz=iv + hp * hp - (x - h) * (LD(6) * z / LD(10)), ozx=-hp, gza=-iv, gzb=-iv * d, sxa=zero, sxb=zero, xa=hpt,
             xb=LD(0.5) * hpt * sd * n1)
    qa = dict(q, ozz=iv + hp * hp + (ax + habs) * (LD(6) * az / LD(10)), ozx=hp, gza=iv, gzb=iv * dabs, xb=np.abs(q["xb"]))
    return q, qa, dict(sxa=zero, sxb=zero)


def implicit_H(model, N, seed, sim, theta, atol=1e-10):
    """One simulation's H at the exact MAP: a dict with H, H1, H2 = H - H1 (float64 [nth, nth]) and bound(reltol), bound_H2(reltol),
    bound_H1 as in the module docstring."""
    assert model in MODELS
    th = np.asarray(theta, dtype=np.float64)
    nth = th.size
    x, zt, n1, n2 = sample(model, N, seed, sim, th)
    zh = exact_map(model, x, zt, N, th)
    K, k, _, _, _ = _per_element(N, th)
    q, qa, dsx = operands(model, x, zh, n1, n2, N, th)
    assert np.all(q["ozz"] > 0), "theta must keep d2 o / dz2 positive at every MAP"
    min_ozz = q["ozz"].min()
    H1, H2 = np.zeros((nth, nth), LD), np.zeros((nth, nth), LD)
    c1, c2, cgf, mapt = (np.zeros((nth, nth), LD) for _ in range(4))
    gz, sx = (q["gza"], q["gzb"]), (q["sxa"], q["sxb"])
    gza_, sxa_ = (qa["gza"], qa["gzb"]), (qa["sxa"], qa["sxb"])
    for col in range(nth):
        kb, kind = col % K, col // K
        m = k == kb
        n = LD(m.sum())
        xq, xqa = (q["xa"], q["xb"])[kind][m], (qa["xa"], qa["xb"])[kind][m]
        b = -q["ozx"][m] * xq                             # dFdtheta1[:, col] on its block
        v = -b / q["ozz"][m]                              # A^{-1} b, A = -ozz
        va = qa["ozx"][m] * xqa / q["ozz"][m]
        for pk in range(2):                               # rows kb (a) and K + kb (b): every other row is zero
            row = pk * K + kb
            H1[row, col] = np.sum(sx[pk][m] * xq)
            H2[row, col] = np.sum(gz[pk][m] * v)          # -dFdtheta^T v, dFdtheta = -gz
            c1[row, col] = np.sqrt(n) * np.sum(sxa_[pk][m] * xqa)
            c2[row, col] = np.sqrt(n) * np.sum(gza_[pk][m] * va)
            cgf[row, col] = np.sqrt(np.sum(gz[pk][m] ** 2)) * np.sqrt(np.sum(b * b)) / min_ozz
            mapt[row, col] = LD(atol) * np.sum(np.abs((dsx["sxa"], dsx["sxb"])[pk][m] * xq) / q["ozz"][m])
    f = lambda M: np.asarray(M, dtype=np.float64)
    return dict(H=f(H1 + H2), H1=f(H1), H2=f(H2),
                bound=lambda reltol=RELTOL_DEFAULT: f(cgf) * reltol + R.rounding(f(c1 + c2)),
                bound_H2=lambda reltol=RELTOL_DEFAULT: f(cgf) * reltol + R.rounding(f(c2)),
                bound_H1=R.rounding(f(c1)) + f(mapt))


def exact_information(n, tau):
    """E[H] of the two Gaussian models with one block of n elements: the Fisher information of x_i ~ N(mu, 1 + e^tau)."""
    e = np.exp(tau)
    return np.diag([n / (1.0 + e), 0.5 * n * (e / (1.0 + e)) ** 2])
