"""Deblurring behind a non-linear detector: the coupled `smooth` model with a pointwise response as state of the problem.

    z_i ~ N(0, e^{theta_k}),   u = A z,   x_i = phi(u_i) + sd_i n_i  where observed,   phi(u) = u + a2 u^2 + a3 u^3

A field with two variance components is blurred by the periodic (1/4, 1/2, 1/4) stencil and seen through a compressive response
(a2 < 0: the gain falls with the signal; a3 > 0 keeps phi monotone, a2^2 < 3 a3), with a noise ramp sd in [0.5, 2] and a masked
stripe.  The model is no longer jointly Gaussian, so there is no closed-form marginal posterior to compare with -- this is the
case MUSE is for.  muse() runs on the HIP path (HipMuseProblem(..., link=(a2, a3))) with the finite-difference covariance (the
implicit-differentiation branch is refused for a problem with a link), and the answer is set beside the truth and beside the root of
the same MUSE gradient evaluated on the host: the data's score minus the mean of the simulations' scores, every MAP solved by
Newton's method with a sparse factorisation of the Hessian, the simulations redrawn at each theta from the engine's own normals."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl
from scipy.optimize import root

import museinference_jl_amd as M

N, nth, truth, nsims, prior_sigma, seed = 2048, 2, [1.0, 0.2], 32, 3.0, 1
link = (-0.08, 0.02)              # compressive and monotone: phi' = 1 - 0.16 u + 0.06 u^2 >= 0.89
sd = np.linspace(0.5, 2.0, N)
mask = np.ones(N, bool)
mask[700:800] = False             # the stripe
mask[[0, N - 1]] = False          # ... and the two pixels next to the periodic wrap

k = (np.arange(N) * nth) // N   # the block of an element (N divides evenly)
om = np.where(mask, 1.0 / (sd * sd), 0.0)
i = np.arange(N)
A = sp.csc_matrix((np.concatenate([np.full(N, 0.5), np.full(N, 0.25), np.full(N, 0.25)]),
                   (np.concatenate([i, i, i]), np.concatenate([i, (i - 1) % N, (i + 1) % N]))), shape=(N, N))
a2, a3 = link
phi = lambda u: u + u * u * (a2 + a3 * u)
dphi = lambda u: 1.0 + u * (2.0 * a2 + 3.0 * a3 * u)
ddphi = lambda u: 2.0 * a2 + 6.0 * a3 * u


def host_map(x, t, z):
    """The MAP of z given x at theta = t by Newton's method from z (fp64, sparse LU of the Hessian; Gauss-Newton while the full
    Hessian's curvature term is negative somewhere)."""
    iv = np.exp(-t)[k]
    xo = np.where(mask, x, 0.0)
    for _ in range(50):
        u = A @ z
        r = xo - phi(u)
        g = iv * z - A.T @ (om * dphi(u) * r)
        if np.abs(g).max() <= 1e-11:
            break
        c = om * (dphi(u) ** 2 - r * ddphi(u))
        c = c if c.min() >= 0 else om * dphi(u) ** 2
        z = z - spl.splu((A.T @ sp.diags(c) @ A + sp.diags(iv)).tocsc()).solve(g)
    return z


def host_root(x, normals, theta_start):
    """The root of the MUSE gradient plus the prior's, from the same streams the engine drew."""
    starts = {}

    def score_at_map(key, xv, t):
        starts[key] = host_map(xv, t, starts.get(key, np.zeros(N)))
        z = starts[key]
        return 0.5 * (np.exp(-t) * np.bincount(k, weights=z * z, minlength=nth) - np.bincount(k, minlength=nth))

    def gradient(t):
        t = np.asarray(t, float)
        sims = []
        for j, (n1, n2) in enumerate(normals):
            z = np.exp(0.5 * t)[k] * n1
            sims.append(score_at_map(j, np.where(mask, phi(A @ z) + sd * n2, 0.0), t))
        return score_at_map("data", x, t) - np.mean(sims, axis=0) - t / prior_sigma ** 2
    sol = root(gradient, theta_start, tol=1e-9)
    assert sol.success, sol.message
    return sol.x


draw = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, noise_sd=sd, mask=mask, link=link)
x, _ = draw.sample_x_z(M.SimRng(2024, M.DATA_SIM), truth)
assert np.all(x[~mask] == 0.0)
# the engine's own normals of the simulations muse() draws (streams 0 .. nsims - 1 of the seed), recovered from a draw at theta = 0
normals = []
for sim in range(nsims):
    xs, zs = draw.sample_x_z(M.SimRng(seed, sim), [0.0] * nth)
    normals.append((zs, np.where(mask, (xs - phi(A @ zs)) / sd, 0.0)))
draw.close()

prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, prior=M.GaussianPrior(0.0, prior_sigma), noise_sd=sd, mask=mask, link=link)
assert prob.get_link() == (link, True)
# (alpha = 0.7, the reference's default: with full steps the quasi-Newton iteration of this non-linear problem settles into a
#  two-cycle around the root instead of converging)
res = M.muse(prob, [0.0] * nth, rng=seed, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-6, alpha=0.7,
             get_covariance=True)
prob.close()
sigma = np.sqrt(np.diag(np.atleast_2d(res.Sigma)))
ref = host_root(x, normals, np.asarray(res.theta, float))
for j in range(nth):
    print(f"nonlinear deblur theta[{j}]: muse = {res.theta[j]:+.4f} +- {sigma[j]:.4f}   host root of the same gradient {ref[j]:+.4f}"
          f"   (truth {truth[j]:+.1f})")
assert np.all(np.abs(np.asarray(res.theta) - np.asarray(truth)) < 5 * sigma)
assert np.all(np.abs(np.asarray(res.theta) - ref) < 4 * sigma / np.sqrt(nsims))
