"""Deblurring behind a detector that SATURATES: the coupled stencil model with a response stated in a header.

    z_i ~ N(0, e^{theta_k}),   u = A z,   x_i = phi(u_i) + sd_i n_i  where observed,   phi(u) = u / sqrt(1 + (p0 u)^2)

No polynomial states this response (|phi| < 1 / p0), so muse_set_link's cubic cannot: the model is
ResponseModel.packaged("saturating_response") -- museinference.jl_amd/models/saturating_response.h, a dozen lines of C -- and the
stencil, the noise ramp, the masked stripe and the response's number p0 are state of the problem, as for model="smooth".  The
header states phi'', so get_H! runs by implicit differentiation (one MAP and ntheta CG solves per simulation instead of
2 ntheta + 1 MAPs); the finite-difference branch is run beside it, and the answer is set beside the truth and beside the root of
the same MUSE gradient evaluated on the host with every MAP solved by Newton's method (sparse LU)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl
from scipy.optimize import root

import museinference_jl_amd as M

N, nth, truth, nsims, prior_sigma, seed = 2048, 2, [1.0, 0.2], 32, 3.0, 1
p0 = 0.35                         # |u| reaches ~3 at theta = 1: phi' falls to ~0.3 on the brightest pixels
sd = np.linspace(0.5, 2.0, N)
mask = np.ones(N, bool)
mask[700:800] = False             # the stripe
mask[[0, N - 1]] = False          # ... and the two pixels next to the periodic wrap

k = (np.arange(N) * nth) // N
om = np.where(mask, 1.0 / (sd * sd), 0.0)
i = np.arange(N)
A = sp.csc_matrix((np.concatenate([np.full(N, 0.5), np.full(N, 0.25), np.full(N, 0.25)]),
                   (np.concatenate([i, i, i]), np.concatenate([i, (i - 1) % N, (i + 1) % N]))), shape=(N, N))
q = lambda u: 1.0 + (p0 * u) ** 2
phi = lambda u: u / np.sqrt(q(u))
dphi = lambda u: q(u) ** -1.5
ddphi = lambda u: -3.0 * p0 * p0 * u * q(u) ** -2.5


def host_map(x, t, z):
    """The MAP of z given x at theta = t by Newton's method from z (fp64, sparse LU; Gauss-Newton while the curvature term is
    negative somewhere)."""
    iv = np.exp(-t)[k]
    xo = np.where(mask, x, 0.0)
    for _ in range(60):
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


model = M.ResponseModel.packaged("saturating_response")
print("header check:", M.check_model_consistency(model, link=(p0, 0.0)))
draw = M.HipMuseProblem(None, model=model, ntheta=nth, N=N, noise_sd=sd, mask=mask, link=(p0, 0.0))
x, _ = draw.sample_x_z(M.SimRng(2024, M.DATA_SIM), truth)
assert np.all(x[~mask] == 0.0)
normals = []
for sim in range(nsims):
    xs, zs = draw.sample_x_z(M.SimRng(seed, sim), [0.0] * nth)
    normals.append((zs, np.where(mask, (xs - phi(A @ zs)) / sd, 0.0)))
draw.close()

prob = M.HipMuseProblem(x, model=model, ntheta=nth, prior=M.GaussianPrior(0.0, prior_sigma), noise_sd=sd, mask=mask, link=(p0, 0.0))
assert prob.get_link() == ((p0, 0.0), True) and prob.has_second_derivatives
res = M.muse(prob, [0.0] * nth, rng=seed, nsims=nsims, maxsteps=60, theta_rtol=1e-5, grad_z_logLike_atol=1e-6, alpha=0.7,
             get_covariance=True)
sigma_fd = np.sqrt(np.diag(np.atleast_2d(res.Sigma)))
# the same covariance with get_H! by implicit differentiation (the J of the run is kept)
imp = M.MuseResult()
imp.theta, imp.J, imp.gs = res.theta, res.J, res.gs
M.get_H_(imp, prob, res.theta, rng=seed, nsims=nsims, implicit_diff=True)
sigma_imp = np.sqrt(np.diag(np.atleast_2d(imp.Sigma)))
cg = np.asarray(imp.metadata["implicit_diff_cg_hists"])
prob.close()
ref = host_root(x, normals, np.asarray(res.theta, float))
for j in range(nth):
    print(f"saturating deblur theta[{j}]: muse = {res.theta[j]:+.4f} +- {sigma_fd[j]:.4f} (implicit get_H!: +- {sigma_imp[j]:.4f})"
          f"   host root of the same gradient {ref[j]:+.4f}   (truth {truth[j]:+.1f})")
print("CG iterations per column:", int(cg.min()), "to", int(cg.max()))
assert np.all(cg > 0)
assert np.all(np.abs(np.asarray(res.theta) - np.asarray(truth)) < 5 * sigma_fd)
assert np.all(np.abs(np.asarray(res.theta) - ref) < 4 * sigma_fd / np.sqrt(nsims))
assert np.all(np.abs(sigma_imp / sigma_fd - 1.0) < 0.25)       # two estimators of the same H over the same simulations
