"""Deblurring with a noise level that changes from pixel to pixel and pixels that were never observed: the coupled `smooth` model
with the noise as state of the problem.

    z_i ~ N(0, e^{theta_k}),   x_i = (A z)_i + sd_i n_i  where observed,   A the periodic (1/4, 1/2, 1/4) blur

A field with two variance components is blurred, a noise ramp sd in [0.5, 2] is added and a stripe of pixels is masked; muse() runs
on the HIP path with the noise map and the mask read by the kernels at run time (HipMuseProblem(..., noise_sd=..., mask=...)), and
the answer is set next to the exact marginal posterior: the model is jointly Gaussian, so d log p(x | theta) / d theta_k =
1/2 (e^{-theta_k} (sum_k z*^2 + tr_k H^-1) - n_k) with z* the posterior mean and H = A^T Omega A + diag(e^{-theta}) its precision,
a periodic pentadiagonal matrix whose inverse's diagonal costs O(N)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl
from scipy.linalg import cholesky_banded, cho_solve_banded
from scipy.optimize import root

import museinference_jl_amd as M

N, nth, truth, nsims, prior_sigma = 8192, 2, [1.0, 0.2], 128, 3.0
sd = np.linspace(0.5, 2.0, N)
mask = np.ones(N, bool)
mask[3000:3400] = False           # the stripe
mask[[0, N - 1]] = False          # ... and the two pixels next to the periodic wrap


def diag_of_inverse(H):
    """diag(H^-1), H symmetric positive definite with cyclic bandwidth 2: the last two indices as a border around a banded block
    (Schur complement), the block's part by the Takahashi recurrence on its banded Cholesky factor."""
    n = H.shape[0] - 2
    ab = np.zeros((3, n))
    for d in range(3):
        ab[2 - d, d:] = H[:n, :n].diagonal(d)
    cb = cholesky_banded(ab)
    U, D = H[:n, n:].toarray(), H[n:, n:].toarray()
    BU = cho_solve_banded((cb, False), U)
    Sinv = np.linalg.inv(D - U.T @ BU)
    r0, r1, r2 = cb[2], np.append(cb[1][1:], [0.0]), np.append(cb[0][2:], [0.0, 0.0])
    z0, z1, z2 = np.zeros(n + 2), np.zeros(n + 2), np.zeros(n + 2)
    for i in range(n - 1, -1, -1):
        z1[i] = -(r1[i] * z0[i + 1] + r2[i] * z1[i + 1]) / r0[i]
        z2[i] = -(r1[i] * z1[i + 1] + r2[i] * z0[i + 2]) / r0[i]
        z0[i] = (1.0 / r0[i] - r1[i] * z1[i] - r2[i] * z2[i]) / r0[i]
    return np.concatenate([z0[:n] + np.einsum("ia,ab,ib->i", BU, Sinv, BU), np.diag(Sinv)])


def exact_posterior(x):
    k = (np.arange(N) * nth) // N
    om = np.where(mask, 1.0 / (sd * sd), 0.0)
    i = np.arange(N)
    A = sp.csc_matrix((np.concatenate([np.full(N, 0.5), np.full(N, 0.25), np.full(N, 0.25)]),
                       (np.concatenate([i, i, i]), np.concatenate([i, (i - 1) % N, (i + 1) % N]))), shape=(N, N))
    b = A.T @ (om * np.where(mask, x, 0.0))

    def grad(t):
        H = (A.T @ sp.diags(om) @ A + sp.diags(np.exp(-t)[k])).tocsc()
        zs = spl.splu(H).solve(b)
        e2 = zs * zs + diag_of_inverse(H)
        return 0.5 * (np.exp(-t) * np.array([e2[k == j].sum() for j in range(nth)]) - np.bincount(k)) - t / prior_sigma ** 2
    mode = root(grad, np.zeros(nth), tol=1e-10).x
    J = np.stack([(grad(mode + h) - grad(mode - h)) / 2e-4 for h in 1e-4 * np.eye(nth)], axis=1)
    return mode, np.sqrt(np.diag(np.linalg.inv(-0.5 * (J + J.T))))


draw = M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, noise_sd=sd, mask=mask)
x, _ = draw.sample_x_z(M.SimRng(2024, M.DATA_SIM), truth)
draw.close()
assert np.all(x[~mask] == 0.0)
prob = M.HipMuseProblem(x, model="smooth", ntheta=nth, prior=M.GaussianPrior(0.0, prior_sigma), noise_sd=sd, mask=mask)
res = M.muse(prob, [0.0] * nth, rng=1, nsims=nsims, maxsteps=40, theta_rtol=1e-5, grad_z_logLike_atol=1e-6, get_covariance=True)
mode, sigma = exact_posterior(x)
got = np.sqrt(np.diag(np.atleast_2d(res.Sigma)))
for j in range(nth):
    print(f"masked deblur theta[{j}]: muse = {res.theta[j]:+.4f} +- {got[j]:.4f}   exact posterior {mode[j]:+.4f} +- {sigma[j]:.4f}"
          f"   (truth {truth[j]:+.1f}; Monte-Carlo error of the mode {sigma[j] / np.sqrt(nsims):.4f})")
assert np.all(np.abs(np.asarray(res.theta) - mode) < 5 * sigma / np.sqrt(nsims)) and np.all(np.abs(got / sigma - 1) < 0.3)
prob.close()
