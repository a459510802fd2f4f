"""Stochastic volatility -- Neal's funnel proper -- on the fast path: a model whose latent enters through its exponential PER ELEMENT
(include/muse_model.h, EXPONENTIALS),

    z_i ~ Normal(mu, exp(tau / 2)),      x_i ~ Normal(0, exp(z_i / 2))            theta = (mu, tau)

1. The model from its TERMS: ElementwiseModel.from_pair_expressions takes `exp` in the objective and in the draw, differentiates
   symbolically and writes the header -- muse_model_exp(...) once per function body.  models/stochastic_volatility.h, the shipped
   header this script runs, is that text with hand-chosen names.
2. muse() on HipMuseProblem with the covariance: theta_hat +- sigma next to the truth.
3. The same model as torch closures on the ENGINE's random streams (BatchedTorchMuseProblem with sample_x_z_batched: element i of
   simulation s takes the engine's normal pair), so that both problems see the same simulations: the scores of one map agree to
   rtol 1e-9, and the measured agreement is printed.  What is left between them is torch's exp against the engine's fixed sequence
   -- at most an ulp in the draw -- and the order of the sums, carried through two independent MAP solves.  Those have to be
   solved that far: from zero, L-BFGS ends on Optim's rule "the value did not change twice" -- a value of ~N/2 = 5000 stops
   changing in its last bit at gradients of 1e-8 to 1e-7 per element, whatever tolerance is asked, and scores of such MAPs differ
   by 3.5e-9 -- so each problem restarts warm from its resident MAPs (z0_mode = Z0_WARM, what muse() does between iterations)
   until every solve's gradient norm is below 1e-9: three restarts each on an MI355X, agreement 3.2e-11.

    python examples/stochastic_volatility.py          (needs a GPU: neither class has a CPU fallback)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M
from museinference_jl_amd.symbolic import pair_header_from_expressions

TERMS = dict(coefs=["a", "exp(b/2)", "exp(-b)", "1"], C="b", o="x**2*exp(-z) + c3*z + c2*(z - c0)**2", z="c0 + c1*n1", x="exp(z/2)*n2")
N, truth = 10000, [-0.5, 0.4]
RTOL = 1e-9     # the stated agreement of one map's scores
MAP_ATOL = 1e-9     # ... of MAPs solved to this gradient norm
dev = "cuda"


def sample_x_z_batched(normals, theta):          # theta [B, 2]: row b is simulation b's own (mu, tau)
    e = normals(N, 2)
    z = theta[:, 0:1] + torch.exp(theta[:, 1:2] / 2) * e[..., 0]
    return torch.exp(z / 2) * e[..., 1], z


def logLike(x, z, theta):
    return -0.5 * (torch.sum(x * x * torch.exp(-z) + z) + torch.exp(-theta[1]) * torch.sum((z - theta[0]) ** 2) + N * theta[1])


def logLike_batched(x, z, theta):
    mu, tau = theta[:, 0:1], theta[:, 1:2]
    return -0.5 * (torch.sum(x * x * torch.exp(-z) + z, dim=-1) + torch.sum(torch.exp(-tau) * (z - mu) ** 2, dim=-1) + N * theta[:, 1])


logPrior = lambda theta: -0.5 * torch.sum(theta ** 2) / 9.0


def solved_map(prob, theta, max_restarts=8):
    """One map (the data and 16 simulations) with every MAP's gradient norm below MAP_ATOL: from zero, then warm from the resident
    MAPs while a solve ended above it (on the unchanged-value rule).  Returns (scores, solver records, restarts)."""
    g, info = prob.map_and_score_batch(7, 0, 16, theta, include_data=True, atol=MAP_ATOL, z0_mode=0)
    restarts = 0
    while float(np.max(np.asarray(info["gnorm"]))) > MAP_ATOL and restarts < max_restarts:
        g, info = prob.map_and_score_batch(7, 0, 16, theta, include_data=True, atol=MAP_ATOL, z0_mode=M.Z0_WARM)
        restarts += 1
    return g, info, restarts


def main():
    text = pair_header_from_expressions("sv_from_terms", **TERMS)
    grad = text.split("MUSE_MODEL_FN double muse_model_grad")[1].split("\n}")[0]
    print("muse_model_grad as generated from the terms:" + grad + "\n}\n")
    model = M.ElementwiseModel.packaged("stochastic_volatility")
    sim = M.HipMuseProblem(None, model=model, ntheta=2, N=N)
    x, _ = sim.sample_x_z(M.SimRng(2024, M.DATA_SIM), truth)
    sim.close()
    engine = M.HipMuseProblem(x, model=model, ntheta=2, prior=M.GaussianPrior(0.0, 3.0))
    res = M.muse(engine, [0.0, 0.0], rng=11, nsims=100, maxsteps=30, theta_rtol=1e-3, grad_z_logLike_atol=1e-4, get_covariance=True)
    sigma = np.sqrt(np.diag(res.Sigma))
    for name, t, s, tr in zip(("mu", "tau"), res.theta, sigma, truth):
        print(f"{name:4s} {t:+.4f} +- {s:.4f}   (truth {tr:+.2f}, {abs(t - tr) / s:.2f} sigma)")
    closures = M.BatchedTorchMuseProblem(torch.as_tensor(x, device=dev), None, logLike, logPrior, device=dev, logLike_batched=logLike_batched,
                                         sample_x_z_batched=sample_x_z_batched)
    theta = [-0.3, 0.2]
    (ga, ia, ra), (gb, ib, rb) = solved_map(engine, theta), solved_map(closures, theta)
    engine.close()
    gb = np.asarray(gb)
    rel = float(np.max(np.abs(ga - gb) / np.maximum(np.abs(ga), 1.0)))
    print(f"one map of 16 simulations and the data at theta = {theta}, gradients below {MAP_ATOL:g}: HipMuseProblem {ra} warm restarts "
          f"(gradient norm {float(np.max(ia['gnorm'])):.2e}), closures {rb} ({float(np.max(np.asarray(ib['gnorm']))):.2e}); "
          f"max relative difference of the scores {rel:.3e}")
    return rel, res.theta, sigma


if __name__ == "__main__":
    rel, theta, sigma = main()
    assert rel <= RTOL
