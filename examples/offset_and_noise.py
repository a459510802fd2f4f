"""Both get_H! branches on a model of the two-parameter family: models/offset_noise.h, z_i ~ N(0, 1), x_i ~ N(z_i + mu_k, e^tau_k).

The header states its second derivatives (MUSE_MODEL_PAIR_SECOND, include/muse_model.h), so get_H! can run by implicit differentiation
(src/muse.jl:335-405: one MAP and ntheta conjugate-gradient solves per simulation) as well as by finite differences (a fiducial MAP and
2 ntheta perturbed MAPs per simulation).  The latent field integrates out, x_i ~ N(mu_k, 1 + e^tau_k), so the answer is known."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import museinference_jl_amd as M

model = M.ElementwiseModel.packaged("offset_noise")
N, K = 20000, 2
truth = np.array([0.5, -1.0, 0.0, 1.0])     # (mu_0, mu_1, tau_0, tau_1)

sim = M.HipMuseProblem(None, model=model, ntheta=2 * K, N=N)
print("consistency of the hand-written derivatives:", M.check_model_consistency(sim, truth))
x, _ = sim.sample_x_z(M.SimRng(101, M.DATA_SIM), truth)
sim.close()

prob = M.HipMuseProblem(x, model=model, ntheta=2 * K, prior=M.GaussianPrior(0.0, 3.0))
result = M.muse(prob, np.zeros(2 * K), nsims=200, rng=0, grad_z_logLike_atol=1e-6, theta_rtol=1e-3, get_covariance=False)
M.get_J_(result, prob, nsims=200)
sigmas = {}
for how, kw in (("implicit differentiation", dict(implicit_diff=True, implicit_diff_cg_kwargs=dict(maxiter=100, reltol=1e-8))),
                ("finite differences", {})):
    result.Hs, result.H = [], None
    M.get_H_(result, prob, nsims=200, **kw)
    sigmas[how] = np.sqrt(np.diag(result.Sigma))
k = (np.arange(N) * K) // N
exact = np.array([x[k == b].mean() for b in range(K)] + [np.log(x[k == b].var() - 1.0) for b in range(K)])
names = ["mu_0", "mu_1", "tau_0", "tau_1"]
for j in range(2 * K):
    print(f"theta[{names[j]}] = {result.theta[j]:+.4f} +- {sigmas['implicit differentiation'][j]:.4f} (implicit) / "
          f"{sigmas['finite differences'][j]:.4f} (finite differences)    truth {truth[j]:+.1f}, exact marginal MLE {exact[j]:+.4f}")
for s in sigmas.values():
    assert np.all(np.abs(result.theta - truth) / s < 4.0)
    assert np.all(np.abs(result.theta - exact) / s < 0.5)
assert np.all(np.abs(sigmas["implicit differentiation"] / sigmas["finite differences"] - 1.0) < 0.1)
prob.close()
