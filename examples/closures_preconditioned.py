"""implicit_diff_cg_kwargs={"Pl": "jacobi"} for a closure problem: get_H! by implicit differentiation through BatchedTorchMuseProblem on a
model whose latents are badly scaled, with and without the diagonal preconditioner.

    z ~ Normal(0, exp(theta / 2) I_256),      x ~ Normal(A (w ⊙ z), I_384)        A: a dense 384 x 256 matrix, w_i = exp(2 sin(1.7 i + 0.3))

The Hessian of -logLike in z is W AᵀA W + e^-θ I: the weights spread its spectrum over e^8, and plain conjugate gradients need many
rounds -- each one a double backward pass of the closure over all simulations, a launch and a synchronisation.  The constructor's
`hess_diag` says what "jacobi" means for the closure; here a callable returns the diagonal w_i² (AᵀA)_ii + e^-θ (a tensor of probes or
"elementwise" would have it formed from Hessian-vector products instead).  The diagonal only preconditions: the two H agree to the
solves' tolerance -- asserted here at 1e-6 |H| with reltol 1e-10 -- and only the counts move.

    python examples/closures_preconditioned.py          (needs a GPU: the batched class has no CPU fallback)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M

dev = "cuda"
n, m, truth = 256, 384, 0.4
A = torch.as_tensor(np.random.RandomState(2).randn(m, n) / np.sqrt(n), device=dev)
w = torch.exp(2.0 * torch.sin(1.7 * torch.arange(n, dtype=torch.float64) + 0.3)).to(dev)
ata = torch.sum(A * A, dim=0)


def sample_x_z(gen, theta):
    z = torch.exp(theta[0] / 2) * torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
    return A @ (w * z) + torch.randn(m, generator=gen, device=dev, dtype=torch.float64), z


def logLike(x, z, theta):
    r = x - A @ (w * z)
    return -0.5 * (torch.sum(r * r) + torch.exp(-theta[0]) * torch.sum(z * z) + n * theta[0])


def hess_diag(x, z, theta):          # x [B, m], z [B, n], theta [B, 1] -> [B, n]: the diagonal of -∂²logLike/∂z²
    return w ** 2 * ata + torch.exp(-theta[:, 0:1]) + 0.0 * z


RTOL = 1e-6     # the stated bound between the two H
CG = {"maxiter": 2000, "reltol": 1e-10}


def main():
    prob = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=dev, hess_diag=hess_diag)
    nsims, out = 16, {}
    for name, kw in (("plain", CG), ("jacobi", dict(CG, Pl="jacobi"))):
        res = M.MuseResult()
        res.theta = np.array([truth])
        M.get_H_(res, prob, rng=1, nsims=nsims, implicit_diff=True, implicit_diff_cg_kwargs=kw)
        counts = np.array(res.metadata["implicit_diff_cg_hists"])
        out[name] = (res.H, counts, prob.last_cg_rounds, prob.last_cg_syncs)
        print(f"H with {name:6s} CG  {res.H[0, 0]:+.12f}   ({nsims} simulations; CG iterations {counts.min()} - {counts.max()} per solve, "
              f"{prob.last_cg_rounds} rounds and {prob.last_cg_syncs} synchronisations for all of them)")
    return out


if __name__ == "__main__":
    out = main()
    Hp, Hj = out["plain"][0], out["jacobi"][0]
    assert np.all(np.abs(Hp - Hj) <= RTOL * np.abs(Hp).max()), (Hp, Hj)
    assert out["jacobi"][1].max() < out["plain"][1].min(), (out["jacobi"][1], out["plain"][1])
