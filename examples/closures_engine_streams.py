"""A closure problem on the ENGINE's random streams: the funnel written as torch closures, its simulations drawn all at once by
`sample_x_z_batched` from EngineNormals (include/muse_lbfgs.h, muse_lbfgs_normals: the stream HipMuseProblem gives its elements,
evaluated for every row of a map in one launch), next to HipMuseProblem(model="funnel") with the same seed.

    z_i ~ Normal(0, exp(theta_k(i) / 2)),      x_i ~ Normal(z_i, 1)        two blocks of elements, one theta each

Element i of simulation s takes the pair (n1, n2) = normal_pair(seed, s, i) in both: `normals(N, 2)[b, i] = (n1(i), n2(i))` of row b's
simulation.  The two problems therefore see the SAME simulations, and muse() -- the same host loop for both (native=False) -- walks the
same θ trajectory; what is left between them is rounding (torch's exp against the engine's fixed sequence, the order of the sums),
carried through MAPs solved to 1e-8.  The bound asserted on every iterate is 1e-6.

    python examples/closures_engine_streams.py          (needs a GPU: neither class has a CPU fallback)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M

dev = "cuda"
N, nth, truth = 1000, 2, [0.5, -0.5]
k = ((torch.arange(N) * nth) // N).to(dev)        # the block of element i
ATOL = 1e-6     # the stated bound between the two trajectories


def sample_x_z_batched(normals, theta):          # theta [B, nθ]: row b is simulation b's own
    e = normals(N, 2)
    z = torch.exp(theta[:, k] / 2) * e[..., 0]
    return z + e[..., 1], z


def logLike(x, z, theta):
    return -0.5 * (torch.sum((x - z) ** 2) + torch.sum(torch.exp(-theta[k]) * z ** 2) + torch.sum(theta[k]))


def logLike_batched(x, z, theta):
    th = theta[:, k]
    return -0.5 * (torch.sum((x - z) ** 2, dim=-1) + torch.sum(torch.exp(-th) * z ** 2, dim=-1) + torch.sum(th, dim=-1))


logPrior = lambda theta: -0.5 * torch.sum(theta ** 2) / 9.0


def main():
    kw = dict(rng=3, nsims=50, maxsteps=12, theta_rtol=1e-4, grad_z_logLike_atol=1e-8, alpha=1.0, native=False)
    closures = M.BatchedTorchMuseProblem(None, None, logLike, logPrior, device=dev, logLike_batched=logLike_batched,
                                         sample_x_z_batched=sample_x_z_batched)
    x, _ = closures.sample_x_z(M.SimRng(1234, M.DATA_SIM), truth)           # the data: one draw at the truth
    closures = M.BatchedTorchMuseProblem(x, None, logLike, logPrior, device=dev, logLike_batched=logLike_batched,
                                         sample_x_z_batched=sample_x_z_batched)
    engine = M.HipMuseProblem(x.cpu().numpy(), model="funnel", ntheta=nth, prior=M.GaussianPrior(0.0, 3.0))
    a = M.muse(closures, [0.0, 0.0], **kw)
    b = M.muse(engine, [0.0, 0.0], **kw)
    engine.close()
    ta, tb = np.array([h["θ"] for h in a.history]), np.array([h["θ"] for h in b.history])
    print("iteration   closures on engine streams        HipMuseProblem(model=\"funnel\")")
    for i in range(max(len(ta), len(tb))):
        row = lambda t: "  ".join(f"{v:+.10f}" for v in t[i]) if i < len(t) else " " * 28
        print(f"{i + 1:9d}   {row(ta)}      {row(tb)}")
    diff = float(np.abs(ta - tb).max()) if ta.shape == tb.shape else float("inf")
    print(f"iterations {len(ta)} and {len(tb)}; max |difference of theta| over the trajectory {diff:.3e}")
    return diff


if __name__ == "__main__":
    assert main() <= ATOL
