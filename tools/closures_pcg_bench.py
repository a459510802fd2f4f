"""One get_H! map by implicit differentiation through BatchedTorchMuseProblem (implicit_H_batch, fiducial MAPs to atol 1e-1 as the driver
asks) with plain conjugate gradients and with cg_Pl="jacobi", on closure models with badly scaled latents; the sibling of
tools/closures_implicit_bench.py.  Both variants run in the same process on the same problem object, alternating, 7 repetitions each
after one that warms both up, the device synchronised around every call:

    (a) heteroscedastic elementwise closures  z ~ N(0, e^θ0), x_i ~ N(z_i, σ_i² e^θ1), σ_i = exp(sin(1.7 i)); N = 10^4, nθ = 2, 100
        simulations; hess_diag = "elementwise" (one Hessian-vector product over the 100 simulations forms the diagonal)
    (b) the scaled dense model  x = A (w ⊙ z) + e, w_i = exp(2 sin(1.7 i + 0.3)), at 2048 x 1024, 32 simulations; hess_diag = the
        callable w_i² (AᵀA)_ii + e^-θ

Prints, per variant: ms per call (median, min - max), the CG rounds and synchronisations, the device time of the CG advance launches
(summed over the call, and per advance), the CG counts' range; and between the variants the largest |dH|.

    python tools/closures_pcg_bench.py [a b] [--out FILE]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M

DEV, REPS = "cuda", 7


def hetero(N):
    sig = torch.exp(torch.sin(1.7 * torch.arange(N, dtype=torch.float64))).to(DEV)

    def sample_x_z(gen, theta):
        z = torch.exp(theta[0] / 2) * torch.randn(N, generator=gen, device=DEV, dtype=torch.float64)
        return z + sig * torch.exp(theta[1] / 2) * torch.randn(N, generator=gen, device=DEV, dtype=torch.float64), z

    def logLike(x, z, theta):
        return -0.5 * (torch.exp(-theta[1]) * torch.sum(((x - z) / sig) ** 2) + N * theta[1] + torch.exp(-theta[0]) * torch.sum(z ** 2) + N * theta[0])
    return sample_x_z, logLike, "elementwise"


def scaled_dense(m, n):
    A = torch.as_tensor(np.random.RandomState(2).randn(m, n) / np.sqrt(n), device=DEV)
    w = torch.exp(2.0 * torch.sin(1.7 * torch.arange(n, dtype=torch.float64) + 0.3)).to(DEV)
    ata = torch.sum(A * A, dim=0)

    def sample_x_z(gen, theta):
        z = torch.exp(theta[0] / 2) * torch.randn(n, generator=gen, device=DEV, dtype=torch.float64)
        return A @ (w * z) + torch.randn(m, generator=gen, device=DEV, dtype=torch.float64), z

    def logLike(x, z, theta):
        r = x - A @ (w * z)
        return -0.5 * (torch.sum(r * r) + torch.exp(-theta[0]) * torch.sum(z * z) + n * theta[0])

    def hess_diag(x, z, theta):
        return w ** 2 * ata + torch.exp(-theta[:, 0:1]) + 0.0 * z
    return sample_x_z, logLike, hess_diag


CASES = {"a": ("heteroscedastic elementwise closures N=10^4, ntheta=2, 100 sims", lambda: hetero(10000), np.array([0.3, -0.5]), 100),
         "b": ("scaled dense 2048 x 1024, 32 sims", lambda: scaled_dense(2048, 1024), np.array([0.5]), 32)}


def run(key, out):
    title, make, theta, nsims = CASES[key]
    sample_x_z, logLike, hess_diag = make()
    prob = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV, hess_diag=hess_diag)
    prob.cg_timing = True
    variants = {"plain": None, "jacobi": "jacobi"}
    t, adv, stats, H = {k: [] for k in variants}, {k: [] for k in variants}, {}, {}
    for rep in range(REPS + 1):     # (repetition 0 warms both up and is dropped)
        for name, Pl in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            H[name], its = prob.implicit_H_batch(7, 0, nsims, theta, cg_Pl=Pl)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep:
                t[name].append(1e3 * (t1 - t0))
                adv[name].append(prob.last_cg_advance_ms)
            stats[name] = (prob.last_cg_rounds, prob.last_cg_syncs, prob.last_cg_chunks, int(its.min()), int(its.max()))
    f = lambda v: f"{np.median(v):10.2f} ms  ({min(v):.2f} - {max(v):.2f})"
    out(f"({key}) {title}")
    for name in variants:
        rounds, syncs, chunks, kmin, kmax = stats[name]
        out(f"    {name:7s}{f(t[name])} per call   {rounds} CG rounds, {syncs} synchronisations, {chunks} chunk(s), CG counts {kmin} - {kmax}, "
            f"CG advances {np.median(adv[name]):.3f} ms (device) per call, {np.median(adv[name]) / max(rounds, 1):.4f} ms per advance")
    out(f"    call time plain / jacobi {np.median(t['plain']) / np.median(t['jacobi']):.2f}   max |dH| {float(np.abs(H['plain'] - H['jacobi']).max()):.1e} "
        f"of |H| {float(np.abs(H['plain']).max()):.1e} (both at the default reltol sqrt(eps); a plain count at maxiter = 100 has not converged)")


if __name__ == "__main__":
    args = sys.argv[1:]
    sink = None
    if "--out" in args:
        i = args.index("--out")
        os.makedirs(os.path.dirname(os.path.abspath(args[i + 1])), exist_ok=True)
        sink = open(args[i + 1], "w")
        del args[i:i + 2]

    def out(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    for key in (args or list(CASES)):
        run(key, out)
