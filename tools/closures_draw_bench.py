"""The draws of a closure problem's maps, one simulation at a time against all at once: BatchedTorchMuseProblem with the per-simulation
`sample_x_z` (a torch.Generator seeded per simulation: the loop) and with `sample_x_z_batched` on the engine's streams (EngineNormals:
one launch of muse_lbfgs_normals per request for all rows), in the same process, alternating, 7 repetitions each after one that warms
both up, the device synchronised around every timed call:

    (a) funnel closures, N = 10^4, nθ = 2, 100 simulations: the draws, one cold map (data + simulations, atol 1e-2), fd_jacobian_batch
        (2 nθ nsims = 400 perturbed rows), implicit_H_batch
    (b) the dense model of examples/closures.py scaled to 2048 x 1024, 100 simulations: the draws, one cold map

Prints ms per call: median (min - max).  "kernel" is the device time between two events recorded around the muse_lbfgs_normals
launches of one batched draw (their sum where a draw makes two requests).  The two samplers draw DIFFERENT random numbers (torch's
generator against the engine's stream), so the whole calls differ in their data too: the solver rounds are printed next to each.

    python tools/closures_draw_bench.py [a b]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M

DEV, REPS, SEED = "cuda", 7, 7


def funnel(N, nth):
    k = ((torch.arange(N) * nth) // N).to(DEV)

    def sample_x_z(gen, theta):
        z = torch.exp(theta[k] / 2) * torch.randn(N, generator=gen, device=DEV, dtype=torch.float64)
        return z + torch.randn(N, generator=gen, device=DEV, dtype=torch.float64), z

    def sample_x_z_batched(normals, theta):
        e = normals(N, 2)
        z = torch.exp(theta[:, k] / 2) * e[..., 0]
        return z + e[..., 1], z

    def logLike(x, z, theta):
        return -0.5 * (torch.sum((x - z) ** 2) + torch.sum(torch.exp(-theta[k]) * z ** 2) + torch.sum(theta[k]))
    return sample_x_z, sample_x_z_batched, logLike


def dense(m, n):
    A = torch.as_tensor(np.random.RandomState(2).randn(m, n) / np.sqrt(n), device=DEV)

    def sample_x_z(gen, theta):
        z = torch.exp(theta[0] / 2) * torch.randn(n, generator=gen, device=DEV, dtype=torch.float64)
        return A @ z + torch.randn(m, generator=gen, device=DEV, dtype=torch.float64), z

    def sample_x_z_batched(normals, theta):
        z = torch.exp(theta[:, :1] / 2) * normals(n)
        return z @ A.T + normals(m), z

    def logLike(x, z, theta):
        r = x - A @ z
        return -0.5 * (torch.sum(r * r) + torch.exp(-theta[0]) * torch.sum(z * z) + n * theta[0])
    return sample_x_z, sample_x_z_batched, logLike


CASES = {"a": ("funnel closures N=10^4, ntheta=2, 100 sims", lambda: funnel(10000, 2), np.array([0.3, -0.8]), 100, True),
         "b": ("dense 2048 x 1024, 100 sims", lambda: dense(2048, 1024), np.array([0.5]), 100, False)}


class TimedNormals(M.EngineNormals):
    """EngineNormals with two events around every launch; kernel_ms() synchronises and sums them."""

    def normals(self, *shape):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = super().normals(*shape)
        e1.record()
        self.__dict__.setdefault("events", []).append((e0, e1))
        return out

    __call__ = normals

    def kernel_ms(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events)


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def fmt(v):
    return f"{np.median(v):9.3f} ms  ({min(v):.3f} - {max(v):.3f})"


def alternate(loop, batched):
    """REPS timings of each of the two calls, alternating, after one repetition that warms both up; and the last results"""
    tl, tb = [], []
    for rep in range(REPS + 1):
        a, ra = timed(loop)
        b, rb = timed(batched)
        if rep:
            tl.append(a)
            tb.append(b)
    return tl, tb, ra, rb


def run(key):
    title, make, theta, nsims, with_H = CASES[key]
    sample_x_z, sample_x_z_batched, logLike = make()
    sims = list(range(nsims))
    draws = M.BatchedTorchMuseProblem(None, None, logLike, device=DEV, sample_x_z_batched=sample_x_z_batched)
    x, _ = draws.sample_x_z(M.SimRng(5, M.DATA_SIM), theta)
    loop = M.BatchedTorchMuseProblem(x, sample_x_z, logLike, device=DEV)
    batched = M.BatchedTorchMuseProblem(x, None, logLike, device=DEV, sample_x_z_batched=sample_x_z_batched)
    TH = batched._theta_rows(theta, nsims)
    print(f"({key}) {title}")
    # the draws alone
    kernel = []

    def draw_batched():
        normals = TimedNormals(DEV, SEED, sims)
        out = batched._draw_rows(normals, TH)
        kernel.append(normals.kernel_ms())
        return out
    tl, tb, _, _ = alternate(lambda: torch.stack([loop._draw(SEED, s, theta)[0] for s in sims]), draw_batched)
    print(f"    draws, per-simulation loop  {fmt(tl)}   {nsims} generators seeded, {nsims} calls of the closure")
    print(f"    draws, one batched call     {fmt(tb)}   kernel {fmt(kernel[1:])} (device events)")
    print(f"    draws: {np.median(tl) / np.median(tb):.1f}x")
    # the whole calls
    def report(name, fl, fb, rounds):
        tl, tb, _, _ = alternate(fl, fb)
        print(f"    {name}, loop sampler     {fmt(tl)}   {rounds(loop)}")
        print(f"    {name}, batched sampler  {fmt(tb)}   {rounds(batched)}     {np.median(tl) / np.median(tb):.2f}x")
    report("cold map (data + sims, atol 1e-2)",
           lambda: loop.map_and_score_batch(SEED, 0, nsims, theta, include_data=True, atol=1e-2, z0_mode=M.Z0_ZERO),
           lambda: batched.map_and_score_batch(SEED, 0, nsims, theta, include_data=True, atol=1e-2, z0_mode=M.Z0_ZERO),
           lambda p: f"{p.last_rounds} rounds, {p.last_syncs} synchronisations")
    if with_H:
        step = np.full(theta.size, 0.05)
        report(f"fd_jacobian_batch ({2 * theta.size * nsims} rows)",
               lambda: loop.fd_jacobian_batch(SEED, 0, nsims, theta, step), lambda: batched.fd_jacobian_batch(SEED, 0, nsims, theta, step),
               lambda p: f"{p.last_rounds} rounds in the perturbed solve")
        report("implicit_H_batch", lambda: loop.implicit_H_batch(SEED, 0, nsims, theta), lambda: batched.implicit_H_batch(SEED, 0, nsims, theta),
               lambda p: f"{p.last_cg_rounds} CG rounds, {p.last_cg_chunks} chunk(s)")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("closures_draw_bench needs a GPU (there is no CPU path)")
    for key in (sys.argv[1:] or list(CASES)):
        run(key)
