"""One cold map (data + simulations, from z = 0) through the serial TorchMuseProblem and through BatchedTorchMuseProblem, in the same
process, alternating, 7 repetitions each, the device synchronised around every map:

    (a) funnel closures, N = 10^4, 100 simulations, atol 1e-2
    (b) the dense model of examples/closures.py scaled to 2048 x 1024, 100 simulations
    (c) funnel closures, N = 10^5, 16 simulations: one workgroup per problem is expected to run out here; ms per advance is reported

Prints ms per map (median, min - max), the batched map's rounds and synchronisations, the device time of its advance launches, and the
serial map's evaluation count (each evaluation of the serial solver synchronises about 20 times: optim.py's float(...) calls).

    python tools/closures_bench.py [a b c]
"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M

driver = importlib.import_module("museinference_jl_amd.muse")     # (the package's attribute `muse` is the function)

DEV, REPS = "cuda", 7


def funnel(N):
    def sample_x_z(gen, theta):
        z = torch.exp(theta[0] / 2) * torch.randn(N, generator=gen, device=theta.device, dtype=theta.dtype)
        return z + torch.randn(N, generator=gen, device=theta.device, dtype=theta.dtype), z

    def logLike(x, z, theta):
        return -0.5 * (torch.sum((x - z) ** 2) + torch.exp(-theta[0]) * torch.sum(z ** 2) + N * theta[0])
    return sample_x_z, logLike


def dense(m, n):
    A = torch.as_tensor(np.random.RandomState(2).randn(m, n) / np.sqrt(n), device=DEV)

    def sample_x_z(gen, theta):
        z = torch.exp(theta[0] / 2) * torch.randn(n, generator=gen, device=DEV, dtype=torch.float64)
        return A @ z + torch.randn(m, generator=gen, device=DEV, dtype=torch.float64), z

    def logLike(x, z, theta):
        r = x - A @ z
        return -0.5 * (torch.sum(r * r) + torch.exp(-theta[0]) * torch.sum(z * z) + n * theta[0])
    return sample_x_z, logLike


CASES = {"a": ("funnel closures N=10^4, 100 sims, atol 1e-2", lambda: funnel(10000), 100, 1e-2),
         "b": ("dense 2048 x 1024, 100 sims, atol 1e-2", lambda: dense(2048, 1024), 100, 1e-2),
         "c": ("funnel closures N=10^5, 16 sims, atol 1e-2", lambda: funnel(100000), 16, 1e-2)}


def run(key):
    title, make, nsims, atol = CASES[key]
    sample_x_z, logLike = make()
    theta = np.array([0.5])
    x, _ = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV).sample_x_z(M.SimRng(1, M.DATA_SIM), theta)
    serial = M.TorchMuseProblem(x, sample_x_z, logLike, device=DEV)
    batched = M.BatchedTorchMuseProblem(x, sample_x_z, logLike, device=DEV)
    ts, tb, adv, evals = [], [], [], 0
    for rep in range(REPS + 1):     # (repetition 0 warms both up and is dropped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gs, _, _, infos = driver._map_serial(serial, 7, theta, theta, range(nsims), True, None, atol, M.Z0_ZERO)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if batched._batch is not None:
            batched._batch.timing, batched._batch.advance_ms = True, 0.0
        g, info = batched.map_and_score_batch(7, 0, nsims, theta, include_data=True, atol=atol, z0_mode=M.Z0_ZERO)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            ts.append(1e3 * (t1 - t0))
            tb.append(1e3 * (t2 - t1))
            adv.append(batched._batch.advance_ms / batched.last_rounds)
            evals = int(sum(int(i["f_calls"]) for i in infos))
    same = bool(np.array_equal(info["f_calls"], [int(i["f_calls"]) for i in infos]))
    f = lambda v: f"{np.median(v):9.2f} ms  ({min(v):.2f} - {max(v):.2f})"
    print(f"({key}) {title}")
    print(f"    serial   {f(ts)}   {evals} evaluations, one simulation at a time")
    print(f"    batched  {f(tb)}   {batched.last_rounds} rounds, {batched.last_syncs} synchronisations, {np.median(adv):.3f} ms per advance (device)")
    print(f"    speed-up {np.median(ts) / np.median(tb):.1f}x   (serial spread {max(ts) - min(ts):.2f} ms); evaluation counts equal: {same}, "
          f"max rel score difference {float(np.abs(g / gs - 1).max()):.1e}")


if __name__ == "__main__":
    for key in (sys.argv[1:] or list(CASES)):
        run(key)
