"""One get_H! map by implicit differentiation (implicit_H_batch, fiducial MAPs to atol 1e-1 as the driver asks) through the serial
TorchMuseProblem and through BatchedTorchMuseProblem, in the same process, alternating, 7 repetitions each after one that warms both
up, the device synchronised around every call:

    (a) funnel closures, N = 10^4, nθ = 2, 100 simulations
    (b) the dense model of examples/closures.py scaled to 2048 x 1024, 32 simulations

The serial class takes one simulation after another, and each costs 2 N reverse passes for its two Jacobians of ∇z: it is timed on
its first --serial-sims simulations (default 2) and reported per simulation and scaled to the whole call, which says so.  Prints ms
per call (median, min - max), the batched call's CG rounds and synchronisations, the device time per CG advance, and where the
batched call's time goes (draws, fiducial MAPs, derivative terms, the CG loop, the epilogue).

    python tools/closures_implicit_bench.py [a b] [--serial-sims K]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import museinference_jl_amd as M

DEV, REPS = "cuda", 7


def funnel(N, nth):
    k = ((torch.arange(N) * nth) // N).to(DEV)

    def sample_x_z(gen, theta):
        z = torch.exp(theta[k] / 2) * torch.randn(N, generator=gen, device=DEV, dtype=torch.float64)
        return z + torch.randn(N, generator=gen, device=DEV, dtype=torch.float64), z

    def logLike(x, z, theta):
        return -0.5 * (torch.sum((x - z) ** 2) + torch.sum(torch.exp(-theta[k]) * z ** 2) + torch.sum(theta[k]))
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


CASES = {"a": ("funnel closures N=10^4, ntheta=2, 100 sims", lambda: funnel(10000, 2), np.array([0.3, -0.8]), 100),
         "b": ("dense 2048 x 1024, 32 sims", lambda: dense(2048, 1024), np.array([0.5]), 32)}


class Phases:
    """Wall time of the batched call's phases: the device synchronised at each boundary (its own run, not the timed one)."""

    def __init__(self, prob):
        self.prob, self.t = prob, {}

    def wrap(self, name, attr):
        inner = getattr(self.prob, attr)

        def timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*a, **k)
            torch.cuda.synchronize()
            self.t[name] = self.t.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
            return out
        setattr(self.prob, attr, timed)


def run(key, serial_sims):
    title, make, theta, nsims = CASES[key]
    sample_x_z, logLike = make()
    serial = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    batched = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    batched.cg_timing = True
    ks = min(serial_sims, nsims)
    ts, tb, adv = [], [], []
    for rep in range(REPS + 1):     # (repetition 0 warms both up and is dropped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Hs, its = serial.implicit_H_batch(7, 0, ks, theta)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        Hb, itb = batched.implicit_H_batch(7, 0, nsims, theta)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            ts.append(1e3 * (t1 - t0) / ks)
            tb.append(1e3 * (t2 - t1))
            adv.append(batched.last_cg_advance_ms / max(batched.last_cg_rounds, 1))
    rounds, syncs, chunks = batched.last_cg_rounds, batched.last_cg_syncs, batched.last_cg_chunks
    # where the batched call's time goes: one more call with the device synchronised around its phases
    ph = Phases(batched)
    ph.wrap("draws", "_draw")
    ph.wrap("fiducial MAPs", "_solve")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batched.implicit_H_batch(7, 0, nsims, theta)
    torch.cuda.synchronize()
    total = 1e3 * (time.perf_counter() - t0)
    f = lambda v: f"{np.median(v):10.2f} ms  ({min(v):.2f} - {max(v):.2f})"
    whole = [t * nsims for t in ts]
    print(f"({key}) {title}")
    print(f"    serial   {f(ts)} per simulation, timed on {ks} of {nsims}; the whole call at that rate: {f(whole)}")
    print(f"    batched  {f(tb)} for all {nsims}   {rounds} CG rounds, {syncs} synchronisations, {chunks} chunk(s), "
          f"{np.median(adv):.3f} ms per CG advance (device)")
    print(f"    speed-up {np.median(whole) / np.median(tb):.1f}x on the whole call   CG counts equal on the first {ks}: "
          f"{bool(np.array_equal(its, itb[:ks]))} (serial {its.ravel().tolist()}), max |dH| {float(np.abs(Hs - Hb[:ks]).max()):.1e} of |H| "
          f"{float(np.abs(Hs).max()):.1e}")
    rest = total - sum(ph.t.values())
    print(f"    batched phases ({total:.2f} ms with a synchronisation around each): " + ", ".join(f"{k} {v:.2f} ms" for k, v in ph.t.items())
          + f", CG advances {batched.last_cg_advance_ms:.2f} ms (device), derivative terms + the closure's double backward per round + epilogue {rest - batched.last_cg_advance_ms:.2f} ms")


if __name__ == "__main__":
    args = sys.argv[1:]
    serial_sims = 2
    if "--serial-sims" in args:
        i = args.index("--serial-sims")
        serial_sims = int(args[i + 1])
        del args[i:i + 2]
    for key in (args or list(CASES)):
        run(key, serial_sims)
