"""The implicit-differentiation get_H! with CG preconditioned by the Hessian's diagonal (MUSE_IMPLICIT_PL_JACOBI) against the default
loop, on the same build and in one session: `python tools/implicit_jacobi_bench.py [reps] [nsims] [N]` alternates one
implicit_H_batch call at the defaults with one at cg_Pl="jacobi", `reps` times after a warm-up of each (libraries loaded, buffers
allocated, normals cache warm), at two shapes -- models/offset_noise.h with 4 components (the shape of profiles/r07_pair_implicit_vs_fd.txt)
and models/cubic.h with 2 (the packaged header: its d2 o / dz2 depends on the MAP, so the diagonal differs from element to element) --
and prints per repetition the wall ms of the call and the launch's own ms (its event pair), with medians and spreads, and the default
path's CG iteration counts over the columns (profiles/r10_implicit_jacobi.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import museinference_jl_amd as M

reps, nsims, N = (int(v) for v in (sys.argv[1:4] + ["7", "512", "10000"][len(sys.argv) - 1:]))
SHAPES = [("offset_noise", np.array([-0.2, 0.3, 0.4, -0.3])), ("cubic", np.array([0.5, -0.3]))]
for name, theta in SHAPES:
    prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged(name), ntheta=theta.size, N=N)
    prob.set_timing(True)
    calls = {"default": lambda: prob.implicit_H_batch(7, 0, nsims, theta, atol=1e-1),
             "jacobi": lambda: prob.implicit_H_batch(7, 0, nsims, theta, atol=1e-1, cg_Pl="jacobi")}
    series = {k: {"wall": [], "kernel": []} for k in calls}
    out = {}
    for c in calls.values():
        c()
    for r in range(reps):
        for k in (("default", "jacobi") if r % 2 == 0 else ("jacobi", "default")):
            prob.synchronize()
            t0 = time.perf_counter()
            out[k] = calls[k]()
            series[k]["wall"].append(1e3 * (time.perf_counter() - t0))
            series[k]["kernel"].append(prob.last_kernel_ms())
    itd, itj = out["default"][1], out["jacobi"][1]
    scale = np.abs(out["default"][0]).max()
    print(f"{name} N={N} ntheta={theta.size} nsims={nsims} atol=1e-1, {reps} alternating repetitions")
    print(f"  CG iterations over the columns: default min {itd.min()} median {np.median(itd):.0f} max {itd.max()}; "
          f"jacobi min {itj.min()} median {np.median(itj):.0f} max {itj.max()}; "
          f"max |H_jacobi - H_default| / max |H| = {np.abs(out['jacobi'][0] - out['default'][0]).max() / scale:.2e}")
    for k, s in series.items():
        for what, v in s.items():
            v = np.array(v)
            print(f"  {k:8s} {what:6s} ms: " + " ".join(f"{t:.3f}" for t in v) +
                  f"   median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} spread {v.max() - v.min():.3f}")
    kd, kj = np.array(series["default"]["kernel"]), np.array(series["jacobi"]["kernel"])
    print(f"  jacobi - default, kernel medians: {np.median(kj) - np.median(kd):+.3f} ms; the default's own spread: {kd.max() - kd.min():.3f} ms")
    prob.close()
