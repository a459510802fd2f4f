"""The stencil model's run-time-weights kernels against the built-in kernels on BASELINE.json's configs[4] share (smooth, N = 10^5,
8 theta, 128 sims, atol 1e-2 from zero): `python tools/stencil_taps_bench.py [reps] [nsims]` alternates one map of a context that
never called muse_set_stencil (the built-in kernels: byte for byte the parent commit's, tools/code_hash.py) with one of a context
at set_stencil((0.5, 0.25)) (the same bits from the kernels that read the weights), `reps` times after a warm-up of each, and
prints both series -- kernel ms from the launch's own event pair, and wall ms -- with their spread (profiles/r08_stencil_taps.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import museinference_jl_amd as M

reps, nsims = (int(v) for v in (sys.argv[1:3] + ["7", "128"][len(sys.argv) - 1:]))
N, nth = 100000, 8
theta = [1.0] * nth
probs = {"builtin": M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N),
         "runtime": M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, stencil=(0.5, 0.25))}
series = {k: {"kernel": [], "wall": []} for k in probs}
out = {}
for p in probs.values():
    p.set_timing(True)
    p.set_normals_cache(False)      # every map draws its simulations: the whole kernel, as bench.py's plain run times it
    p.map_and_score_batch(0, 0, nsims, theta, atol=1e-2)
for r in range(reps):
    for name in (("builtin", "runtime") if r % 2 == 0 else ("runtime", "builtin")):
        p = probs[name]
        p.synchronize()
        t0 = time.perf_counter()
        out[name] = p.map_and_score_batch(0, 0, nsims, theta, atol=1e-2)
        series[name]["wall"].append(1e3 * (time.perf_counter() - t0))
        series[name]["kernel"].append(p.last_kernel_ms())
assert out["builtin"][0].tobytes() == out["runtime"][0].tobytes() and out["builtin"][1].tobytes() == out["runtime"][1].tobytes()
print(f"smooth N={N} ntheta={nth} nsims={nsims} atol=1e-2, {reps} alternating repetitions; the two series computed the same bits")
for name, s in series.items():
    for what, v in s.items():
        v = np.array(v)
        print(f"{name:8s} {what:6s} ms: " + " ".join(f"{t:.3f}" for t in v) +
              f"   median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} spread {v.max() - v.min():.3f}")
kb, kr = np.array(series["builtin"]["kernel"]), np.array(series["runtime"]["kernel"])
print(f"runtime - builtin, kernel medians: {np.median(kr) - np.median(kb):+.3f} ms; the built-in's own spread: {kb.max() - kb.min():.3f} ms")
for p in probs.values():
    p.close()
