"""The stencil model's link kernels against its run-time-noise kernels on BASELINE.json's configs[4] share (smooth, N = 10^5,
8 theta, 128 sims, atol 1e-2 from zero): `python tools/link_bench.py [reps] [nsims]` alternates one map of a context at
set_noise(ones) (the noise kernels: byte for byte the parent commit's, tools/code_hash.py) with one of a context at
set_noise(ones) and set_link((0, 0)) (the same bits, the same solves, from the kernels that also evaluate phi and phi': the
difference is the link's arithmetic alone), `reps` times after a warm-up of each, and prints both series -- kernel ms from the
launch's own event pair, and wall ms -- with their spread (profiles/r11_link.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import museinference_jl_amd as M

reps, nsims = (int(v) for v in (sys.argv[1:3] + ["7", "128"][len(sys.argv) - 1:]))
N, nth = 100000, 8
theta = [1.0] * nth
probs = {"noise": M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, noise_sd=np.ones(N)),
         "link": M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, noise_sd=np.ones(N), link=(0.0, 0.0))}
assert probs["link"].get_link()[1] and not probs["noise"].get_link()[1]
series = {k: {"kernel": [], "wall": []} for k in probs}
out = {}
for p in probs.values():
    p.set_timing(True)
    p.set_normals_cache(False)      # every map draws its simulations: the whole kernel, as bench.py's plain run times it
    p.map_and_score_batch(0, 0, nsims, theta, atol=1e-2)
for r in range(reps):
    for name in (("noise", "link") if r % 2 == 0 else ("link", "noise")):
        p = probs[name]
        p.synchronize()
        t0 = time.perf_counter()
        out[name] = p.map_and_score_batch(0, 0, nsims, theta, atol=1e-2)
        series[name]["wall"].append(1e3 * (time.perf_counter() - t0))
        series[name]["kernel"].append(p.last_kernel_ms())
assert out["noise"][0].tobytes() == out["link"][0].tobytes() and out["noise"][1].tobytes() == out["link"][1].tobytes()
print(f"smooth N={N} ntheta={nth} nsims={nsims} atol=1e-2, {reps} alternating repetitions; the two series computed the same bits")
for name, s in series.items():
    for what, v in s.items():
        v = np.array(v)
        print(f"{name:8s} {what:6s} ms: " + " ".join(f"{t:.3f}" for t in v) +
              f"   median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} spread {v.max() - v.min():.3f}")
kn, kl = np.array(series["noise"]["kernel"]), np.array(series["link"]["kernel"])
print(f"link - noise, kernel medians: {np.median(kl) - np.median(kn):+.3f} ms ({100 * (np.median(kl) / np.median(kn) - 1):+.1f} %); "
      f"the noise kernels' own spread: {kn.max() - kn.min():.3f} ms")
print(f"iterations per problem (mean): {out['link'][1]['iterations'].mean():.2f}, objective evaluations: {out['link'][1]['f_calls'].mean():.2f}")
for p in probs.values():
    p.close()
