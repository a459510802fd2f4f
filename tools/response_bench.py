"""The response header family on BASELINE.json's configs[4] share (N = 10^5, 8 theta, 128 sims): `python tools/response_bench.py
[reps] [nsims]` takes two measurements, each `reps` alternating repetitions after a warm-up of every context, kernel ms from the
launch's own event pair (profiles/r12_response.txt).

(a) The built-in link kernels (a "smooth" context with set_link, byte for byte the parent commit's: tools/code_hash.py) against
    models/poly_response.h at the same coefficients: one map each, atol 1e-2 from zero.  The two compute the same bits and take
    the same solves (asserted); the arithmetic is identical, so the expectation is a median inside the built-in series' own spread.
(b) models/saturating_response.h: get_H! for the same simulations by implicit differentiation (implicit_H_batch: one MAP and
    ntheta CG solves per simulation) against finite differences (fd_jacobian_batch: 2 ntheta + 1 MAPs), both at the same MAP
    tolerance, wall ms per call (several launches each)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import museinference_jl_amd as M

reps, nsims = (int(v) for v in (sys.argv[1:3] + ["7", "128"][len(sys.argv) - 1:]))
N, nth = 100000, 8
theta = [1.0] * nth
link = (0.05, 0.02)          # monotone (a2^2 < 3 a3); at theta = 1 phi' between ~0.9 and ~1.6 over the draws


def spread(name, what, v):
    v = np.array(v)
    print(f"{name:20s} {what:6s} ms: " + " ".join(f"{t:.3f}" for t in v) +
          f"   median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} spread {v.max() - v.min():.3f}")
    return v


# ---- (a)
probs = {"builtin link": M.HipMuseProblem(None, model="smooth", ntheta=nth, N=N, noise_sd=np.ones(N), link=link),
         "poly_response": M.HipMuseProblem(None, model=M.ResponseModel.packaged("poly_response"), ntheta=nth, N=N, noise_sd=np.ones(N), link=link)}
series = {k: {"kernel": [], "wall": []} for k in probs}
out = {}
for p in probs.values():
    assert p.get_link() == (link, True)
    p.set_timing(True)
    p.set_normals_cache(False)      # every map draws its simulations: the whole kernel, as bench.py's plain run times it
    p.map_and_score_batch(0, 0, nsims, theta, atol=1e-2)
names = list(probs)
for r in range(reps):
    for name in (names if r % 2 == 0 else names[::-1]):
        p = probs[name]
        p.synchronize()
        t0 = time.perf_counter()
        out[name] = p.map_and_score_batch(0, 0, nsims, theta, atol=1e-2)
        series[name]["wall"].append(1e3 * (time.perf_counter() - t0))
        series[name]["kernel"].append(p.last_kernel_ms())
assert out[names[0]][0].tobytes() == out[names[1]][0].tobytes() and out[names[0]][1].tobytes() == out[names[1]][1].tobytes()
print(f"(a) N={N} ntheta={nth} nsims={nsims} atol=1e-2 link={link}, {reps} alternating repetitions; the two series computed the same bits "
      f"and took the same solves")
v = {name: {what: spread(name, what, s[what]) for what in s} for name, s in series.items()}
kb, kp = v[names[0]]["kernel"], v[names[1]]["kernel"]
print(f"poly_response - builtin link, kernel medians: {np.median(kp) - np.median(kb):+.3f} ms ({100 * (np.median(kp) / np.median(kb) - 1):+.1f} %); "
      f"the built-in series' own spread: {kb.max() - kb.min():.3f} ms -> {'inside' if abs(np.median(kp) - np.median(kb)) <= kb.max() - kb.min() else 'OUTSIDE'}")
print(f"iterations per problem (mean): {out[names[1]][1]['iterations'].mean():.2f}, objective evaluations: {out[names[1]][1]['f_calls'].mean():.2f}")
for p in probs.values():
    p.close()

# ---- (b)
p0, atol = 0.35, 1e-1       # (get_H!'s fiducial MAP tolerance, src/muse.jl:344)
prob = M.HipMuseProblem(None, model=M.ResponseModel.packaged("saturating_response"), ntheta=nth, N=N, noise_sd=np.ones(N), link=(p0, 0.0))
step = 0.1 * np.ones(nth)
calls = {"implicit_H_batch": lambda: prob.implicit_H_batch(0, 0, nsims, theta, atol=atol),
         "fd_jacobian_batch": lambda: prob.fd_jacobian_batch(0, 0, nsims, theta, step, atol=atol)}
res, wall = {}, {k: [] for k in calls}
for c in calls.values():
    c()
names = list(calls)
for r in range(reps):
    for name in (names if r % 2 == 0 else names[::-1]):
        prob.synchronize()
        t0 = time.perf_counter()
        res[name] = calls[name]()
        wall[name].append(1e3 * (time.perf_counter() - t0))
its = res["implicit_H_batch"][1]
assert np.all(its > 0), "a column stopped on an indefinite Hessian"
print(f"(b) saturating_response p0={p0} N={N} ntheta={nth} nsims={nsims} atol={atol}, {reps} alternating repetitions; CG iterations per column "
      f"{int(its.min())} .. {int(its.max())} (mean {its.mean():.1f})")
w = {name: spread(name, "wall", wall[name]) for name in names}
print(f"fd / implicit, wall medians per call: {np.median(w['fd_jacobian_batch']) / np.median(w['implicit_H_batch']):.2f}x")
Hi, Hf = res["implicit_H_batch"][0].mean(axis=0), res["fd_jacobian_batch"][0].mean(axis=0)
print("mean H, implicit diag:", np.round(np.diag(Hi), 3).tolist(), " finite differences diag:", np.round(np.diag(Hf), 3).tolist())
prob.close()
