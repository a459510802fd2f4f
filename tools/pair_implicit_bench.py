"""get_H! of a two-parameter model by implicit differentiation against finite differences, on the same build:
`python tools/pair_implicit_bench.py implicit|fd [N] [ntheta] [nsims]` prints the wall time of one implicit_H_batch /
fd_jacobian_batch call on models/offset_noise.h after a warm-up call (libraries loaded, buffers allocated, normals cache warm).
Run each mode under `rocprofv3 --kernel-trace --stats -- python ...` for the kernel times (profiles/r07_pair_implicit_vs_fd.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import museinference_jl_amd as M

mode = sys.argv[1]
N, nth, nsims = (int(v) for v in (sys.argv[2:5] + ["10000", "4", "512"][len(sys.argv) - 2:]))
theta = np.concatenate([np.linspace(-0.2, 0.3, nth // 2), np.linspace(0.4, -0.3, nth // 2)])
prob = M.HipMuseProblem(None, model=M.ElementwiseModel.packaged("offset_noise"), ntheta=nth, N=N)
call = ((lambda: prob.implicit_H_batch(7, 0, nsims, theta, atol=1e-1)) if mode == "implicit" else
        (lambda: prob.fd_jacobian_batch(7, 0, nsims, theta, np.full(nth, 0.05), atol=1e-2)))
call()
times = []
for _ in range(5):
    t0 = time.perf_counter()
    H = call()[0]
    times.append(time.perf_counter() - t0)
print(f"{mode}: N={N} ntheta={nth} nsims={nsims}  wall ms per call: " + " ".join(f"{1e3 * t:.3f}" for t in times) +
      f"   mean H diagonal {np.mean(H, axis=0).diagonal()}")
prob.close()
