"""What an exponential per element costs a header model (include/muse_model.h, EXPONENTIALS; csrc/model_math.hpp).

  python tools/model_exp_bench.py              time one cold 512-simulation map at N = 10^4 (atol 1e-4, from zero), the variants
                                               alternating in ONE process, three rounds; prints the placement that ran and the
                                               median kernel time of each:
                                                   stochastic_volatility        the device exponential (muse::model_exp)
                                                   stochastic_volatility_plainexp   the same header with muse::muse_exp inlined
                                                                                (-DMUSE_MODEL_EXP_PLAIN: the branchy sequence)
                                                   normal_mean_var              its sibling without an exponential (K = 1)
                                               and lognormal_obs / lognormal_obs_plainexp / cubic likewise (one parameter).
  python tools/model_exp_bench.py --resources  the kernels' registers / spills / scratch of those libraries (tools/regs.py
                                               --library rows), as recorded in profiles/r18_model_exp_resources.txt

The iteration counts of the variants differ (they are different models; the two builds of one header take the same path): the
figure per iteration is printed beside the total."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [  # (label, header, library name, build switches, ntheta, theta)
    ("stochastic_volatility", "stochastic_volatility", "stochastic_volatility", (), 2, [0.3, -0.5]),
    ("stochastic_volatility_plainexp", "stochastic_volatility", "stochastic_volatility_plainexp", ("-DMUSE_MODEL_EXP_PLAIN",), 2, [0.3, -0.5]),
    ("normal_mean_var", "normal_mean_var", "normal_mean_var", (), 2, [0.3, -0.5]),
    ("lognormal_obs", "lognormal_obs", "lognormal_obs", (), 1, [-0.5]),
    ("lognormal_obs_plainexp", "lognormal_obs", "lognormal_obs_plainexp", ("-DMUSE_MODEL_EXP_PLAIN",), 1, [-0.5]),
    ("cubic", "cubic", "cubic", (), 1, [-0.5]),
]


def libraries():
    from museinference_jl_amd import build as b
    return {label: b.build_model_library(os.path.join(b.MODELS_DIR, header + ".h"), lib, defines=defs) for label, header, lib, defs, _, _ in VARIANTS}


def resources():
    spec = importlib.util.spec_from_file_location("regs", os.path.join(ROOT, "tools", "regs.py"))
    regs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(regs)
    for label, path in libraries().items():
        print(f"== {label}")
        for short, vgpr, vspill, sspill, scratch, dyn in sorted(regs.library_report(path), key=lambda r: (-r[4], r[0])):
            print(f"{short:78s} vgpr {vgpr:3d} vspill {vspill:3d} sspill {sspill:3d} scratch {scratch:4d}{' CALLS' if dyn else ''}")
        print(f"{len(regs.check_library(path))} kernels beyond {regs.LIBRARY_SCRATCH_LIMIT} bytes of scratch or with calls")


def bench(N=10000, nsims=512, rounds=3):
    import numpy as np
    import museinference_jl_amd as M
    libs = libraries()
    probs = {}
    for label, header, lib, defs, nth, theta in VARIANTS:
        model = M.ElementwiseModel.packaged(header).use_library(libs[label])      # (the comparison build of the same header)
        p = M.HipMuseProblem(None, model=model, ntheta=nth, N=N)
        p.set_timing(True)
        p.set_normals_cache(False)
        probs[label] = (p, theta)
    times = {label: [] for label in probs}
    its = {}
    for r in range(rounds + 1):                           # (round 0 warms every library up)
        for label, (p, theta) in probs.items():
            _, info = p.map_and_score_batch(42, 0, nsims, theta, atol=1e-4, z0_mode=0)
            if r:
                times[label].append(p.last_kernel_ms())
            its[label] = (int(info["iterations"].min()), float(info["iterations"].mean()), int(info["iterations"].max()), int(info["f_calls"].sum()))
    print(f"one cold map, N = {N}, {nsims} simulations, atol 1e-4, from zero; kernel time, median of {rounds} alternating rounds")
    for label, (p, _) in probs.items():
        ms = float(np.median(times[label]))
        lo, mean, hi, fc = its[label]
        pi = p.placement_info()
        place = f"{'resident' if pi['resident'] else 'streaming'} x{pi['threads']}"
        print(f"{label:32s} {ms:8.3f} ms   iterations {lo}-{hi} (mean {mean:.1f}), {fc} evaluations   {1e3 * ms / mean:7.1f} us per mean iteration   "
              f"{place}   all rounds {['%.3f' % t for t in times[label]]}")
        p.close()


if __name__ == "__main__":
    if "--resources" in sys.argv:
        resources()
    else:
        bench()
