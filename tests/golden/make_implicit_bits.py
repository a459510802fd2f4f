#!/usr/bin/env python3
"""Records tests/golden/implicit_bits.npz on a GPU: the implicit-differentiation get_H! of every branch of the solver's implicit
section, as raw float64 H and the returned CG iteration counts, for the case list below -- what tests/test_gpu_implicit_bits.py
holds a change of that section to, bit for bit.  The values are the engine's own at the commit that recorded them (they pin a
refactor; the checks against the longdouble references are tests/test_gpu_implicit_jacobi.py, test_pair_implicit.py,
test_gpu_noise_weights.py, test_gpu_response.py), so the file is recorded BEFORE the code changes and not again with it.

Shapes: N = 1001 (odd: the pad element is live, a block boundary falls inside a wave), N = 65536 (the smallest cluster), N = 4096
with 9 components (the smallest big-tier launch).  Default keywords unless a case says otherwise; each case keeps its first three
simulations.  Needs the libraries build() compiles.  Run from the repository root:
    python tests/golden/make_implicit_bits.py [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "implicit_bits.npz")
SEED, KEEP = 17, 3
FUNNEL3 = [0.3, -0.5, 1.0]
FUNNEL8 = [0.3, -0.5, 1.0, 0.2, -0.1, 0.4, 0.0, -0.3]
JACOBI = (("default", {}), ("jacobi", dict(cg_Pl="jacobi")))


def _cases():
    """[(key, dict)]: model, N, theta (None: the module's theta_of), nsims, entry ("batch" / "columns"), cluster, variant, kw."""
    out = []

    def add(key, **c):
        c.setdefault("nsims", 3)
        c.setdefault("entry", "batch")
        c.setdefault("cluster", False)
        c.setdefault("variant", None)
        c.setdefault("kw", {})
        out.append((key, c))

    for how, kw in JACOBI:
        add(f"funnel_1001x3_{how}", model="funnel", N=1001, theta=FUNNEL3, kw=kw)                   # one column per workgroup
        add(f"funnel_1001x3_300sims_{how}", model="funnel", N=1001, theta=FUNNEL3, nsims=300, kw=kw)   # all columns in one workgroup
        add(f"funnel_1001x3_columns_{how}", model="funnel", N=1001, theta=FUNNEL3, entry="columns", kw=kw)
        add(f"funnel_65536x2_{how}", model="funnel", N=65536, theta=[0.3, -0.5], cluster=True, kw=kw)
        add(f"noise_1001_{how}", model="noise", N=1001, theta=[-0.2], kw=kw)
        add(f"noise_65536_{how}", model="noise", N=65536, theta=[0.4], cluster=True, kw=kw)
        add(f"cubic_1001x2_{how}", model="cubic", N=1001, theta=[0.5, -0.3], kw=kw)
        add(f"cubic_65536x1_{how}", model="cubic", N=65536, theta=[0.5], cluster=True, kw=kw)
        pair = dict(kw, cg_reltol=1e-3, H1_is_zero=True)
        add(f"offset_noise_1001x4_{how}", model="offset_noise", N=1001, theta=None, kw=pair)
        add(f"offset_noise_65536x4_{how}", model="offset_noise", N=65536, theta=None, cluster=True, kw=pair)
    add("funnel_1001x8_2sims", model="funnel", N=1001, theta=FUNNEL8, nsims=2)
    add("funnel_4096x9", model="funnel", N=4096, theta=FUNNEL8 + [0.6])                              # the big tier
    for variant in ("built", "stencil", "noise"):
        add(f"smooth_1001x3_{variant}", model="smooth", N=1001, nth=3, theta=None, variant=variant)
        add(f"smooth_65536x2_{variant}", model="smooth", N=65536, nth=2, theta=None, cluster=True, variant=variant)
    add("smooth_4096x9_noise", model="smooth", N=4096, nth=9, theta=None, variant="noise")
    for N, nth, cluster in ((1001, 3, False), (65536, 2, True), (4096, 9, False)):
        for how, kw in (("default", {}), ("reltol", dict(cg_reltol=1e-3)), ("maxiter1", dict(cg_maxiter=1))):
            add(f"saturating_{N}x{nth}_{how}", model="saturating_response", N=N, nth=nth, theta=None, cluster=cluster, variant="noise", kw=kw)
    return out


CASES = _cases()


def run_case(M, c):
    """(H [<= 3, ntheta, ntheta] float64, iteration counts [<= 3, ntheta] int32) of one case."""
    import response_cases as RC
    from test_gpu_noise_weights import noise_of, theta_of as stencil_theta
    from test_pair_implicit import theta_of as pair_theta
    model, N = c["model"], c["N"]
    if model == "offset_noise":
        theta = pair_theta(model, 4)
    elif c["theta"] is None:
        theta = stencil_theta(c["nth"])
    else:
        theta = np.asarray(c["theta"], dtype=np.float64)
    nth = theta.size
    if model in ("cubic", "offset_noise"):
        m = M.ElementwiseModel.packaged(model)
    elif model == "saturating_response":
        m = M.ResponseModel.packaged(model)
    else:
        m = model
    prob = M.HipMuseProblem(None, model=m, ntheta=nth, N=N)
    info = prob.placement_info()
    assert (info["workgroups_per_element"] > 1) == c["cluster"], info
    if c["variant"] == "stencil":
        prob.set_stencil((0.6, 0.2))
    if c["variant"] == "noise":
        sd, mask, _ = noise_of(N, nth, info["threads"], info["workgroups_per_element"])
        prob.set_noise(sd, mask)
    if model == "saturating_response":
        prob.set_link(RC.SAT)
    nsims = c["nsims"]
    if c["entry"] == "columns":
        cols, ic = prob.implicit_H_columns(SEED, 0, 0, nsims * nth, theta, **c["kw"])
        H, its = cols.reshape(nsims, nth, nth).transpose(0, 2, 1), ic.reshape(nsims, nth)
    else:
        H, its = prob.implicit_H_batch(SEED, 0, nsims, theta, **c["kw"])
    prob.close()
    return np.ascontiguousarray(H[:KEEP], dtype=np.float64), np.ascontiguousarray(its[:KEEP], dtype=np.int32)


if __name__ == "__main__":
    import museinference_jl_amd as M
    out = {}
    for key, c in CASES:
        H, its = run_case(M, c)
        assert np.all(np.isfinite(H)), key
        print(key, "CG iterations", its.tolist())
        out[key + "_H"], out[key + "_it"] = H, its
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(CASES), "cases")
