"""-m gpu: the map kernel's hand-over (csrc/kernels.hpp, the dynamic deal of map_score_kernel; DESIGN.md, "Between two solves")
three and more problems deep, in every placement, model and entry point that is an instantiation of its own.

The hand-over's safety argument -- the ticket word of one parity is rewritten only two problems later; the placements that reduce
inside begin() keep the reduction scratch's halves alternating across problems -- comes into play from a workgroup's THIRD problem
on.  Every deep launch here carries at least 16 problems per compute unit plus one: no non-cluster placement has more than four
workgroups per compute unit (muse_engine.cpp, place_wgs_per_cu), so the average chain is at least four problems long, some workgroup
takes five, and the one-per-compute-unit headline placement takes about sixteen.

Yardstick 1, exact: nothing between two solves computes anything, so a deep launch must return -- scores, whole solver records,
MAPs, Jacobians, CG counts, bit for bit -- what the same simulations return in launches of num_cus // 2 problems, where the grid
equals the problem count and every problem is its workgroup's first and only.  For one row per model the first 8 simulations are
also launched one per call, the reference of tests/test_gpu_map_handover.py.

Yardstick 2, the mathematics, on 12 elements of each deep map launch (the first, the last, around grid and 2 grid): the records
against the MAP written out (tests/test_gpu_highprec.py, check_records, at its own bounds) for the models of hp_reference.MODELS;
the two exponential models against the CPU checker over 8 consecutive simulations around the grid at the tolerances of
tests/test_gpu_model_exp.py; finite-difference Jacobians against the oracle at rtol 1e-8 and implicit-differentiation H against
hp_reference.implicit_H at rtol 1e-6, as the existing tests hold them.  No tolerance is new.

Every case asserts its depth on the problem count the engine launches and the placement that ran against the one its row names.
N stays below 65536 and no element split is set: the cluster placements draw no tickets."""
import collections

import numpy as np
import pytest

import hp_reference as R
from test_gpu_highprec import check_records
from test_gpu_map_handover import SEED, THETA, THETA2, _one_per_call
from test_gpu_model_exp import hess_inf_ln, hess_inf_sv
from test_gpu_parity import assert_same_path_or_close
from test_model_exp_models import LN, SV
from test_user_model import CUBIC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.HAVE_LD, reason=R.SKIP_REASON)]

ATOL, COLD_ATOL, WARM_ATOL = 1e-4, 1e-2, 1e-6      # (cold and warm: those of test_gpu_map_handover's warm start)
NO_SPECULATION = 1 << 5                             # debug bit 5: the speculating trial off (solver.hpp, eval SPEC)
BUILTIN = ("funnel", "noise", "smooth")
EXPONENTIAL = {"stochastic_volatility": (SV, hess_inf_sv), "lognormal_obs": (LN, hess_inf_ln)}


def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def depth():
    """The least problem count of a deep launch."""
    return 16 * num_cus() + 1


def chunk():
    """The problem count of a reference launch: below every placement's grid, so each problem is its workgroup's first."""
    return max(1, num_cus() // 2)


def grid_of(ran, N, nproblems, implicit=False):
    """The grid a launch of `nproblems` gets (muse_engine.cpp, launch_batch and place_wgs_per_cu): four workgroups per compute unit
    for the 256-thread placements, one for PlaceResident<512, 10> (resident, N > 4096), two otherwise; the implicit-differentiation
    batches always run PlaceStreaming<512>."""
    if implicit:
        per_cu = 2
    else:
        per_cu = 4 if ran["threads"] == 256 else (1 if ran["resident"] and N > 4096 else 2)
    return min(nproblems, num_cus() * per_cu)


def same_bits(a, b, what, ctx):
    """array_equal, and on failure the first differing indices."""
    assert a.shape == b.shape, (ctx, what, a.shape, b.shape)
    assert np.array_equal(a, b), (ctx, what, "first differing indices", np.argwhere(a != b)[:10].tolist())


def spread(n, grid):
    """12 elements of a launch of n problems: the first two, the last, three around grid and around 2 grid, three in between."""
    picks = [0, 1, n - 1, grid - 1, grid, grid + 1, 2 * grid - 1, 2 * grid, 2 * grid + 1, n // 3, (5 * n) // 8, (7 * n) // 8]
    out = sorted({e for e in picks if 0 <= e < n})
    e = n - 2
    while len(out) < min(12, n):       # (collisions on another card's grid: fill from the end)
        if e not in out:
            out.append(e)
        e -= 1
    return sorted(out)


# ---- the rows ---------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "id model N theta placement resident threads start flags tie")


def _row(id, model, N, theta, placement=-1, resident=True, threads=512, start="zero", flags=0, tie=False):
    return Row(id, model, N, tuple(theta), placement, resident, threads, start, flags, tie)


FUNNEL4 = [0.6, -0.3, 1.0, 0.2]
MAP_ROWS = [
    # 1. PlaceResident<512, 10, true>, odd N (the pad element is live): the headline's kernel, x and g in LDS, no reduction in begin()
    _row("funnel-4097-zero", "funnel", 4097, THETA, tie=True),
    _row("funnel-4097-true", "funnel", 4097, THETA, start="true"),
    _row("funnel-4097-warm", "funnel", 4097, THETA, start="warm"),
    _row("funnel-4097-no-speculation", "funnel", 4097, THETA, flags=NO_SPECULATION),
    # 2. the shapes of test_gpu_map_handover.py, which reduce inside begin(): PlaceResident<512, 4> and <256, 1>
    _row("funnel-1001", "funnel", 1001, THETA),
    _row("funnel-64", "funnel", 64, THETA, threads=256),
    # 3. several components: the non-uniform line search of the resident kernel, PlaceStreaming<512> and <256> in the big tier
    _row("funnel4-4097-resident", "funnel", 4097, FUNNEL4),
    _row("funnel4-4097-streaming", "funnel", 4097, FUNNEL4, placement=0, resident=False),
    _row("funnel4-300-streaming", "funnel", 300, FUNNEL4, placement=0, resident=False, threads=256),
    _row("funnel9-1001-big-tier", "funnel", 1001, np.round(np.linspace(-1.0, 1.5, 9), 3), resident=False),
    # 4. noise
    _row("noise-513-resident", "noise", 513, [0.3], tie=True),
    _row("noise-513-streaming", "noise", 513, [0.3], placement=0, resident=False),
    # 5. the stencil model: it kept the two barriers and reads the parity word
    _row("smooth2-601", "smooth", 601, [1.0, 0.5], resident=False, tie=True),
    _row("smooth2-64", "smooth", 64, [1.0, 0.5], resident=False, threads=256),
    # 6. the packaged headers: libraries, and so compilations, of their own
    _row("cubic-4097", "cubic", 4097, [0.3], tie=True),
    _row("normal_mean_var-4097", "normal_mean_var", 4097, [0.3, -0.5], tie=True),
    _row("stochastic_volatility2-4097", "stochastic_volatility", 4097, [0.3, -0.5], tie=True),
    _row("stochastic_volatility4-4097-fenced", "stochastic_volatility", 4097, [0.2, -0.4, -0.3, 0.1], resident=False),
    _row("lognormal_obs-4097", "lognormal_obs", 4097, [-0.5], tie=True),
]
# The exponential models' long solves (the rule of test_gpu_model_exp.against_the_checker): its rows for these shapes and thetas
# say False and True; the four-parameter shape is in no row of it and takes the cubic test's rule, more than 20 oracle iterations.
LONG = {"stochastic_volatility2-4097": False, "lognormal_obs-4097": True, "stochastic_volatility4-4097-fenced": None}


def _model(M, name):
    return name if name in BUILTIN else M.ElementwiseModel.packaged(name)


def _make(M, row, xdata=None):
    """The row's problem; the placement that will run is the one the row names, and never a cluster's."""
    prob = M.HipMuseProblem(xdata, model=_model(M, row.model), ntheta=len(row.theta), N=None if xdata is not None else row.N)
    if row.placement >= 0:
        prob.set_placement(row.placement)
    if row.flags:
        prob.debug_flags(row.flags)
    ran = prob.placement_info()
    assert (ran["resident"], ran["threads"], ran["workgroups_per_element"]) == (row.resident, row.threads, 1), (row.id, ran)
    return prob, ran


def _solve_theta(row):
    return list(THETA2) if row.start == "warm" else list(row.theta)


def _launch(prob, M, row, s0, s1, include_data=False):
    """One launch over simulations [s0, s1) -- a warm start: the cold launch at the row's theta first, then the warm one at THETA2."""
    if row.start == "warm":
        prob.map_and_score_batch(SEED, s0, s1, list(row.theta), atol=COLD_ATOL, z0_mode=M.Z0_ZERO)
        g, info = prob.map_and_score_batch(SEED, s0, s1, list(THETA2), atol=WARM_ATOL, z0_mode=M.Z0_WARM)
    else:
        z0_mode = M.Z0_TRUE if row.start == "true" else M.Z0_ZERO
        g, info = prob.map_and_score_batch(SEED, s0, s1, list(row.theta), include_data=include_data, atol=ATOL, z0_mode=z0_mode)
    return g, info, prob.get_zhat(0, len(info))


def _chunked(M, row, sims):
    """Yardstick 1's reference: the same simulations in launches of num_cus // 2 problems."""
    prob, ran = _make(M, row)
    c = chunk()
    assert c <= grid_of(ran, row.N, c)
    parts = [_launch(prob, M, row, s0, min(s0 + c, sims)) for s0 in range(0, sims, c)]
    prob.close()
    out = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    for arr in out:
        arr.setflags(write=False)
    return out


_REF = {}


def _reference(M, row, sims, share=False):
    """(share: computed once, used by more than one test, never written to)"""
    if not share:
        return _chunked(M, row, sims)
    key = (row.id, sims)
    if key not in _REF:
        _REF[key] = _chunked(M, row, sims)
    return _REF[key]


def _tie_to_one_per_call(M, row, ref):
    """The chunked reference's first 8 simulations against one simulation per call, the reference of test_gpu_map_handover.py."""
    gr, ir, zr = ref
    if row.model == "funnel" and len(row.theta) == 1 and row.theta == tuple(THETA):
        g1, i1, z1 = _one_per_call(M, row.N, 8, M.Z0_ZERO, ATOL)
    else:
        prob, _ = _make(M, row)
        one = [_launch(prob, M, row, s, s + 1) for s in range(8)]
        prob.close()
        g1, i1, z1 = (np.concatenate([p[k] for p in one]) for k in range(3))
    same_bits(gr[:8], g1, "scores", (row.id, "one per call"))
    same_bits(ir[:8], i1, "records", (row.id, "one per call"))
    same_bits(zr[:8], z1, "MAPs", (row.id, "one per call"))


def _check_mathematics(M, O, row, prob, elements, sim_of, theta, atol, g, info, z, grid):
    """Yardstick 2 on `elements` of the launch (sim_of: element -> simulation)."""
    theta = np.asarray(theta, dtype=np.float64)
    if row.model in R.MODELS:
        xs = [prob.sample_x_z(M.SimRng(SEED, sim_of(e)), theta)[0] for e in elements]
        check_records(row.model, xs, theta, z[elements], g[elements], info[elements], atol, ctx=f"{row.id} elements {elements}")
        return
    # the exponential models: the CPU checker over 8 consecutive simulations around the grid, tolerances of against_the_checker
    header, hess_inf = EXPONENTIAL[row.model]
    e0 = max(0, min(grid - 4, len(info) - 8))
    s0 = sim_of(e0)
    with O.user_model(header, row.model):
        go, zo, io = O.map_and_score_batch("user", row.N, SEED, s0, s0 + 8, theta, atol=atol, z0_mode=0, nthreads=4)
    long = LONG[row.id] if LONG[row.id] is not None else int(io["iterations"].max()) > 20
    sl = slice(e0, e0 + 8)
    same = assert_same_path_or_close(info[sl], io, z[sl], zo, g[sl], go, atol, theta, "funnel", ctx=f"{row.id} sims {s0}..{s0 + 7}",
                                     hess_inf=hess_inf(theta, zo, atol), z_atol=1e-7 if long else 1e-9, g_rtol=1e-6 if long else 1e-10)
    assert same.all() if not long else same.mean() >= 0.8, (info["iterations"][sl], io["iterations"], info["f_calls"][sl], io["f_calls"])


# ---- rows 1 to 6: plain maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", MAP_ROWS, ids=[r.id for r in MAP_ROWS])
def test_deep_map_equals_first_problem_launches(gpu, M, O, row):
    sims = depth()
    ref = _reference(M, row, sims, share=row.id == "funnel-4097-zero")
    prob, ran = _make(M, row)
    g, info, z = _launch(prob, M, row, 0, sims)
    nproblems = len(info)
    grid = grid_of(ran, row.N, nproblems)
    assert nproblems >= 16 * num_cus() + 1 and nproblems - grid >= 3 * grid, (nproblems, grid)
    print(f"{row.id}: {ran} problems {nproblems} grid {grid} hand-overs {nproblems - grid}")
    assert info["iterations"].max() >= 1
    same_bits(g, ref[0], "scores", row.id)
    same_bits(info, ref[1], "records", row.id)
    same_bits(z, ref[2], "MAPs", row.id)
    _check_mathematics(M, O, row, prob, spread(nproblems, grid), lambda e: e, _solve_theta(row),
                       WARM_ATOL if row.start == "warm" else ATOL, g, info, z, grid)
    prob.close()
    if row.tie:
        _tie_to_one_per_call(M, row, ref)


# ---- row 7: the data element is problem 0 -------------------------------------------------------------------------------------
def test_deep_map_with_the_data_element(gpu, M, O):
    row = MAP_ROWS[0]
    sims = depth()
    ref = _reference(M, row, sims, share=True)
    draw = M.HipMuseProblem(None, model="funnel", ntheta=1, N=row.N)
    xdata = draw.sample_x_z(M.SimRng(SEED, M.DATA_SIM), list(row.theta))[0]
    draw.close()
    prob, ran = _make(M, row, xdata)
    g, info, z = _launch(prob, M, row, 0, sims, include_data=True)
    nproblems = len(info)
    grid = grid_of(ran, row.N, nproblems)
    assert nproblems == sims + 1 >= 16 * num_cus() + 1
    print(f"include_data: {ran} problems {nproblems} grid {grid} hand-overs {nproblems - grid}")
    g1, i1, z1 = _launch(prob, M, row, 0, 1, include_data=True)       # the data element's reference: data and one simulation
    same_bits(g[0], g1[0], "scores", "data element")
    same_bits(info[:1], i1[:1], "records", "data element")
    same_bits(z[0], z1[0], "MAPs", "data element")
    same_bits(g[1:], ref[0], "scores", "simulations beside the data")
    same_bits(info[1:], ref[1], "records", "simulations beside the data")
    same_bits(z[1:], ref[2], "MAPs", "simulations beside the data")
    elements = spread(nproblems, grid)
    theta = np.asarray(row.theta)
    xs = [xdata if e == 0 else prob.sample_x_z(M.SimRng(SEED, e - 1), theta)[0] for e in elements]
    check_records("funnel", xs, theta, z[elements], g[elements], info[elements], ATOL, ctx=f"include_data elements {elements}")
    prob.close()


# ---- row 8: several maps in one launch, and on two lanes ----------------------------------------------------------------------
MULTI = _row("funnel2-1001-multi", "funnel", 1001, [0.6, -0.3])
MULTI_THETAS = np.array([[0.6, -0.3], [0.65, 0.1], [-0.2, 0.9]])


def test_deep_multi_map_launch(gpu, M, O):
    n = -(-depth() // 3)
    refs = [_chunked(M, MULTI._replace(theta=tuple(th)), n) for th in MULTI_THETAS]
    gr, ir, zr = (np.concatenate([r[k] for r in refs]) for k in range(3))
    prob, ran = _make(M, MULTI)
    total = prob.map_and_score_multi_async(SEED, 0, n, MULTI_THETAS, atol=ATOL, z0_mode=M.Z0_ZERO)
    grid = grid_of(ran, MULTI.N, total)
    assert total == 3 * n >= 16 * num_cus() + 1
    print(f"multi-map: {ran} problems {total} grid {grid} hand-overs {total - grid}")
    g, info = prob.batch_wait(total, 0)
    z = prob.get_zhat(0, total)
    for m in range(3):         # element e of map m: row and slot m n + e (include/muse_hip.h)
        rows = slice(m * n, (m + 1) * n)
        same_bits(g[rows], gr[rows], "scores", ("map", m))
        same_bits(info[rows], ir[rows], "records", ("map", m))
        same_bits(z[rows], zr[rows], "MAPs", ("map", m))
    for e in spread(total, grid):
        th = MULTI_THETAS[e // n]
        x = prob.sample_x_z(M.SimRng(SEED, e % n), th)[0]
        check_records("funnel", [x], th, z[e:e + 1], g[e:e + 1], info[e:e + 1], ATOL, ctx=f"multi-map element {e}")
    prob.close()
    prob, _ = _make(M, MULTI)
    # two lanes: areas 0 and 2 on lane 0, area 1 on lane 1, all three enqueued before the first wait (the lanes' ticket counters
    # run on from launch to launch; muse_get_zhat reads lane 0's slots, compared after the lane's last launch)
    prob.set_concurrency(2)
    for area in (0, 1, 2):
        assert prob.map_and_score_multi_async(SEED, 0, n, MULTI_THETAS, atol=ATOL, z0_mode=M.Z0_ZERO, result_area=area) == total
    for area in (0, 1, 2):
        g, info = prob.batch_wait(total, result_area=area)
        same_bits(g, gr, "scores", ("area", area))
        same_bits(info, ir, "records", ("area", area))
    same_bits(prob.get_zhat(0, total), zr, "MAPs", "lane 0")
    prob.close()


# ---- row 9: finite-difference batches with the folded fiducial ----------------------------------------------------------------
FD_ROWS = [_row("fd-funnel-1001", "funnel", 1001, THETA), _row("fd-cubic-1001", "cubic", 1001, [0.4])]
FD_STEP = [0.05]


@pytest.mark.parametrize("row", FD_ROWS, ids=[r.id for r in FD_ROWS])
def test_deep_fd_batch_equals_chunked_calls(gpu, M, O, row):
    """2 ntheta nsims + 1 problems: the fiducial (wait_fiducial sits inside begin(), in front of the publishing barrier) and, per
    simulation and component, the problems at theta +- step.  The reference: the same call over chunks of at most num_cus // 4
    problems."""
    nth = len(row.theta)
    atol = COLD_ATOL if row.model == "funnel" else ATOL       # (those of the existing finite-difference tests of each model)
    nsims = -(-(depth() - 1) // (2 * nth))
    nproblems = 2 * nth * nsims + 1
    per_call = (num_cus() // 4 - 1) // (2 * nth)
    assert per_call >= 1 and 2 * nth * per_call + 1 <= num_cus() // 4
    prob, ran = _make(M, row)
    grid = grid_of(ran, row.N, nproblems)
    assert nproblems >= 16 * num_cus() + 1 and nproblems - grid >= 3 * grid, (nproblems, grid)
    print(f"{row.id}: {ran} problems {nproblems} grid {grid} hand-overs {nproblems - grid}")
    Hs, info = prob.fd_jacobian_batch(SEED, 0, nsims, list(row.theta), FD_STEP, atol=atol)
    parts = [prob.fd_jacobian_batch(SEED, s0, min(s0 + per_call, nsims), list(row.theta), FD_STEP, atol=atol)
             for s0 in range(0, nsims, per_call)]
    prob.close()
    same_bits(Hs, np.concatenate([p[0] for p in parts]), "Jacobians", row.id)
    same_bits(info, np.concatenate([p[1] for p in parts]), "records", row.id)
    checked = sorted({0, grid // (2 * nth), grid // nth, nsims - 1})         # (problems around grid and 2 grid among them)
    assert len(checked) == 4
    if row.model == "funnel":
        _, zfid, _ = O.map_and_score_batch("funnel", row.N, SEED, M.MASTER_SIM, M.MASTER_SIM + 1, list(row.theta), atol=atol, z0_mode=0)
        for s in checked:
            Ho = O.fd_jacobian("funnel", row.N, SEED, s, list(row.theta), FD_STEP, zfid[0], atol=atol)
            np.testing.assert_allclose(Hs[s], Ho, rtol=1e-8, atol=1e-8 * np.abs(Ho).max(), err_msg=f"sim {s}")
    else:
        with O.user_model(CUBIC, "cubic"):
            _, zfid, _ = O.map_and_score_batch("user", row.N, SEED, M.MASTER_SIM, M.MASTER_SIM + 1, list(row.theta), atol=atol, z0_mode=0)
            for s in checked:
                Ho = O.fd_jacobian("user", row.N, SEED, s, list(row.theta), FD_STEP, zfid[0], atol=atol)
                np.testing.assert_allclose(Hs[s], Ho, rtol=1e-8, atol=1e-9, err_msg=f"sim {s}")


# ---- row 10: the implicit-differentiation kernels -------------------------------------------------------------------------------
# (the placement asserted is the one of the problem's maps; an implicit batch runs PlaceStreaming<512> whatever N: grid_of)
IMPLICIT_ROWS = [
    (_row("implicit-funnel2-257", "funnel", 257, [0.4, -0.1], threads=256), None),                      # run_implicit
    (_row("implicit-funnel2-257-jacobi", "funnel", 257, [0.4, -0.1], threads=256), "jacobi"),           # run_implicit<JACOBI>
    (_row("implicit-stochastic_volatility2-257", "stochastic_volatility", 257, [0.3, -0.5], threads=256), None),   # run_implicit_pair
    (_row("implicit-smooth-65", "smooth", 65, [1.0], resident=False, threads=256), None),             # the stencil model's
]


@pytest.mark.parametrize("row,cg_Pl", IMPLICIT_ROWS, ids=[r.id for r, _ in IMPLICIT_ROWS])
def test_deep_implicit_batch_equals_chunked_calls(gpu, M, row, cg_Pl):
    nsims = depth()
    kw = dict(atol=1e-10, cg_maxiter=1000, cg_Pl=cg_Pl)
    prob, ran = _make(M, row)
    grid = grid_of(ran, row.N, nsims, implicit=True)
    assert nsims >= 16 * num_cus() + 1 and nsims - grid >= 3 * grid and chunk() <= grid, (nsims, grid)
    print(f"{row.id}: {ran} problems {nsims} grid {grid} hand-overs {nsims - grid}")
    Hs, its = prob.implicit_H_batch(SEED, 0, nsims, list(row.theta), **kw)
    parts = [prob.implicit_H_batch(SEED, s0, min(s0 + chunk(), nsims), list(row.theta), **kw) for s0 in range(0, nsims, chunk())]
    prob.close()
    assert its.max() >= 1
    same_bits(Hs, np.concatenate([p[0] for p in parts]), "H", row.id)
    same_bits(its, np.concatenate([p[1] for p in parts]), "CG counts", row.id)
    if row.model in R.MODELS:       # rtol 1e-6: CG's stopping rule (test_gpu_highprec.test_implicit_H_against_the_reference)
        for s in (0, grid, nsims - 1):
            Hh = R.implicit_H(row.model, row.N, SEED, s, list(row.theta)).astype(np.float64)
            np.testing.assert_allclose(Hs[s], Hh, rtol=1e-6, atol=1e-6 * np.abs(Hh).max(), err_msg=f"sim {s}")
