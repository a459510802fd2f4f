"""The HagerZhang machine's branches in the two placements that keep the solve in LDS / registers, at their smallest sizes.

tests/test_gpu_linesearch.py runs the non-quadratic user model (tests/models/quartic.h) at N = 10^4; here it runs at
N = 4097 -- the lowest N of the LDS-resident placement (PlaceResident<512, 10, true>), odd, so that the pad slot behind the
vector is live -- and at N = 513, the lowest N of the all-register placement (PlaceResident<512, 4, false>).  In both the
line search's control flow is scalar: bracket expansion, bisection, the secant^2 updates and the
interval-shrink test are branches of the scalar unit there, and these problems take them -- against the oracle's solver:
equal iteration and evaluation counts and status on at least nine of the twelve cases, MAPs to 1e-9 and minima to 1e-12
where the paths agree, the same MAP within the solve's accuracy where a count differs (tree-ordered against sequential
sums).

And the built-in funnel at N = 4097 from a cold start: the resident placement and the streaming one reduce in the same
order (muse_engine.cpp, choose_place), so scores, solver records and MAPs are the same bits."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
QUARTIC = os.path.join(HERE, "models", "quartic.h")


@pytest.mark.parametrize("N", [4097, 513])
def test_line_search_branches_in_the_resident_placements(gpu, M, O, N):
    prob = M.HipMuseProblem(None, model=M.ElementwiseModel("quartic", QUARTIC), ntheta=1, N=N)
    pi = prob.placement_info()
    assert pi["resident"] and pi["threads"] == 512 and pi["workgroups_per_element"] == 1, pi
    rng = np.random.default_rng(11)
    same_path, n = 0, 0
    iters, evals, report = [], [], []
    with O.user_model(QUARTIC, "quartic"):
        for theta in (-2.0, 0.0, 1.5):
            for scale, start in ((3.0, "zero"), (1.0, "far")):
                for atol in (1e-2, 1e-7):
                    x = rng.standard_normal(N) * scale
                    z0 = np.zeros(N) if start == "zero" else 4.0 * rng.standard_normal(N)
                    z, info = prob.zhat_at_theta(x, z0, [theta], atol)
                    it, fc, status = info["iterations"], info["f_calls"], info["status"]
                    zo, io = O.zhat_at_theta("user", x, z0, [theta], atol)
                    report.append((n, theta, atol, (it, fc, status), (io["iterations"], io["f_calls"], io["status"])))
                    n += 1
                    # converged one way or another on both sides (0: gradient, 1: zero step, 2: objective unchanged twice)
                    assert status in (0, 1, 2) and io["status"] in (0, 1, 2), report[-1]
                    iters.append(io["iterations"])
                    evals.append(io["f_calls"])
                    if (it, fc, status) == (io["iterations"], io["f_calls"], io["status"]):
                        same_path += 1
                        np.testing.assert_allclose(z, zo, rtol=0, atol=1e-9, err_msg=f"N={N} case {n}")
                        np.testing.assert_allclose(info["f_min"], io["f_min"], rtol=1e-12)
                    else:   # the strictly convex objective has one MAP: both ended within the solve's accuracy of it
                        assert abs(it - io["iterations"]) <= (3 if status == io["status"] else 8), report[-1]
                        assert np.abs(z - zo).max() <= max(2 * atol, 1e-6), report[-1]
                    if status == 0:
                        assert info["gnorm"] <= atol
    prob.close()
    print(N, report)
    # real line-search work on the oracle's side (what the kernel is held to): several iterations in every case, and more
    # evaluations than the initial one plus two per line search -- the route of a quadratic (first trial, one secant step)
    assert n == 12 and min(iters) >= 3
    assert sum(evals) > 12 + 2 * sum(iters), (evals, iters)
    assert same_path >= n - 3, (N, same_path, report)


def test_funnel_cold_start_resident_and_streaming_give_the_same_bits(gpu, M):
    N, nsims, theta = 4097, 8, [1.0]
    prob = M.HipMuseProblem(None, model="funnel", ntheta=1, N=N)
    assert prob.placement_info()["resident"]
    g_r, i_r = prob.map_and_score_batch(0, 0, nsims, theta, atol=1e-2, z0_mode=M.Z0_ZERO)
    z_r = prob.get_zhat(0, nsims)
    prob.set_placement(0)
    assert not prob.placement_info()["resident"]
    g_s, i_s = prob.map_and_score_batch(0, 0, nsims, theta, atol=1e-2, z0_mode=M.Z0_ZERO)
    z_s = prob.get_zhat(0, nsims)
    prob.close()
    assert np.isfinite(g_r).all() and (i_r["iterations"] >= 1).all()
    assert g_r.tobytes() == g_s.tobytes()
    assert i_r.tobytes() == i_s.tobytes(), (i_r, i_s)
    assert z_r.tobytes() == z_s.tobytes()
