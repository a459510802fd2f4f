"""-m gpu: the map kernel outside its solves -- the workgroup's prologue, the hand-over from one problem to the next, and the
pick-up of the starting point (csrc/kernels.hpp, map_score_kernel's dynamic deal; csrc/solver.hpp, begin).

None of the three computes anything, so the yardstick is equality: a launch in which workgroups take several problems must
return, bit for bit, what the same simulations return launched ONE PER CALL, where no workgroup hands over and every problem is
its workgroup's first.  Beside that every case is held to the CPU oracle at the tolerances of tests/test_gpu_parity.py (scores
rtol 1e-10, MAPs atol 1e-9, equal iteration and evaluation counts; a finite-difference Jacobian, which the engine returns instead
of the scores it is formed from, at that file's rtol 1e-8 of its largest entry).

Built-in funnel, one component, the resident placements: N = 1001 is odd (the pad element is live) and N = 64 sits in the
smallest tier."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 29
THETA = [0.6]
THETA2 = [0.65]          # a warm restart's theta
STEP = [0.05]


def _new(M, N):
    return M.HipMuseProblem(None, model="funnel", ntheta=1, N=N)


def _one_per_call(M, N, sims, z0_mode, atol):
    """Scores, infos and MAPs of `sims` simulations, every one in a launch of its own (one problem, one workgroup, slot 0).
    Z0_WARM: a cold call at THETA, then the warm one at THETA2, per simulation."""
    prob = _new(M, N)
    g, info, z = [], [], []
    for s in range(sims):
        if z0_mode == M.Z0_WARM:
            prob.map_and_score_batch(SEED, s, s + 1, THETA, atol=1e-2, z0_mode=M.Z0_ZERO)
            gs, i = prob.map_and_score_batch(SEED, s, s + 1, THETA2, atol=atol, z0_mode=M.Z0_WARM)
        else:
            gs, i = prob.map_and_score_batch(SEED, s, s + 1, THETA, atol=atol, z0_mode=z0_mode)
        g.append(gs[0].copy())
        info.append(i[0].copy())
        z.append(prob.get_zhat(0, 1)[0])
    prob.close()
    return np.array(g), np.array(info), np.array(z)


_REF = {}


def _reference(M, N, sims, z0_mode, atol):
    """(computed once per shape and start, shared, never written to)"""
    key = (N, sims, z0_mode, atol)
    if key not in _REF:
        _REF[key] = _one_per_call(M, N, sims, z0_mode, atol)
        for arr in _REF[key]:
            arr.setflags(write=False)
    return _REF[key]


def _assert_oracle(O, N, s0, s1, theta, atol, z0_mode, g, info, z, zhat0=None):
    go, zo, io = O.map_and_score_batch("funnel", N, SEED, s0, s1, theta, atol=atol, z0_mode=z0_mode, zhat=zhat0, nthreads=4)
    assert np.array_equal(info["status"], io["status"])
    assert np.array_equal(info["iterations"], io["iterations"]), (info["iterations"], io["iterations"])
    assert np.array_equal(info["f_calls"], io["f_calls"]), (info["f_calls"], io["f_calls"])
    np.testing.assert_allclose(g, go, rtol=1e-10)
    np.testing.assert_allclose(z, zo, rtol=0, atol=1e-9)
    return zo


# ---- the hand-over ---------------------------------------------------------------------------------------------------------
HAND_N, HAND_SIMS, HAND_ATOL = 1001, 600, 1e-3


def test_handover_equals_one_problem_per_launch(gpu, M):
    """600 problems on a grid of two workgroups per compute unit (PlaceResident<512, 4>): on a card of 256 compute units 512
    workgroups take their first problem and 88 tickets are handed over, so some workgroups take a second problem and none needs
    a third -- the chains of three and more are tests/test_gpu_handover_matrix.py's.  Every problem must equal the same
    simulation solved in a launch of its own."""
    gr, ir, zr = _reference(M, HAND_N, HAND_SIMS, M.Z0_ZERO, HAND_ATOL)
    prob = _new(M, HAND_N)
    g, info = prob.map_and_score_batch(SEED, 0, HAND_SIMS, THETA, atol=HAND_ATOL, z0_mode=M.Z0_ZERO)
    z = prob.get_zhat(0, HAND_SIMS)
    prob.close()
    assert info["iterations"].max() >= 1
    assert np.array_equal(g, gr), np.argwhere(g != gr)[:10]
    assert np.array_equal(info, ir), np.argwhere(info != ir)[:10]
    assert np.array_equal(z, zr), np.argwhere(z != zr)[:10]


def test_handover_word_and_ticket_base_carry_across_launches(gpu, M):
    """The same launch three times on two lanes, the result areas cycling (areas 0 and 2 on lane 0, area 1 on lane 1, all three
    enqueued before the first wait): a lane's ticket counter runs on from launch to launch and the kernel's ticket words start
    every launch afresh.  (muse_get_zhat reads lane 0's slots: the MAPs are compared after the lane's last launch.)"""
    gr, ir, zr = _reference(M, HAND_N, HAND_SIMS, M.Z0_ZERO, HAND_ATOL)
    prob = _new(M, HAND_N)
    prob.set_concurrency(2)
    for cycle in range(2):
        for area in (0, 1, 2):
            assert prob.map_and_score_batch_async(SEED, 0, HAND_SIMS, THETA, atol=HAND_ATOL, z0_mode=M.Z0_ZERO, result_area=area) == HAND_SIMS
        for area in (0, 1, 2):
            g, info = prob.batch_wait(HAND_SIMS, result_area=area)
            assert np.array_equal(g, gr), (cycle, area, np.argwhere(g != gr)[:10])
            assert np.array_equal(info, ir), (cycle, area, np.argwhere(info != ir)[:10])
        z = prob.get_zhat(0, HAND_SIMS)
        assert np.array_equal(z, zr), (cycle, np.argwhere(z != zr)[:10])
    prob.close()


# ---- the start's pick-up ----------------------------------------------------------------------------------------------------
PICK_SIMS = 40


@pytest.mark.parametrize("N", [1001, 64])
@pytest.mark.parametrize("start", ["zero", "true", "warm"])
def test_start_pickup(gpu, M, O, N, start):
    """Z0_ZERO, Z0_TRUE and Z0_WARM after a cold call: 40 simulations in one launch against one per call, and against the oracle."""
    z0_mode = {"zero": M.Z0_ZERO, "true": M.Z0_TRUE, "warm": M.Z0_WARM}[start]
    atol = 1e-6 if start == "warm" else 1e-2
    gr, ir, zr = _reference(M, N, PICK_SIMS, z0_mode, atol)
    prob = _new(M, N)
    zcold = None
    if start == "warm":
        gc, ic = prob.map_and_score_batch(SEED, 0, PICK_SIMS, THETA, atol=1e-2, z0_mode=M.Z0_ZERO)
        zcold = _assert_oracle(O, N, 0, PICK_SIMS, THETA, 1e-2, 0, gc, ic, prob.get_zhat(0, PICK_SIMS))
        g, info = prob.map_and_score_batch(SEED, 0, PICK_SIMS, THETA2, atol=atol, z0_mode=M.Z0_WARM)
    else:
        g, info = prob.map_and_score_batch(SEED, 0, PICK_SIMS, THETA, atol=atol, z0_mode=z0_mode)
    z = prob.get_zhat(0, PICK_SIMS)
    prob.close()
    assert np.array_equal(g, gr), np.argwhere(g != gr)[:10]
    assert np.array_equal(info, ir), np.argwhere(info != ir)[:10]
    assert np.array_equal(z, zr), np.argwhere(z != zr)[:10]
    _assert_oracle(O, N, 0, PICK_SIMS, THETA2 if start == "warm" else THETA, atol, int(z0_mode), g, info, z,
                   zhat0=None if zcold is None else zcold.copy())


def _assert_fd_oracle(M, O, N, sims, Hs):
    _, zfid, _ = O.map_and_score_batch("funnel", N, SEED, M.MASTER_SIM, M.MASTER_SIM + 1, THETA, atol=1e-2, z0_mode=0)   # the fiducial MAP
    for s in range(sims):
        Ho = O.fd_jacobian("funnel", N, SEED, s, THETA, STEP, zfid[0], atol=1e-2)
        np.testing.assert_allclose(Hs[s], Ho, rtol=1e-8, atol=1e-8 * np.abs(Ho).max())


@pytest.mark.parametrize("N", [1001, 64])
def test_start_pickup_copy(gpu, M, O, N):
    """Z0_COPY is the start of a finite-difference batch's problems (every one copies the fiducial MAP and samples at a theta
    other than the one it solves at): the Jacobians and solver records of 40 simulations in one call against one call each."""
    prob = _new(M, N)
    Hs, info = prob.fd_jacobian_batch(SEED, 0, PICK_SIMS, THETA, STEP, atol=1e-2)
    for s in range(PICK_SIMS):
        H1, i1 = prob.fd_jacobian_batch(SEED, s, s + 1, THETA, STEP, atol=1e-2)
        assert np.array_equal(H1[0], Hs[s]), s
        assert np.array_equal(i1[0], info[s]), s
    prob.close()
    _assert_fd_oracle(M, O, N, PICK_SIMS, Hs)


# ---- the prologue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sims", [3, 1])
def test_prologue_fewer_problems_than_compute_units(gpu, M, O, sims):
    """Every problem is its workgroup's first and last: what it reads of the launch's arguments, it reads behind the prologue alone."""
    prob = _new(M, HAND_N)
    g, info = prob.map_and_score_batch(SEED, 5, 5 + sims, THETA, atol=1e-4, z0_mode=M.Z0_ZERO)
    z = prob.get_zhat(0, sims)
    prob.close()
    _assert_oracle(O, HAND_N, 5, 5 + sims, THETA, 1e-4, 0, g, info, z)


def test_prologue_samples_at_another_theta(gpu, M, O):
    """A finite-difference call of 4 simulations: its problems sample at theta +- step and solve at theta (the descriptor's
    tsample >= 0, whose sampling coefficient comes from the launch's table, not from the MAP's theta)."""
    prob = _new(M, HAND_N)
    Hs, _ = prob.fd_jacobian_batch(SEED, 0, 4, THETA, STEP, atol=1e-2)
    prob.close()
    _assert_fd_oracle(M, O, HAND_N, 4, Hs)
