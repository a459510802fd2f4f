"""BatchedTorchMuseProblem.implicit_H_batch on the GPU (get_H! by implicit differentiation, all simulations at once: lock-step L-BFGS
for the fiducial MAPs, lock-step conjugate gradients for the nsims nθ linear solves) against the serial TorchMuseProblem's
implicit_H_batch (the parent's code, unchanged) on the same device: the same draws bit for bit, the same solver and CG counts, Hs
within ten times what the serial path itself moves between a CPU and a GPU run; chunking, the driver's keywords, the refusal of a
preconditioner, and the finite-difference H on tight MAPs."""
import importlib

import numpy as np
import pytest
import torch

from test_simple_problem import mixing_problem
from test_gpu_batched_closures import funnel_closures_host_draws, same_counts

DEV = "cuda"
driver = importlib.import_module("museinference_jl_amd.muse")

FUNNEL = dict(N=300, nth=2, theta0=np.array([0.3, -0.8]), seed=3, nsims=3, atol=1e-8)
# The dense model (z of length 24 in every one of x's 40 entries), 4 simulations.  Its CG counts (17 or 18 of at most 24) are decided by
# |r| <= sqrt(eps) |b| in the last iterations, where the order of the sums can move a count by one.  The seed is the first of 0, 1, 2, ...
# whose serial counts are the same in a CPU run, a GPU run and a GPU run with the latents permuted (pick_dense_seed() below prints the
# three rows per seed).  On an MI355X seed 0 gave [17 18 18 18] three times (as did each of the seeds 1 - 5 its own row).
DENSE = dict(n=24, m=40, theta0=np.array([0.4]), seed=0, nsims=4, atol=1e-8)
# How far the SERIAL class's implicit Hs move between a run on the CPU and a run on the GPU with the same draws (host draws: the two
# runs of the reference path differ only in the order of their sums), max |dH|; measured by measure_serial_H_between_devices() below
# on an MI355X: funnel 3.55e-15 (|H| up to 28; the same value in two runs), dense 1.04e-13 (|H| up to 6.5; seeds 1 - 5: 0.4 - 2.5e-13).
SERIAL_H_MOVES = {"funnel": 3.552713678800501e-15, "dense": 1.0391687510491465e-13}


def mixing_host_draws(M, device, n, m, perm=None):
    """mixing_problem with its random numbers from a CPU generator seeded like the one it is handed (as funnel_closures_host_draws), and
    optionally with the latents permuted (the same model: z -> z[perm], A's columns with it)."""
    A, _, _ = mixing_problem(M, "cpu", n, m)
    if perm is not None:
        A = A[:, perm]
    A = A.to(device)

    def sample_x_z(gen, theta):
        cpu = torch.Generator()
        cpu.manual_seed(gen.initial_seed())
        z = torch.randn(n, generator=cpu, dtype=theta.dtype)
        e = torch.randn(m, generator=cpu, dtype=theta.dtype).to(theta.device)
        z = (z if perm is None else z[perm]).to(theta.device)
        z = torch.exp(theta[0] / 2) * z
        return A.to(theta.device) @ z + e, z

    def logLike(x, z, theta):
        r = x - A.to(z.device) @ z
        return -0.5 * (torch.sum(r * r) + torch.exp(-theta[0]) * torch.sum(z * z) + n * theta[0])
    return sample_x_z, logLike


def noise_closures_host_draws(N):
    """z ~ N(0, e^θ0), x ~ N(z, e^θ1): the score's θ1 component holds (x - z)², so -- unlike the funnel's and the dense model's, whose θ
    multiplies z² alone -- it depends on the draw and H1 is not zero."""
    def sample_x_z(gen, theta):
        cpu = torch.Generator()
        cpu.manual_seed(gen.initial_seed())
        n1 = torch.randn(N, generator=cpu, dtype=theta.dtype).to(theta.device)
        n2 = torch.randn(N, generator=cpu, dtype=theta.dtype).to(theta.device)
        z = torch.exp(theta[0] / 2) * n1
        return z + torch.exp(theta[1] / 2) * n2, z

    def logLike(x, z, theta):
        return -0.5 * (torch.exp(-theta[1]) * torch.sum((x - z) ** 2) + N * theta[1] + torch.exp(-theta[0]) * torch.sum(z ** 2) + N * theta[0])
    return sample_x_z, logLike


NOISE = dict(N=50, theta0=np.array([0.3, -0.5]), seed=4, nsims=3)


def closures(M, model, device, perm=None):
    if model == "funnel":
        return funnel_closures_host_draws(FUNNEL["N"], FUNNEL["nth"]), FUNNEL
    return mixing_host_draws(M, device, DENSE["n"], DENSE["m"], perm), DENSE


def serial_implicit(M, model, device, perm=None, seed=None):
    (sample_x_z, logLike), c = closures(M, model, device, perm)
    prob = M.TorchMuseProblem(None, sample_x_z, logLike, device=device)
    return prob.implicit_H_batch(c["seed"] if seed is None else seed, 0, c["nsims"], c["theta0"], atol=c["atol"])


def measure_serial_H_between_devices(M, model):
    return float(np.abs(serial_implicit(M, model, "cpu")[0] - serial_implicit(M, model, DEV)[0]).max())


def pick_dense_seed(M, seeds=range(6)):
    perm = torch.as_tensor(np.random.RandomState(5).permutation(DENSE["n"]))
    for seed in seeds:
        rows = [serial_implicit(M, "dense", "cpu", seed=seed)[1].ravel(), serial_implicit(M, "dense", DEV, seed=seed)[1].ravel(),
                serial_implicit(M, "dense", DEV, perm=perm, seed=seed)[1].ravel()]
        print("seed", seed, "cpu", rows[0], "gpu", rows[1], "gpu permuted", rows[2], "agree", all(np.array_equal(rows[0], r) for r in rows))


_serial = {}


def serial_reference(M, model):
    """The serial class on the GPU, once per model: (Hs, counts)"""
    if model not in _serial:
        _serial[model] = serial_implicit(M, model, DEV)
    return _serial[model]


def batched(M, model):
    (sample_x_z, logLike), c = closures(M, model, DEV)
    return M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV), c


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["funnel", "dense"])
def test_implicit_H_batch_equals_the_serial_class(M, gpu, model):
    """Tolerance: ten times SERIAL_H_MOVES[model], the distance between two runs of the serial path itself: funnel 3.55e-14, dense
    1.04e-12.  Measured between the batched and the serial class on an MI355X: funnel 2.5e-14, dense 1.7e-13."""
    prob, c = batched(M, model)
    serial = M.TorchMuseProblem(None, prob._sample, prob._logLike, device=DEV)
    infos = []
    for s in range(c["nsims"]):      # the draws: bit-equal; the fiducial MAPs' records
        a, b = serial.sample_x_z(M.SimRng(c["seed"], s), c["theta0"]), prob.sample_x_z(M.SimRng(c["seed"], s), c["theta0"])
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        infos.append(serial.zhat_at_theta(a[0], torch.zeros_like(a[1]), c["theta0"], c["atol"])[1])
    Hs, its = prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=c["atol"])
    ref, ref_its = serial_reference(M, model)
    nth = c["theta0"].size
    print(model, "max |dH| batched - serial", float(np.abs(Hs - ref).max()), "|H|", float(np.abs(ref).max()), "counts", its.ravel(), "serial",
          ref_its.ravel(), "rounds", prob.last_cg_rounds, "syncs", prob.last_cg_syncs)
    assert Hs.shape == (c["nsims"], nth, nth) and its.shape == (c["nsims"], nth) and its.dtype == np.int32
    same_counts(prob.last_fiducial_info, infos)
    assert np.array_equal(its, ref_its)
    if model == "funnel":
        assert np.all(its == 1)       # b lives in one block, where the Hessian is a multiple of the identity
    assert prob.last_cg_chunks == 1 and prob.last_cg_rounds == its.max() and prob.last_cg_syncs == prob.last_cg_rounds + 2
    np.testing.assert_allclose(Hs, ref, rtol=0, atol=10 * SERIAL_H_MOVES[model])


@pytest.mark.gpu
def test_chunks_of_one_simulation_give_the_same_bits(M, gpu):
    """Rows are independent: for a closure whose batched form is elementwise with per-row sums (the funnel under vmap) the chunking
    changes nothing.  (A closure that becomes a batched matrix product is as row-independent as torch's kernels for it are.)"""
    prob, c = batched(M, "funnel")
    Hs, its = prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=c["atol"])
    prob.IMPLICIT_MAX_ELEMS = c["N"] * c["nth"]
    Hc, itc = prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=c["atol"])
    assert prob.last_cg_chunks == c["nsims"] and prob.last_cg_syncs == prob.last_cg_rounds + 2 * prob.last_cg_chunks
    assert np.array_equal(Hs, Hc) and np.array_equal(its, itc)


@pytest.mark.gpu
def test_the_driver_reaches_the_batched_seam_with_every_keyword(M, gpu):
    prob, c = batched(M, "funnel")
    full, _ = prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"])

    def get_H(**kw):
        res = M.MuseResult()
        res.theta = c["theta0"]
        M.get_H_(res, prob, rng=c["seed"], nsims=c["nsims"], implicit_diff=True, **kw)
        return res
    res = get_H()
    hists = np.array(res.metadata["implicit_diff_cg_hists"])
    assert hists.shape == (c["nsims"], c["nth"]) and np.all(hists == 1)
    np.testing.assert_array_equal(res.H, full.mean(axis=0))
    # H1_is_zero and IterativeSolvers' keywords: a TypeError on the inherited serial seam
    res0 = get_H(implicit_diff_H1_is_zero=True, implicit_diff_cg_kwargs={"abstol": 1e-3, "maxiter": 5})
    assert np.array(res0.metadata["implicit_diff_cg_hists"]).shape == (c["nsims"], c["nth"])
    with pytest.raises(ValueError, match="jacobi"):
        get_H(implicit_diff_cg_kwargs={"Pl": "jacobi"})


@pytest.mark.gpu
def test_H1_is_zero_leaves_out_exactly_H1(M, gpu):
    """On a model whose H1 is not zero (the funnel's and the dense model's are, identically).  H1 itself is the H of a call whose CG takes
    no iteration (maxiter = 0: y = 0, H = H1), and that is compared with the serial class's: sums of N = 50 terms of either sign in
    float64, bounded here by 1e-12 |H| (N eps |H| ~ 1e-14 |H|); `full - (H1 = 0 call)` against it adds one subtraction's rounding."""
    sample_x_z, logLike = noise_closures_host_draws(NOISE["N"])
    prob = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    serial = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    args = (NOISE["seed"], 0, NOISE["nsims"], NOISE["theta0"])
    full, its = prob.implicit_H_batch(*args)
    Hz, _ = prob.implicit_H_batch(*args, H1_is_zero=True)
    H1, k0 = prob.implicit_H_batch(*args, cg_maxiter=0)
    H1s, _ = serial.implicit_H_batch(*args, cg_maxiter=0)
    scale = float(np.abs(full).max())
    print("|H1|", float(np.abs(H1).max()), "|H|", scale, "max |H1 - serial H1|", float(np.abs(H1 - H1s).max()), "max |(full - Hz) - H1|",
          float(np.abs(full - Hz - H1).max()), "counts", its.ravel())
    assert np.all(k0 == 0) and np.all(its >= 1) and np.abs(H1).max() > 1e-3 * scale
    np.testing.assert_allclose(H1, H1s, rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(full - Hz, H1, rtol=0, atol=1e-12 * scale)


@pytest.mark.gpu
def test_implicit_H_equals_the_finite_difference_H_on_tight_maps(M, gpu):
    """The bound test_implicit_differentiation_H_by_autograd holds the serial class to: rtol 1e-6, atol 1e-6 max |H|."""
    prob, c = batched(M, "funnel")
    Hs, its = prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=1e-10)
    Hfd, info = prob.fd_jacobian_batch(c["seed"], 0, c["nsims"], c["theta0"], np.array([1e-4, 1e-4]), atol=1e-12, fid_mode=1)
    print("max |H implicit - H fd|", float(np.abs(Hs - Hfd).max()), "|H|", float(np.abs(Hfd).max()))
    assert np.all(its >= 1) and np.all(info["status"] == 0)
    for s in range(c["nsims"]):
        np.testing.assert_allclose(Hs[s], Hfd[s], rtol=1e-6, atol=1e-6 * np.abs(Hfd[s]).max())
