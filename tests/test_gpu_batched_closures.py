"""simple.BatchedTorchMuseProblem on the GPU against the serial TorchMuseProblem (the parent's code, unchanged) on the same device: the
same draws bit for bit, the same solver counts, MAPs within 1e-9 and scores within rtol 1e-10; muse() end to end against the exact
posterior and the serial class's θ history; the dense model of examples/closures.py; get_H_ by finite differences; the refusals."""
import importlib

import numpy as np
import pytest
import torch

from test_simple_problem import funnel_closures, gaussian_prior, mixing_problem

DEV = "cuda"
driver = importlib.import_module("museinference_jl_amd.muse")     # (the package's attribute `muse` is the function)


def funnel_batched(N, nth):
    k = (torch.arange(N) * nth) // N

    def logLike_batched(x, z, theta):
        th = theta[:, k.to(z.device)]
        return -0.5 * (torch.sum((x - z) ** 2, dim=-1) + torch.sum(torch.exp(-th) * z ** 2, dim=-1) + torch.sum(th, dim=-1))
    return logLike_batched


def funnel_closures_host_draws(N, nth):
    """funnel_closures whose random numbers come from a CPU generator seeded like the one it is handed: a run on the CPU and a run on the
    GPU then see the same draws, and differ only in the order of their sums."""
    k = (torch.arange(N) * nth) // N
    _, logLike = funnel_closures(N, nth)

    def sample_x_z(gen, theta):
        cpu = torch.Generator()
        cpu.manual_seed(gen.initial_seed())
        n1 = torch.randn(N, generator=cpu, dtype=theta.dtype).to(theta.device)
        n2 = torch.randn(N, generator=cpu, dtype=theta.dtype).to(theta.device)
        z = torch.exp(theta[k.to(theta.device)] / 2) * n1
        return z + n2, z
    return sample_x_z, logLike


def same_counts(info, infos):
    for k in ("status", "iterations", "f_calls"):
        assert np.array_equal(info[k], np.array([int(i[k]) for i in infos])), (k, info[k], [int(i[k]) for i in infos])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["vmap", "logLike_batched"])
def test_map_and_score_batch_equals_the_serial_class(M, gpu, form):
    N, theta, nsims, atol = 700, np.array([0.3, -0.8]), 6, 1e-6
    sample_x_z, logLike = funnel_closures(N, 2)
    x, _ = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV).sample_x_z(M.SimRng(5, M.DATA_SIM), theta)
    serial = M.TorchMuseProblem(x, sample_x_z, logLike, device=DEV)
    prob = M.BatchedTorchMuseProblem(x, sample_x_z, logLike, device=DEV, logLike_batched=funnel_batched(N, 2) if form == "logLike_batched" else None)
    assert not prob.supports_native_muse
    for s in range(nsims):      # the draws: bit-equal
        a, b = serial.sample_x_z(M.SimRng(9, s), theta), prob.sample_x_z(M.SimRng(9, s), theta)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    zprev = None
    for z0_mode in (M.Z0_ZERO, M.Z0_TRUE, M.Z0_WARM):      # (the warm start: from the Z0_TRUE map's MAPs)
        th = theta if z0_mode != M.Z0_WARM else theta + 0.05
        g, info = prob.map_and_score_batch(9, 0, nsims, th, include_data=True, atol=atol, z0_mode=z0_mode)
        gs, _, zs, infos = driver._map_serial(serial, 9, th, th, range(nsims), True, zprev, atol, z0_mode)
        Z = prob.get_zhat(0, nsims + 1)
        print(form, z0_mode, "f_calls", info["f_calls"], "max |dz|", max(float(np.abs(Z[e] - zs[e].cpu().numpy()).max()) for e in range(nsims + 1)),
              "max rel dg", float(np.abs(g / gs - 1).max()), "rounds", prob.last_rounds, "syncs", prob.last_syncs)
        assert g.shape == (nsims + 1, 2) and info.dtype == M._capi.INFO_DTYPE
        same_counts(info, infos)
        for e in range(nsims + 1):
            np.testing.assert_allclose(Z[e], zs[e].cpu().numpy(), rtol=0, atol=1e-9)
        np.testing.assert_allclose(g, gs, rtol=1e-10)
        np.testing.assert_allclose(info["f_min"], [float(i["f_min"]) for i in infos], rtol=1e-11)
        assert prob.last_syncs == prob.last_rounds + 1      # one synchronisation per round, one for the records
        zprev = zs
    assert info["iterations"].max() >= 1


@pytest.mark.gpu
def test_muse_on_the_funnel_against_the_exact_posterior_and_the_serial_class(M, gpu):
    from test_exact_marginal import exact_scale_family
    N, nsims = 2000, 60
    sample_x_z, logLike = funnel_closures(N, 1)
    x, _ = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV).sample_x_z(M.SimRng(5, M.DATA_SIM), [0.7])
    kw = dict(rng=11, nsims=nsims, maxsteps=30, theta_rtol=1e-4, grad_z_logLike_atol=1e-6, alpha=1.0)
    prob = M.BatchedTorchMuseProblem(x, sample_x_z, logLike, logPrior=gaussian_prior(3.0), device=DEV)
    res = M.muse(prob, [0.0], get_covariance=True, **kw)
    mode, sigma = exact_scale_family(x.cpu().numpy(), 1)
    assert np.all(np.abs(res.theta - mode) / (sigma / np.sqrt(nsims)) < 4.0), (res.theta, mode, sigma)
    assert np.all(np.abs(np.sqrt(np.diag(np.atleast_2d(res.Sigma))) / sigma - 1.0) < 0.6)
    ref = M.muse(M.TorchMuseProblem(x, sample_x_z, logLike, logPrior=gaussian_prior(3.0), device=DEV), [0.0], **kw)
    assert len(res.history) == len(ref.history)
    np.testing.assert_allclose([h["θ"] for h in res.history], [h["θ"] for h in ref.history], rtol=1e-8)
    np.testing.assert_allclose(res.theta, ref.theta, rtol=1e-8)


@pytest.mark.gpu
def test_dense_model_with_latents_and_data_of_different_lengths(M, gpu):
    """examples/closures.py's model (z of length 24 in every one of x's 40 entries), held to that example's assertion."""
    n, m = 24, 40
    A, sample_x_z, logLike = mixing_problem(M, DEV, n, m)
    x, _ = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV).sample_x_z(M.SimRng(100, M.DATA_SIM), [0.4])
    prob = M.BatchedTorchMuseProblem(x, sample_x_z, logLike, gaussian_prior(3.0), device=DEV)
    result = M.muse(prob, [0.0], rng=0, nsims=50, maxsteps=30, theta_rtol=1e-3, grad_z_logLike_atol=1e-6, alpha=1.0, get_covariance=True)
    An = A.cpu().numpy()
    lam, U = np.linalg.eigh(An @ An.T)
    y2 = (U.T @ x.cpu().numpy()) ** 2
    ts = np.linspace(-6, 6, 4001)
    lp = np.array([-0.5 * np.sum(np.log1p(np.exp(t) * lam) + y2 / (1 + np.exp(t) * lam)) - 0.5 * t * t / 9.0 for t in ts])
    w = np.exp(lp - lp.max())
    w /= w.sum()
    mean = float(np.sum(w * ts))
    sd = float(np.sqrt(np.sum(w * (ts - mean) ** 2)))
    sigma = float(np.sqrt(result.Sigma[0, 0]))
    assert prob.get_zhat(0, 1).shape == (1, n)
    assert abs(result.theta[0] - ts[np.argmax(lp)]) < 2.5 * sd and 0.3 < sigma / sd < 3.0


FD = dict(N=300, theta0=np.array([0.3, -0.8]), step=np.array([0.05, 0.08]), rng=3, nsims=3, atol=1e-8)
# How far the SERIAL class's H moves between a run on the CPU and a run on the GPU with the same draws (funnel_closures_host_draws: two
# runs of the reference path that differ only in the order of sums), max |dH| over the three 2 x 2 Jacobians; measured by
# measure_serial_H_between_devices() below on an MI355X: 2.13e-13 (|H| up to 28; the same value in two runs).
SERIAL_H_MOVES = 2.1316282072803006e-13


def serial_fd(M, device):
    sample_x_z, logLike = funnel_closures_host_draws(FD["N"], 2)
    prob = M.TorchMuseProblem(None, sample_x_z, logLike, device=device)
    return np.array(driver._fd_serial(prob, FD["rng"], FD["nsims"], FD["theta0"], M.central_fdm(3, 1), FD["step"], FD["atol"], None, 0))


def measure_serial_H_between_devices(M):
    return float(np.abs(serial_fd(M, "cpu") - serial_fd(M, DEV)).max())


@pytest.mark.gpu
def test_fd_jacobian_batch_equals_the_serial_finite_differences(M, gpu):
    """get_H_'s finite-difference map, nsims = 3, nθ = 2, MAPs to 1e-8: fd_jacobian_batch against muse._fd_serial on the serial class.
    Tolerance: ten times SERIAL_H_MOVES, the distance between two runs of the serial path itself (see there): 2.13e-12.  Measured
    between the batched and the serial class on an MI355X: 1.8e-13."""
    sample_x_z, logLike = funnel_closures_host_draws(FD["N"], 2)
    prob = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    Hs, info = prob.fd_jacobian_batch(FD["rng"], 0, FD["nsims"], FD["theta0"], FD["step"], atol=FD["atol"], fid_mode=0, fid_sim=M.MASTER_SIM)
    ref = serial_fd(M, DEV)
    print("max |dH| batched - serial", float(np.abs(Hs - ref).max()), "serial cpu - gpu", measure_serial_H_between_devices(M), "|H|", float(np.abs(ref).max()))
    assert Hs.shape == (3, 2, 2) and info.shape == (3, 2, 2) and np.all(info["status"] == 0)
    np.testing.assert_allclose(Hs, ref, rtol=0, atol=10 * SERIAL_H_MOVES)
    # ... and through the driver: get_H_ takes the batched seam
    res = M.MuseResult()
    res.theta = FD["theta0"]
    M.get_H_(res, prob, rng=FD["rng"], nsims=FD["nsims"], step=FD["step"], grad_z_logLike_atol=FD["atol"])
    np.testing.assert_allclose(res.H, ref.mean(axis=0), rtol=0, atol=10 * SERIAL_H_MOVES)


def test_a_cpu_device_is_refused(M):
    sample_x_z, logLike = funnel_closures(10, 1)
    with pytest.raises(M.MuseError) as e:
        M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device="cpu")
    assert "no HIP device" in str(e.value)


@pytest.mark.gpu
def test_a_closure_vmap_cannot_trace_is_refused(M, gpu):
    sample_x_z, _ = funnel_closures(10, 1)

    def logLike(x, z, theta):
        return -0.5 * (torch.sum((x - z) ** 2) + float(torch.exp(-theta[0]).item()) * torch.sum(z ** 2))
    prob = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    with pytest.raises(ValueError, match="logLike_batched"):
        prob.map_and_score_batch(1, 0, 2, [0.1], atol=1e-4)
