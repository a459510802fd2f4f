"""BatchedTorchMuseProblem(sample_x_z_batched=...) on the GPU: all simulations of a map drawn at once from the ENGINE's streams
(EngineNormals: libmuse_lbfgs.so's muse_lbfgs_normals).  The draws against the oracle bit for bit; the map against a serial loop over the
public per-simulation calls; batch independence; the finite-difference and the implicit get_H!; the oracle's funnel as checker of the
closure path; and the default path (no batched sampler), which must not have moved.

Models: the funnel as closures with N = 300, nθ = 2 and the dense model with n = 24, m = 40 (tests/test_gpu_batched_implicit.py's)."""
import numpy as np
import pytest
import torch

from test_simple_problem import funnel_closures, mixing_problem
from test_gpu_batched_closures import same_counts

DEV = "cuda"
N, NTH = 300, 2
THETA = np.array([0.3, -0.8])
DENSE = dict(n=24, m=40, theta=np.array([0.4]))


def funnel_engine(N, nth):
    """The funnel on engine streams: element i of a simulation takes the pair (n1(i), n2(i)) the header model gives it."""
    k = (torch.arange(N) * nth) // N

    def sample_x_z_batched(normals, theta):
        e = normals(N, 2)
        z = torch.exp(theta[:, k.to(theta.device)] / 2) * e[..., 0]
        return z + e[..., 1], z
    return sample_x_z_batched, funnel_closures(N, nth)[1]


def dense_engine(M):
    """mixing_problem's model, two requests per draw: the latents' n numbers, then the noise's m."""
    n, m = DENSE["n"], DENSE["m"]
    A, _, logLike = mixing_problem(M, DEV, n, m)

    def sample_x_z_batched(normals, theta):
        z = torch.exp(theta[:, :1] / 2) * normals(n)
        return z @ A.T + normals(m), z
    return sample_x_z_batched, logLike


def problem(M, model, x=None):
    sampler, logLike = funnel_engine(N, NTH) if model == "funnel" else dense_engine(M)
    theta = THETA if model == "funnel" else DENSE["theta"]
    return M.BatchedTorchMuseProblem(x, None, logLike, device=DEV, sample_x_z_batched=sampler), theta


@pytest.mark.gpu
def test_funnel_draws_are_the_engines_bit_for_bit(M, O, gpu):
    assert O.exp_fixed(0.0) == 1.0
    prob, _ = problem(M, "funnel")
    seed = 7
    k = (torch.arange(N) * NTH) // N
    for sim in range(4):
        x, z = prob.sample_x_z(M.SimRng(seed, sim), np.zeros(NTH))
        xo, zo = O.sample_x_z("funnel", N, seed, sim, np.zeros(NTH))
        assert x.shape == (N,) and z.shape == (N,) and not x.requires_grad
        assert torch.equal(x.cpu().view(torch.int64), torch.as_tensor(xo).view(torch.int64))
        assert torch.equal(z.cpu().view(torch.int64), torch.as_tensor(zo).view(torch.int64))
        # θ = (0.3, -0.8): torch's exp, so sd n1 and z + n2 in torch from the oracle's normals
        n1, n2 = (torch.as_tensor(a, device=DEV) for a in O.normals(seed, sim, N))
        x, z = prob.sample_x_z(M.SimRng(seed, sim), THETA)
        zt = torch.exp(torch.as_tensor(THETA, device=DEV)[k.to(DEV)] / 2) * n1
        assert torch.equal(z.view(torch.int64), zt.view(torch.int64)) and torch.equal(x.view(torch.int64), (zt + n2).view(torch.int64))
    # ... and the same bits in a batch: row b of a map's one call
    X, Z = prob._draw_sims(seed, [0, 1, 2, 3], prob._theta_rows(THETA, 4))
    for sim in range(4):
        x, z = prob.sample_x_z(M.SimRng(seed, sim), THETA)
        assert torch.equal(X[sim], x) and torch.equal(Z[sim], z)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["funnel", "dense"])
def test_map_and_score_batch_equals_a_serial_loop(M, gpu, model):
    """The bounds of test_map_and_score_batch_equals_the_serial_class: equal status, iterations and f_calls, MAPs within 1e-9, scores to
    rtol 1e-10.  The serial side: prob.sample_x_z(SimRng(seed, s), θ), TorchMuseProblem.zhat_at_theta, grad_theta_logLike."""
    seed, nsims, atol = 9, 6, 1e-6
    draws, theta = problem(M, model)
    xdata, _ = draws.sample_x_z(M.SimRng(5, M.DATA_SIM), theta)
    prob, _ = problem(M, model, xdata)
    g, info = prob.map_and_score_batch(seed, 0, nsims, theta, include_data=True, atol=atol, z0_mode=M.Z0_ZERO)
    Z = prob.get_zhat(0, nsims + 1)
    gs, infos, zs = [], [], []
    for e in range(nsims + 1):
        x = xdata if e == 0 else prob.sample_x_z(M.SimRng(seed, e - 1), theta)[0]
        zh, rec = M.TorchMuseProblem.zhat_at_theta(prob, x, torch.zeros(Z.shape[1], dtype=torch.float64, device=DEV), theta, atol)
        gs.append(prob.grad_theta_logLike(x, zh, theta))
        infos.append(rec)
        zs.append(zh.cpu().numpy())
    gs = np.array(gs)
    print(model, "f_calls", info["f_calls"], "max |dz|", float(np.abs(Z - np.array(zs)).max()), "max rel dg", float(np.abs(g / gs - 1).max()))
    assert g.shape == (nsims + 1, theta.size) and info["iterations"].max() >= 1
    same_counts(info, infos)
    np.testing.assert_allclose(Z, np.array(zs), rtol=0, atol=1e-9)
    np.testing.assert_allclose(g, gs, rtol=1e-10)


@pytest.mark.gpu
def test_a_map_does_not_depend_on_how_the_simulations_are_batched(M, gpu):
    seed, atol = 9, 1e-6
    prob, theta = problem(M, "funnel")
    g, info = prob.map_and_score_batch(seed, 0, 6, theta, atol=atol)
    Z = prob.get_zhat(0, 6)
    for a, b in ((0, 2), (2, 6)):
        part, _ = problem(M, "funnel")
        gp, ip = part.map_and_score_batch(seed, a, b, theta, atol=atol)
        assert np.array_equal(gp, g[a:b]) and ip.tobytes() == info[a:b].tobytes()
        assert np.array_equal(part.get_zhat(0, b - a), Z[a:b])


@pytest.mark.gpu
def test_implicit_H_equals_the_finite_difference_H_on_engine_streams(M, gpu):
    """The bound of test_implicit_H_equals_the_finite_difference_H_on_tight_maps: rtol 1e-6, atol 1e-6 max |H|; fiducial MAPs per
    simulation (fid_mode = 1)."""
    seed, nsims = 3, 3
    prob, theta = problem(M, "funnel")
    Hs, its = prob.implicit_H_batch(seed, 0, nsims, theta, atol=1e-10)
    Hfd, info = prob.fd_jacobian_batch(seed, 0, nsims, theta, np.array([1e-4, 1e-4]), atol=1e-12, fid_mode=1)
    print("max |H implicit - H fd|", float(np.abs(Hs - Hfd).max()), "|H|", float(np.abs(Hfd).max()), "counts", its.ravel())
    assert Hs.shape == (nsims, NTH, NTH) and info.shape == (nsims, NTH, 2)
    assert np.all(its >= 1) and np.all(info["status"] == 0)
    for s in range(nsims):
        np.testing.assert_allclose(Hs[s], Hfd[s], rtol=1e-6, atol=1e-6 * np.abs(Hfd[s]).max())
    # the fiducial at the master stream (fid_mode = 0): the same rows, another starting point -- the same bound
    Hfd0, info0 = prob.fd_jacobian_batch(seed, 0, nsims, theta, np.array([1e-4, 1e-4]), atol=1e-12, fid_mode=0)
    assert np.all(info0["status"] == 0)
    for s in range(nsims):
        np.testing.assert_allclose(Hfd0[s], Hfd[s], rtol=1e-6, atol=1e-6 * np.abs(Hfd[s]).max())


@pytest.mark.gpu
def test_implicit_chunks_give_the_same_bits(M, gpu):
    seed, nsims = 3, 3
    prob, theta = problem(M, "funnel")
    Hs, its = prob.implicit_H_batch(seed, 0, nsims, theta, atol=1e-8)
    assert prob.last_cg_chunks == 1
    prob.IMPLICIT_MAX_ELEMS = N * NTH
    Hc, itc = prob.implicit_H_batch(seed, 0, nsims, theta, atol=1e-8)
    assert prob.last_cg_chunks == nsims
    assert np.array_equal(Hs, Hc) and np.array_equal(its, itc)


@pytest.mark.gpu
def test_the_draws_as_functions_of_theta_are_the_same_numbers(M, gpu):
    """What _implicit_chunk relies on, for a sampler with two requests per draw (the dense model): the same streams from their start
    (EngineNormals.fresh) at a θ that requires grad give the first call's x and z bit for bit, now differentiable in θ."""
    prob, theta = problem(M, "dense")
    normals = M.EngineNormals(DEV, 4, [0, 1, 2, M.MASTER_SIM])
    TH = prob._theta_rows(theta, 4)
    X, Z = prob._draw_rows(normals, TH)
    assert X.shape == (4, DENSE["m"]) and Z.shape == (4, DENSE["n"]) and not X.requires_grad and normals.cursor == 12 + 20
    th = TH.clone().requires_grad_(True)
    Xg, Zg = prob._draw_rows(normals.fresh(), th)
    assert Xg.requires_grad and Zg.requires_grad and torch.equal(Xg.detach(), X) and torch.equal(Zg.detach(), Z)
    row, = torch.autograd.grad(Zg[2].sum(), th)
    assert torch.all(row[[0, 1, 3]] == 0) and row[2, 0] != 0          # row b depends on its own θ row only
    Hs, its = prob.implicit_H_batch(4, 0, 3, theta, atol=1e-8)
    assert Hs.shape == (3, 1, 1) and np.all(its >= 1) and np.all(np.isfinite(Hs)) and np.all(Hs != 0)


ORACLE_CASES = [(np.array([0.3, -0.8]), 1e-6), (np.array([0.0, 0.0]), 1e-2), (np.array([1.0, 0.5]), 1e-8)]


@pytest.mark.gpu
def test_the_oracles_funnel_checks_the_closure_path(M, O, gpu):
    """Funnel closures on engine streams against oracle.map_and_score_batch("funnel", ...) on the same seed, cold maps, the data's
    element included: the same simulations, so equal solver counts and scores to the project's parity bound, rtol 1e-10 (the closure
    takes exp from torch, the oracle its fixed sequence; the sums differ in order).  Measured on an MI355X over the three cases:
    max relative score difference 1.8e-15 (1.0e-15, 5.6e-16, 1.8e-15), MAPs within 8.9e-16 -- far inside the parity bound, which stays."""
    seed, nsims = 7, 6
    worst = 0.0
    for theta, atol in ORACLE_CASES:
        xdata, _ = O.sample_x_z("funnel", N, 5, M.DATA_SIM, theta)
        prob, _ = problem(M, "funnel", xdata)
        g, info = prob.map_and_score_batch(seed, 0, nsims, theta, include_data=True, atol=atol, z0_mode=M.Z0_ZERO)
        go, zo, io = O.map_and_score_batch("funnel", N, seed, 0, nsims, theta, atol=atol, x_data=xdata, z0_mode=0)
        rel = float(np.abs(g / go - 1).max())
        worst = max(worst, rel)
        print("theta", theta, "atol", atol, "f_calls", info["f_calls"], "max rel dg", rel, "max |dz|", float(np.abs(prob.get_zhat(0, nsims + 1) - zo).max()))
        for k in ("status", "iterations", "f_calls"):
            assert np.array_equal(info[k], io[k]), (k, info[k], io[k])
        np.testing.assert_allclose(g, go, rtol=1e-10)
        np.testing.assert_allclose(prob.get_zhat(0, nsims + 1), zo, rtol=0, atol=1e-9)
    print("max rel dg over the cases", worst)


@pytest.mark.gpu
def test_the_default_path_has_not_moved(M, gpu, monkeypatch):
    """Without sample_x_z_batched: the draws are the serial class's (torch.Generator streams), no EngineNormals is made, and
    map_and_score_batch is, bit for bit, the solve and the scores of its own per-simulation draws stacked."""
    from museinference_jl_amd import simple

    def refuse(*a, **k):
        raise AssertionError("the default path made an EngineNormals")
    monkeypatch.setattr(simple, "EngineNormals", refuse)
    seed, nsims, atol = 9, 5, 1e-6
    sample_x_z, logLike = funnel_closures(N, NTH)
    prob = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    serial = M.TorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    g, info = prob.map_and_score_batch(seed, 0, nsims, THETA, atol=atol)
    Z = prob.get_zhat(0, nsims)
    xs = []
    for s in range(nsims):
        x, z = prob.sample_x_z(M.SimRng(seed, s), THETA)
        xs_, zs_ = serial.sample_x_z(M.SimRng(seed, s), THETA)
        assert torch.equal(x, xs_) and torch.equal(z, zs_)
        xs.append(x)
    other = M.BatchedTorchMuseProblem(None, sample_x_z, logLike, device=DEV)
    other._zshape = (N,)
    X, TH = torch.stack(xs), other._theta_rows(THETA, nsims)
    zhat, rec = other._solve(X, torch.zeros((nsims, N), dtype=torch.float64, device=DEV), TH, atol)
    assert np.array_equal(other._scores(X, zhat, TH), g) and rec.tobytes() == info.tobytes()
    assert np.array_equal(zhat.cpu().numpy(), Z)
