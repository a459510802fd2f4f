"""implicit_diff_cg_kwargs' Pl = "jacobi" for closure problems, on the CPU through the serial TorchMuseProblem: the constructor's hess_diag
(a callable, a tensor of probes, "elementwise") says what the diagonal is, implicit_H_batch(cg_Pl="jacobi") runs simple._pcg with it.

Two models, both with badly scaled latents (tests/test_gpu_batched_preconditioned.py runs the same two through the batched class):

    heteroscedastic elementwise   z ~ N(0, e^θ0), x_i ~ N(z_i, σ_i² e^θ1), σ_i = exp(sin(1.7 i)), N = 50.  The Hessian in z is diagonal,
                                  d_i = e^-θ1 / σ_i² + e^-θ0: N distinct values, so plain CG takes many iterations and the preconditioned
                                  one exactly 1, with the analytic diagonal or the all-ones probe.
    scaled dense                  z ~ N(0, e^θ I_24), x ~ N(A (w ⊙ z), I_40), w_i = exp(2 sin(1.7 i + 0.3)).  The Hessian is
                                  W AᵀA W + e^-θ I, its diagonal w_i² (AᵀA)_ii + e^-θ.

The bound between a preconditioned and a plain H at cg_reltol = 1e-12: both solves end at a recurrence residual |r| <= reltol |b|, so
each y_j is within |M⁻¹| |r| <= reltol |b_j| / λ_min of the exact one, the recurrence residual is within about k eps κ |b_j| of the true
one after k iterations, and H_ij = H1_ij - dF_i . y_j moves by at most |dF_i| times that, twice (two solves):
    |ΔH_ij| <= 2 (reltol + k eps κ) |dF_i| |b_j| / λ_min
with dF, b, λ_min and κ computed by the test itself from the model (h_bound below)."""
import numpy as np
import pytest
import torch

from test_simple_problem import mixing_problem

EPS = float(np.finfo(np.float64).eps)
HETERO = dict(N=50, theta0=np.array([0.3, -0.5]), seed=4, nsims=3, atol=1e-8)
SCALED = dict(n=24, m=40, theta0=np.array([0.4]), seed=0, nsims=4, atol=1e-8)


def hetero_sigma(N, device="cpu"):
    return torch.exp(torch.sin(1.7 * torch.arange(N, dtype=torch.float64))).to(device)


def hetero_closures(N, device="cpu"):
    """(sample_x_z, logLike, hess_diag, logLike_batched): the random numbers from a CPU generator seeded like the one handed in, so that
    a simulation's draw is the same bits on every device."""
    sig = hetero_sigma(N, device)

    def sample_x_z(gen, theta):
        cpu = torch.Generator()
        cpu.manual_seed(gen.initial_seed())
        n1 = torch.randn(N, generator=cpu, dtype=theta.dtype).to(theta.device)
        n2 = torch.randn(N, generator=cpu, dtype=theta.dtype).to(theta.device)
        z = torch.exp(theta[0] / 2) * n1
        return z + sig * torch.exp(theta[1] / 2) * n2, z

    def logLike(x, z, theta):
        return -0.5 * (torch.exp(-theta[1]) * torch.sum(((x - z) / sig) ** 2) + N * theta[1] + torch.exp(-theta[0]) * torch.sum(z ** 2) + N * theta[0])

    def hess_diag(x, z, theta):          # [B, N]: the diagonal of -∂²logLike/∂z², row b at its own θ
        return torch.exp(-theta[:, 1:2]) / sig ** 2 + torch.exp(-theta[:, 0:1]) + 0.0 * z

    def logLike_batched(x, z, theta):
        return -0.5 * (torch.exp(-theta[:, 1]) * torch.sum(((x - z) / sig) ** 2, dim=1) + N * theta[:, 1]
                       + torch.exp(-theta[:, 0]) * torch.sum(z ** 2, dim=1) + N * theta[:, 0])
    return sample_x_z, logLike, hess_diag, logLike_batched


def scaled_weights(n):
    return torch.exp(2.0 * torch.sin(1.7 * torch.arange(n, dtype=torch.float64) + 0.3))


def scaled_dense_closures(M, device="cpu", n=SCALED["n"], m=SCALED["m"], perm=None):
    """(sample_x_z, logLike, hess_diag, A, w): mixing_problem's A with the latents scaled by w, host draws as above; optionally with the
    latents permuted (the same model: z -> z[perm], A's columns and w with it)."""
    A, _, _ = mixing_problem(M, "cpu", n, m)
    w = scaled_weights(n)
    if perm is not None:
        A, w = A[:, perm], w[perm]
    A, w = A.to(device), w.to(device)
    ata = torch.sum(A * A, dim=0)

    def sample_x_z(gen, theta):
        cpu = torch.Generator()
        cpu.manual_seed(gen.initial_seed())
        z = torch.randn(n, generator=cpu, dtype=theta.dtype)
        e = torch.randn(m, generator=cpu, dtype=theta.dtype).to(theta.device)
        z = (z if perm is None else z[perm]).to(theta.device)
        z = torch.exp(theta[0] / 2) * z
        return A @ (w * z) + e, z

    def logLike(x, z, theta):
        r = x - A @ (w * z)
        return -0.5 * (torch.sum(r * r) + torch.exp(-theta[0]) * torch.sum(z * z) + n * theta[0])

    def hess_diag(x, z, theta):
        return w ** 2 * ata + torch.exp(-theta[:, 0:1]) + 0.0 * z
    return sample_x_z, logLike, hess_diag, A, w


def model(M, name, device="cpu", hess_diag="callable", perm=None):
    """(the serial problem, its constants, the model's Hessian in z at θ0 as a dense matrix)"""
    if name == "hetero":
        c = HETERO
        sample, logLike, hd, _ = hetero_closures(c["N"], device)
        Hz = torch.diag(np.exp(-c["theta0"][1]) / hetero_sigma(c["N"]) ** 2 + np.exp(-c["theta0"][0]))
    else:
        c = SCALED
        sample, logLike, hd, A, w = scaled_dense_closures(M, device, perm=perm)
        A, w = A.cpu(), w.cpu()
        Hz = w[:, None] * (A.T @ A) * w[None, :] + np.exp(-c["theta0"][0]) * torch.eye(c["n"], dtype=torch.float64)
    kind = {"callable": hd, "none": None}.get(hess_diag, hess_diag)
    return M.TorchMuseProblem(None, sample, logLike, device=device, hess_diag=kind), c, Hz


def implicit(prob, c, **kw):
    return prob.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=c["atol"], **kw)


def h_bound(M, prob, c, Hz, reltol, kmax):
    """[nsims, nθ, nθ]: 2 (reltol + k eps κ) |dF_i| |b_j| / λ_min (the module docstring), dF and b by autograd as the seam takes them."""
    lam = np.linalg.eigvalsh(Hz.numpy())
    jac = torch.autograd.functional.jacobian
    th0 = prob._theta(c["theta0"])
    out = []
    for s in range(c["nsims"]):
        rng = M.SimRng(c["seed"], s)
        x, z = prob.sample_x_z(rng, c["theta0"])
        zh = prob.zhat_at_theta(x, torch.zeros_like(z), c["theta0"], c["atol"])[0].detach()

        def x_of(th):
            gen = torch.Generator(device=prob.device)
            gen.manual_seed(prob._stream(rng))
            return prob._sample(gen, th)[0]

        def grad_z(xx, th):
            zz = zh.clone().requires_grad_(True)
            return torch.autograd.grad(prob._logLike(xx, zz, th), zz, create_graph=True)[0]
        dF = jac(lambda th: grad_z(x, th), th0).reshape(-1, th0.numel())
        b = jac(lambda th: grad_z(x_of(th), th0), th0).reshape(-1, th0.numel())
        out.append(2 * (reltol + kmax * EPS * lam[-1] / lam[0]) * np.outer(dF.norm(dim=0).numpy(), b.norm(dim=0).numpy()) / lam[0])
    return np.array(out)


def test_hetero_model_takes_one_iteration_with_its_diagonal(M):
    prob, c, Hz = model(M, "hetero", hess_diag="none")
    Hp, kp = implicit(prob, c, cg_reltol=1e-12)
    assert np.all(kp > 1)
    bound = h_bound(M, prob, c, Hz, 1e-12, int(kp.max()))
    for kind in ("elementwise", "callable"):
        pj, _, _ = model(M, "hetero", hess_diag=kind)
        Hj, kj = implicit(pj, c, cg_reltol=1e-12, cg_Pl="jacobi")
        print("hetero", kind, "counts", kj.ravel(), "plain", kp.ravel(), "max |dH|", float(np.abs(Hj - Hp).max()), "bound", float(bound.min()),
              "|H|", float(np.abs(Hp).max()))
        assert kj.shape == kp.shape and np.all(kj == 1)
        assert np.all(np.abs(Hj - Hp) <= bound)
        # ... and at the default tolerance
        assert np.all(implicit(pj, c, cg_Pl="jacobi")[1] == 1)


def test_scaled_dense_model_takes_fewer_iterations_with_its_diagonal(M):
    prob, c, Hz = model(M, "scaled", hess_diag="none")
    H0, k0 = implicit(prob, c)
    pj, _, _ = model(M, "scaled")
    H1, k1 = implicit(pj, c, cg_Pl="jacobi")
    print("scaled dense counts: plain", k0.ravel(), "jacobi", k1.ravel())
    assert np.all(k1 > 0) and np.all(k1 < k0)
    Hp, kp = implicit(prob, c, cg_reltol=1e-12)
    Hj, kj = implicit(pj, c, cg_reltol=1e-12, cg_Pl="jacobi")
    bound = h_bound(M, prob, c, Hz, 1e-12, int(max(kp.max(), kj.max())))
    print("at 1e-12: plain", kp.ravel(), "jacobi", kj.ravel(), "max |dH|", float(np.abs(Hj - Hp).max()), "bound", float(bound.min()), "|H|",
          float(np.abs(Hp).max()))
    assert np.all(kj > 0) and np.all(kj < kp) and np.all(kp < 100)
    assert np.all(np.abs(Hj - Hp) <= bound)


def test_one_hot_probes_give_the_callables_diagonal(M):
    """n one-hot probes read the diagonal off n Hessian-vector products: the callable's, to the rounding of a double backward pass
    (sums of m = 40 products: a few m eps relative)."""
    n = SCALED["n"]
    pj, c, Hz = model(M, "scaled")
    pp, _, _ = model(M, "scaled", hess_diag=torch.eye(n, dtype=torch.float64))
    x, z = pj.sample_x_z(M.SimRng(c["seed"], 0), c["theta0"])
    th = pj._theta(c["theta0"])
    zz = z.clone().requires_grad_(True)
    g = torch.autograd.grad(pj._logLike(x, zz, th), zz, create_graph=True)[0]
    hvp = lambda V: -torch.autograd.grad(g, zz, V[0], retain_graph=True)[0][None]
    d_call = pj._hess_diagonal(x[None], z[None], th[None], hvp)
    d_probe = pp._hess_diagonal(x[None], z[None], th[None], hvp)
    assert d_call.shape == d_probe.shape == (1, n)
    np.testing.assert_allclose(d_probe.numpy(), d_call.numpy(), rtol=8 * SCALED["m"] * EPS, atol=0)
    np.testing.assert_allclose(d_call.numpy()[0], np.diag(Hz.numpy()), rtol=8 * SCALED["m"] * EPS, atol=0)
    # the same counts and, at 1e-12, the same H to the bound
    Hj, kj = implicit(pj, c, cg_Pl="jacobi")
    Hq, kq = implicit(pp, c, cg_Pl="jacobi")
    assert np.array_equal(kj, kq)
    # any positive diagonal gives the same H to the tolerance -- here the right one in the wrong order -- and only the counts move
    _, _, hd, _, _ = scaled_dense_closures(M)
    pw = M.TorchMuseProblem(None, pj._sample, pj._logLike, hess_diag=lambda x, z, th: torch.flip(hd(x, z, th), dims=(1,)))
    Hw, kw = implicit(pw, c, cg_reltol=1e-12, cg_Pl="jacobi")
    Hp, kp = implicit(pj, c, cg_reltol=1e-12, cg_Pl="jacobi")
    print("flipped diagonal: counts", kw.ravel(), "against", kp.ravel(), "max |dH|", float(np.abs(Hw - Hp).max()))
    assert np.all(kw > 0) and np.all(kw >= kp)
    assert np.all(np.abs(Hw - Hp) <= h_bound(M, pj, c, Hz, 1e-12, int(max(kw.max(), kp.max()))))


def test_probe_tensors_that_are_no_partition_are_refused(M):
    n = SCALED["n"]
    eye = torch.eye(n, dtype=torch.float64)
    for bad in (eye[:-1], torch.cat([eye, eye[:1]]), 2.0 * eye, 0.5 * torch.ones(2, n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)):
        with pytest.raises(ValueError, match="hess_diag"):
            model(M, "scaled", hess_diag=bad)
    with pytest.raises(ValueError, match="hess_diag"):
        model(M, "scaled", hess_diag="diagonal")
    # a partition of the wrong latent shape is refused where the shape is known
    pw, c, _ = model(M, "scaled", hess_diag=torch.eye(n + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="hess_diag"):
        implicit(pw, c, cg_Pl="jacobi")
    # two probes (even / odd elements) are a partition
    two = torch.stack([eye[0::2].sum(dim=0), eye[1::2].sum(dim=0)])
    pt, c, _ = model(M, "hetero", hess_diag=torch.stack([torch.eye(50, dtype=torch.float64)[0::2].sum(dim=0), torch.eye(50, dtype=torch.float64)[1::2].sum(dim=0)]))
    assert np.all(implicit(pt, c, cg_Pl="jacobi")[1] == 1) and two.shape == (2, n)


def test_jacobi_without_hess_diag_is_refused_before_any_draw(M):
    def no_draw(gen, theta):
        raise AssertionError("the sampler was called")
    _, logLike, _, _ = hetero_closures(HETERO["N"])
    prob = M.TorchMuseProblem(None, no_draw, logLike)
    with pytest.raises(ValueError, match="jacobi") as e:
        prob.implicit_H_batch(0, 0, 2, HETERO["theta0"], cg_Pl="jacobi")
    assert "hess_diag" in str(e.value)
    with pytest.raises(ValueError, match="cg_Pl"):
        M.TorchMuseProblem(None, no_draw, logLike, hess_diag="elementwise").implicit_H_batch(0, 0, 2, HETERO["theta0"], cg_Pl="diagonal")
    # ... and through the driver
    res = M.MuseResult()
    res.theta = HETERO["theta0"]
    with pytest.raises(ValueError, match="jacobi"):
        M.get_H_(res, prob, rng=0, nsims=2, implicit_diff=True, implicit_diff_cg_kwargs={"Pl": "jacobi"})


def test_a_diagonal_that_is_not_positive_is_reported_through_the_count(M):
    sample, logLike, hd, _ = hetero_closures(HETERO["N"])
    prob = M.TorchMuseProblem(None, sample, logLike, hess_diag=lambda x, z, th: -hd(x, z, th))
    Hs, its = implicit(prob, HETERO, cg_Pl="jacobi")
    assert np.all(its == -1)
    res = M.MuseResult()
    res.theta = HETERO["theta0"]
    with pytest.raises(M.MuseError):
        M.get_H_(res, prob, rng=HETERO["seed"], nsims=2, implicit_diff=True, implicit_diff_cg_kwargs={"Pl": "jacobi"})


def test_get_H_records_the_preconditioned_counts(M):
    pj, c, _ = model(M, "scaled")
    _, k1 = prob_counts = pj.implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=1e-1, cg_Pl="jacobi")
    _, k0 = model(M, "scaled", hess_diag="none")[0].implicit_H_batch(c["seed"], 0, c["nsims"], c["theta0"], atol=1e-1)
    res = M.MuseResult()
    res.theta = c["theta0"]
    M.get_H_(res, pj, rng=c["seed"], nsims=c["nsims"], implicit_diff=True, implicit_diff_cg_kwargs={"Pl": "jacobi"})
    hists = np.array(res.metadata["implicit_diff_cg_hists"])
    print("get_H_ counts", hists.ravel(), "plain", k0.ravel())
    assert np.array_equal(hists, k1) and np.all(hists < k0)
    np.testing.assert_array_equal(res.H, prob_counts[0].mean(axis=0))
