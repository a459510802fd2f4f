"""libmuse_lbfgs.so at its C ABI on the GPU (through simple.LbfgsBatch, a thin wrapper of the four entry points) against optim.lbfgs on
CPU torch.  The objective is evaluated in numpy on the HOST for both sides, so both see identical f and g for identical z:

    f = 1/2 sum (x - h(z))^2 + 1/2 sum iv_i z_i^2,   h(v) = v + 0.1 v^3,   iv = e^{-theta_k} over ntheta contiguous blocks
    RandomState(17 + N):  z = e^{theta_k / 2} randn(N)  first, then  x = h(z) + randn(N)

N in {1, 2, 63, 255, 256, 257, 1001, 5000} x {(theta [0.4, -0.3] ([0.4] at N = 1), tol 1e-6), (theta [1.0], tol 1e-2)} x start {zero, true z}:
the workgroup size (256) +- 1, odd lengths (rows only 8-byte aligned), several strides per thread, the second workgroup size (N = 5000),
18-51 iterations (the history of 10 wraps), about three evaluations per iteration.  Per problem status, iterations and f_calls are
EQUAL to optim.lbfgs's, the minimiser within 1e-9 and f_min within rtol 1e-11 (the project's same-path tolerances).  These cases'
paths do not depend on the order of summation (optim.lbfgs gives the same counts on them under permuted element orders)."""
import numpy as np
import pytest
import torch

from museinference_jl_amd import optim

NS = (1, 2, 63, 255, 256, 257, 1001, 5000)
CONFIGS = {"two_blocks_1e-6": ([0.4, -0.3], 1e-6), "one_block_1e-2": ([1.0], 1e-2)}
h = lambda v: v + 0.1 * v ** 3


def draw(N, theta):
    th = np.asarray(theta if N > 1 else theta[:1], dtype=np.float64)
    k = (np.arange(N) * th.size) // N
    rs = np.random.RandomState(17 + N)
    z = np.exp(th[k] / 2) * rs.randn(N)
    x = h(z) + rs.randn(N)
    return x, z, np.exp(-th[k])


def objective(x, iv, z):
    """rows of z [B, N] (x, iv [B, N]) -> f [B], g [B, N]"""
    r = x - h(z)
    return 0.5 * np.sum(r * r, axis=-1) + 0.5 * np.sum(iv * z * z, axis=-1), -r * (1 + 0.3 * z * z) + iv * z


def solve_on_gpu(M, x, iv, z0, tol, keep_points=False):
    """x, iv, z0: [B, N] numpy.  Returns (zhat [B, N], info [B], the evaluation points of every round if asked for)."""
    dev = torch.device("cuda")
    batch = M.LbfgsBatch(dev, *z0.shape)
    batch.begin(torch.as_tensor(z0, device=dev), tol)
    points = []
    while True:
        z = batch.z_eval.cpu().numpy()
        if keep_points:
            points.append(z.copy())
        with np.errstate(all="ignore"):
            f, g = objective(x, iv, z)
        if batch.advance(torch.as_tensor(f, device=dev), torch.as_tensor(g, device=dev)) == 0:
            break
        assert batch.rounds < 5000
    if keep_points:
        points.append(batch.z_eval.cpu().numpy().copy())
    zhat, info = batch.result()
    return zhat.cpu().numpy(), info, points


def solve_on_cpu(x, iv, z0, tol):
    def fg(z):
        f, g = objective(x, iv, z.numpy())
        return float(f), torch.from_numpy(g)
    z, info = optim.lbfgs(fg, torch.from_numpy(z0.copy()), tol)
    return z.numpy(), info


_cache = {}


def both(M, N, config):
    """One batch of two problems (zero start, true-z start) per (N, config), and optim.lbfgs on each: computed once."""
    if (N, config) not in _cache:
        theta, tol = CONFIGS[config]
        x, ztrue, iv = draw(N, theta)
        z0 = np.stack([np.zeros(N), ztrue])
        X, IV = np.stack([x, x]), np.stack([iv, iv])
        zg, info, _ = solve_on_gpu(M, X, IV, z0, tol)
        _cache[(N, config)] = (zg, info, [solve_on_cpu(x, iv, z0[b], tol) for b in range(2)])
    return _cache[(N, config)]


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["zero", "true"])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("N", NS)
def test_counts_equal_optim_lbfgs(M, gpu, N, config, start):
    zg, info, ref = both(M, N, config)
    b = 0 if start == "zero" else 1
    zc, ic = ref[b]
    got = (int(info["status"][b]), int(info["iterations"][b]), int(info["f_calls"][b]))
    print(N, config, start, "gpu", got, "cpu", (ic["status"], ic["iterations"], ic["f_calls"]), "max |dz|", np.abs(zg[b] - zc).max(),
          "rel df", abs(info["f_min"][b] - ic["f_min"]) / abs(ic["f_min"]))
    assert got == (ic["status"], ic["iterations"], ic["f_calls"])
    assert int(info["hist_words"][b]) == 0
    np.testing.assert_allclose(zg[b], zc, rtol=0, atol=1e-9)
    np.testing.assert_allclose(info["f_min"][b], ic["f_min"], rtol=1e-11)
    assert info["gnorm"][b] <= CONFIGS[config][1]


@pytest.mark.gpu
@pytest.mark.parametrize("N", [257, 5000])
def test_a_problem_does_not_depend_on_its_batch(M, gpu, N):
    """One problem alone, and the same problem as row 3 of a batch of 7 different problems -- one of them converged at the start, one not
    finite, so the rows finish in different rounds: the same bits, the same record, and a finished row's evaluation point stays put."""
    theta, tol = CONFIGS["two_blocks_1e-6"]
    x, ztrue, iv = draw(N, theta)
    rs = np.random.RandomState(5)
    X = np.stack([x + 0.3 * rs.randn(N) for _ in range(7)])
    IV = np.stack([iv * np.exp(0.2 * rs.randn()) for _ in range(7)])
    Z0 = np.stack([0.5 * rs.randn(N) for _ in range(7)])
    X[3], IV[3], Z0[3] = x, iv, np.zeros(N)
    X[1], Z0[1] = 0.0, 0.0                      # the minimum itself: converged at the start
    X[5, N // 2] = np.nan                       # not finite
    z1, info1, _ = solve_on_gpu(M, X[3:4], IV[3:4], Z0[3:4], tol)
    z7, info7, points = solve_on_gpu(M, X, IV, Z0, tol, keep_points=True)
    assert np.array_equal(z1[0], z7[3])
    assert info1[0] == info7[3]
    assert (info7["status"][1], info7["iterations"][1], info7["f_calls"][1]) == (optim.STATUS_G_CONVERGED, 0, 1)
    assert (info7["status"][5], info7["iterations"][5], info7["f_calls"][5]) == (optim.STATUS_NONFINITE, 0, 1)
    assert len(set(int(c) for c in info7["f_calls"])) >= 4          # the rows finish in different rounds
    for b in range(7):
        # row b was evaluated f_calls[b] times: points[f_calls[b] - 1] is its last evaluation point, and it never moves again
        last = int(info7["f_calls"][b]) - 1
        for later in points[last + 1:]:
            assert np.array_equal(later[b], points[last][b], equal_nan=True), b
        if b != 5:
            assert np.array_equal(points[-1][b], z7[b]), b
    # the other rows are minimised too (their paths are not pinned: only the committed cases above were checked for that)
    for b in (0, 2, 4, 6):
        assert info7["status"][b] == optim.STATUS_G_CONVERGED
        assert np.abs(objective(X[b], IV[b], z7[b])[1]).max() <= tol


@pytest.mark.gpu
def test_bad_arguments_are_refused(M, gpu):
    from museinference_jl_amd import _capi
    lib = _capi.load_lbfgs_library()
    assert lib.muse_lbfgs_workspace_bytes(0, 5, 10) < 0 and lib.muse_lbfgs_workspace_bytes(2, 0, 10) < 0
    batch = M.LbfgsBatch("cuda", 2, 5)
    with pytest.raises(ValueError):
        batch.begin(torch.zeros((2, 4), dtype=torch.float64, device="cuda"), 1e-6)
    assert lib.muse_lbfgs_advance(None, 2, 5, 10, None, None, None, None, None) == -1
