"""The cases tests/test_gpu_link.py and tests/test_link_reference.py share (no GPU, no package import at module level): the twins'
ramp and mask, the link, and the harder case in which the stencil kernels' HagerZhang brackets and bisects -- with the fp64 numpy
objective optim.lbfgs runs it on, its sums formed pairwise or sequentially."""
import math

import numpy as np

import hp_reference as R
import link_reference as L
import stencil_reference as S

ATOL = 1e-8
LINK = (0.25, 0.5)          # monotone (a2^2 < 3 a3); phi' between ~0.96 and ~1.7 over the draws' range at theta ~ -4
HARD_LINK = (0.4, 0.3)      # monotone; at theta ~ 0, |u| reaches ~2: phi' from ~0.87 to ~4, the objective far from quadratic
# (N, theta, stencil, seed of the data draw): the harder case with both stencils and two data vectors each.  Kept are draws whose
# solve reaches atol = 1e-8 with the same (iterations, f_calls) in EVERY summation order of ORDERS below (tests/test_link_reference.py
# checks exactly that), and with f moved by up to JITTER_ULPS ulps and every component of g by up to one, at random (JITTERS
# streams): the kernels' own order -- a thread's fma chain, then a tree -- is none of the listed ones, and a sum of 301 terms formed
# in any order errs by a few ulps.  (With one ulp and 8 streams the builtin stencil's seed 112 still passed; the kernels' order
# stalled it one iteration before the host's last, and 2 of 24 streams at four ulps do the same: replaced by 147.)  Of the seeds
# 60 .. 259 three per stencil pass the listed orders: most
# solves stall at the resolution of f ~ 150 in one order or another -- |g| ~ 5e-8 moves f by less than an ulp, status F_CONVERGED --
# and their counts then follow the order of the sums (numpy's own np.sum differs between two CPUs); those draws were replaced.
HARD = [{"N": 301, "theta": [0.0], "w": w, "seed": seed, "link": HARD_LINK}
        for w, seeds in ((None, (91, 147)), ((0.3, 0.35), (104, 138))) for seed in seeds]
JITTERS, JITTER_ULPS = 24, 4


def _lanes(width):
    """The sum as `width` interleaved accumulators would form it (a vector unit's lanes), then those in sequence."""
    def total(v):
        rows = np.concatenate([v, np.zeros((-v.size) % width)]).reshape(-1, width)
        acc = np.zeros(width)
        for row in rows:
            acc = acc + row
        return float(np.cumsum(acc)[-1])
    return total


# the orders in which the objective's sum is formed ("exact" is the correctly rounded sum: the same on every machine, and what the
# GPU test's host solve uses)
ORDERS = {
    "exact": lambda v: math.fsum(v),
    "sequential": lambda v: float(np.cumsum(v)[-1]),
    "reversed": lambda v: float(np.cumsum(v[::-1])[-1]),
    "lanes4": _lanes(4), "lanes8": _lanes(8), "lanes16": _lanes(16),
    "pairwise": lambda v: float(np.sum(v)),
}


def ramp_and_mask(N, marked):
    """The twins' noise: sd a ramp in [0.5, 2], a mask of about 5 % of the elements among them `marked`."""
    sd = np.linspace(0.5, 2.0, N)
    mask = np.ones(N, bool)
    mask[marked] = False
    rest = np.setdiff1d(np.arange(N), marked)
    mask[np.random.default_rng(N).choice(rest, size=N // 20 - len(marked), replace=False)] = False
    return sd, mask


def hard_marked(N):
    return [0, N - 1, 2 * 64, 2 * 127 + 1]


def hard_data(case):
    """(x fp64, sd, mask, omega, s, w): the data of a harder case, drawn by the reference at the case's theta."""
    N, w = case["N"], S.BUILTIN if case["w"] is None else case["w"]
    sd, mask = ramp_and_mask(N, hard_marked(N))
    om, s = L.weights(N, sd, mask)
    x = L.sample_x_z(N, case["seed"], 0, case["theta"], w, s, case["link"])[0].astype(np.float64)
    return x, sd, mask, om, s, w


def numpy_objective(x, theta, w, om, link, total):
    """fg(z) -> (f, grad) in fp64 numpy, the model's definition with the sums formed by `total`."""
    import torch
    N = x.size
    th = np.asarray(theta, np.float64)
    k = R.blocks(N, th.size)
    iv = np.exp(-th)[k]
    cst = float(np.sum(R.block_sizes(N, th.size) * th))
    omf = np.asarray(om, np.float64)
    xf = np.where(omf != 0, x, 0.0)
    w0, w1 = float(w[0]), float(w[1])
    a2, a3 = (0.0, 0.0) if link is None else link
    A = lambda v: w1 * (np.roll(v, 1) + np.roll(v, -1)) + w0 * v

    def fg(zt):
        z = zt.numpy()
        u = A(z)
        r = xf - (u + u * u * (a2 + a3 * u))
        q = omf * r
        f = 0.5 * (total(q * r + iv * z * z) + cst)
        g = iv * z - A(q * (1.0 + u * (2.0 * a2 + 3.0 * a3 * u)))
        return f, torch.from_numpy(g)
    return fg


def _jittered(fg, stream):
    """fg with its value moved by up to JITTER_ULPS and every component of its gradient by up to one unit of 2^-53 relative, at
    random."""
    import torch
    rng = np.random.default_rng(1000 + stream)

    def out(z):
        f, g = fg(z)
        g = g.numpy() * (1.0 + rng.integers(-1, 2, g.numel()) * 2.0 ** -53)
        return f * (1.0 + int(rng.integers(-JITTER_ULPS, JITTER_ULPS + 1)) * 2.0 ** -53), torch.from_numpy(g)
    return out


def hard_problem(case):
    """(x, {order: fg with the sums formed so, and the exact one jittered}, fg of the same data without the link)."""
    x, sd, mask, om, s, w = hard_data(case)
    fgs = {name: numpy_objective(x, case["theta"], w, om, case["link"], total) for name, total in ORDERS.items()}
    for k in range(JITTERS):
        fgs["jitter%d" % k] = _jittered(fgs["exact"], k)
    return x, fgs, numpy_objective(x, case["theta"], w, om, None, ORDERS["exact"])


def lbfgs(M, fg, N, atol):
    import torch
    from museinference_jl_amd import optim
    return optim.lbfgs(fg, torch.zeros(N, dtype=torch.float64), atol)
