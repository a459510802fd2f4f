"""libmuse_lbfgs.so's lock-step conjugate gradients on the GPU, through simple.CgBatch: the operators of tests/test_cg_control.py applied
with torch on the device, against simple._cg on the host (reltol sqrt(eps), maxiter 100).  Sizes: the strided passes' edges (1, 5, one
below and one above the 256 threads) and the switch between the 256- and the 1024-thread kernels (4096 / 4097)."""
import math

import numpy as np
import pytest
import torch

from museinference_jl_amd import simple

DEV = "cuda"
RELTOL = math.sqrt(np.finfo(np.float64).eps)
NS = (1, 5, 255, 257, 4096, 4097)
INDEFINITE, ZERO = 6, 5


def mixed_batch(n):
    """7 rows: diagonal M with k = 1 .. 5 distinct values 1 + 0.75 (i mod k), a row with b = 0, and a row whose M is negative definite.
    Returns (D [7, n]: the diagonals, b [7, n]) on the host."""
    i = np.arange(n)
    D = np.stack([1.0 + 0.75 * (i % k) for k in (1, 2, 3, 4, 5)] + [1.0 + 0.75 * (i % 2), -1.0 - 0.5 * (i % 2)])
    b = np.random.RandomState(11).randn(7, n)
    b[ZERO] = 0.0
    return torch.as_tensor(D), torch.as_tensor(b)


def run(D, b, maxiter=100, abstol=0.0, keep_p=False):
    """Drive CgBatch with M = diag(D) applied on the device.  Returns y, counts, resnorm, the active word per round, p_eval per round."""
    D, b = D.to(DEV), b.to(DEV)
    cg = simple.CgBatch(DEV, b.shape[0], b.shape[1])
    actives, ps = [cg.begin(b, RELTOL, abstol, maxiter)], []
    ps.append(cg.p_eval.clone())
    while actives[-1] > 0:
        actives.append(cg.advance(D * cg.p_eval))
        if keep_p:
            ps.append(cg.p_eval.clone())
        assert cg.rounds <= maxiter
    y, its, res = cg.result()
    assert cg.syncs == cg.rounds + 2          # begin's word, one per round, the result
    return y.cpu(), its, res, actives, ps, cg.rounds


_reference = {}


def host_reference(n):
    """simple._cg on the host, row by row (computed once per size): counts and true residuals"""
    if n not in _reference:
        D, b = mixed_batch(n)
        out = []
        for r in range(7):
            if r == INDEFINITE:
                out.append((None, None))
                continue
            y, k = simple._cg(lambda p: D[r] * p, b[r], 100, RELTOL)
            out.append((k, float(torch.linalg.norm(b[r] - D[r] * y))))
        _reference[n] = out
    return _reference[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_mixed_batch_equals_cg_on_the_host(gpu, n):
    D, b = mixed_batch(n)
    y, its, res, actives, ps, rounds = run(D, b, keep_p=True)
    ref = host_reference(n)
    finished_at = {}
    for r in range(7):
        if r == INDEFINITE:
            assert its[r] == -1 and torch.all(y[r] == 0.0)        # p.Mp < 0 in the first round: -1 - 0, y as it was
            finished_at[r] = 1
            continue
        k, ref_res = ref[r]
        tol = RELTOL * float(torch.linalg.norm(b[r]))
        true_res = float(torch.linalg.norm(b[r] - D[r] * y[r]))
        print("n", n, "row", r, "count", int(its[r]), "_cg", k, "true residual", true_res, "_cg", ref_res, "tol", tol, "recurrence", float(res[r]))
        assert its[r] == k == (0 if r == ZERO else min(r + 1, n)), (r, its, k)      # one iteration per distinct value
        assert true_res <= max(tol, 2.0 * ref_res)
        assert res[r] <= tol
        finished_at[r] = k
    assert torch.all(y[ZERO] == 0.0)
    # the word: begin reports every row but the zero one; then it only falls, to 0; as many rounds as the largest count
    assert actives[0] == 6 and actives[-1] == 0 and all(a >= c for a, c in zip(actives, actives[1:]))
    assert rounds == int(its.max()) == len(actives) - 1
    # a finished row's direction stays where it was, bit for bit, from the round it finished to the last (and is finite)
    for r, k in finished_at.items():
        for p in ps[k + 1:]:
            assert torch.equal(p[r], ps[k][r])
        assert torch.all(torch.isfinite(ps[-1][r]))
    # the neighbours of the indefinite row: the same batch without it gives the same bits
    y6, its6, res6, *_ = run(D[:6], b[:6])
    assert torch.equal(y6, y[:6]) and np.array_equal(its6, its[:6]) and np.array_equal(res6, res[:6])
    # ... and row 3 of 7 alone, as a batch of 1
    y1, its1, res1, *_ = run(D[3:4], b[3:4])
    assert np.array_equal(y1[0].numpy(), y[3].numpy()) and its1[0] == its[3] and res1[0] == res[3]


@pytest.mark.gpu
@pytest.mark.parametrize("n,s,expected", [(33, 1.0, 17), (257, 1.0, 20), (257, 0.25, 37)])
def test_periodic_operator_counts(gpu, n, s, expected):
    """(2 + s) p_i - p_{i-1} - p_{i+1}, periodic, with test_cg_control.py's right-hand side; a second row with abstol's and maxiter's
    effect checked on the same operator"""
    b = torch.as_tensor(np.random.RandomState(1).randn(4097)[:n].copy()).reshape(1, n)
    op = lambda p: (2.0 + s) * p - torch.roll(p, 1, dims=-1) - torch.roll(p, -1, dims=-1)

    def drive(maxiter, abstol):
        cg = simple.CgBatch(DEV, 1, n)
        active = cg.begin(b.to(DEV), RELTOL, abstol, maxiter)
        while active > 0:
            active = cg.advance(op(cg.p_eval))
        y, its, res = cg.result()
        return y.cpu(), int(its[0]), float(res[0]), cg.rounds
    y, k, res, rounds = drive(100, 0.0)
    yh, kh = simple._cg(lambda p: op(p), b[0], 100, RELTOL)
    tol = RELTOL * float(torch.linalg.norm(b))
    true_res, ref_res = float(torch.linalg.norm(b[0] - op(y[0]))), float(torch.linalg.norm(b[0] - op(yh)))
    print("n", n, "s", s, "count", k, "_cg", kh, "true residual", true_res, "_cg", ref_res, "tol", tol)
    assert k == kh == expected == rounds
    assert true_res <= max(tol, 2.0 * ref_res)
    assert drive(3, 0.0)[1] == 3
    y0, k0, _, rounds0 = drive(0, 0.0)
    assert k0 == 0 and rounds0 == 0 and torch.all(y0 == 0.0)
    ya, ka, resa, _ = drive(100, 1e-4)
    assert 1e-4 > tol and 0 < ka < k and resa <= 1e-4


@pytest.mark.gpu
def test_nan_operator_and_refusals(gpu):
    b = torch.as_tensor(np.random.RandomState(2).randn(2, 5)).to(DEV)
    cg = simple.CgBatch(DEV, 2, 5)
    assert cg.begin(b, RELTOL, 0.0, 100) == 2
    assert cg.advance(torch.full_like(b, math.nan)) == 0
    y, its, _ = cg.result()
    assert np.all(its < 0) and torch.all(y == 0.0)
    with pytest.raises(ValueError):
        cg.begin(b[:1], RELTOL, 0.0, 100)
    with pytest.raises(ValueError):
        cg.advance(cg.p_eval)
