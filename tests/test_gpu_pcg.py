"""simple.CgBatch with a diagonal (libmuse_lbfgs.so's muse_lbfgs_pcg_*) on the GPU: the cases of tests/test_pcg_control.py as ONE batch per
n in (5, 257, 4097) -- both workgroup sizes -- against simple._pcg on the CPU: equal counts, the true residual within the CPU test's
bound; a row alone and inside the batch bit for bit; rows_per_diag; guard rows and their neighbours; rounds and synchronisations; and a
CgBatch used with a diagonal and then without."""
import numpy as np
import pytest
import torch

from museinference_jl_amd import simple
from test_cg_control import MASTER, RELTOL
from test_pcg_control import SCALED_COUNTS, WEIGHTS

DEV = "cuda"
NS = (5, 257, 4097)


def t(a, device):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(device)


def scaled(n, device):
    w = t(WEIGHTS[:n], device)

    def M(p):
        q = w * p
        return w * (3.0 * q - torch.roll(q, 1) - torch.roll(q, -1))
    return M, 3.0 * (w * w)


def diagonal(n, k, device):
    d = t(1.0 + 0.75 * (np.arange(n) % k), device)
    return (lambda p: d * p), d


def periodic(s):
    return lambda p: (2.0 + s) * p - torch.roll(p, 1) - torch.roll(p, -1)


def rows_of(n, device):
    """[(name, operator, diagonal, right-hand side, expected count or None, guard row?)] for one batch of row length n"""
    b = t(MASTER[:n], device)
    one = torch.ones(n, dtype=torch.float64, device=device)
    M, d = scaled(n, device)
    rows = [("scaled", M, d, b, SCALED_COUNTS[n], False)]
    for k in (1, 2, 3, 5):
        Mk, dk = diagonal(n, k, device)
        rows.append((f"diag_k{k}", Mk, dk, b, 1, False))
        rows.append((f"unit_diag_k{k}", Mk, one, b, min(k, n), False))
    rows.append(("unit_periodic_s1", periodic(1.0), one, b, None, False))
    rows.append(("unit_periodic_s025", periodic(0.25), one, b, None, False))
    rows.append(("scaled_other_rhs", M, d, torch.flip(b, dims=(0,)) * 3.0, None, False))
    rows.append(("zero_rhs", M, d, torch.zeros_like(b), 0, False))
    for kind, bad in (("zero", 0.0), ("negative", -1.0), ("infinite", float("inf")), ("nan", float("nan"))):
        dd = d.clone()
        dd[n // 2] = bad
        rows.append(("bad_diag_" + kind, M, dd, b, -1, True))
    sign, two = -one.clone(), 2.0 * one
    sign[0], two[0] = 1.0, 1.0
    rows.append(("indefinite", lambda p: sign * p, one, two, -1, True))       # M = diag(1, -1, ...), b = (1, 2, ...): p.Mp = 1 - 4 (n - 1)
    rows.append(("negative_definite", lambda p: -p, one, b, -1, True))
    rows.append(("nan_operator", lambda p: p * float("nan"), one, b, -1, True))
    return rows


def run_batch(rows, device, reltol=RELTOL, abstol=0.0, maxiter=100, cg=None, use_diag=True, rows_per_diag=1, diag=None):
    n = rows[0][3].numel()
    cg = cg or simple.CgBatch(device, len(rows), n)
    B = torch.stack([r[3] for r in rows])
    if use_diag:
        D = torch.stack([r[2] for r in rows]) if diag is None else diag
        active = cg.begin(B, reltol, abstol, maxiter, diag=D, rows_per_diag=rows_per_diag)
    else:
        active = cg.begin(B, reltol, abstol, maxiter)
    while active > 0:
        Mp = torch.stack([r[1](cg.p_eval[i]) for i, r in enumerate(rows)])
        active = cg.advance(Mp)
        assert cg.rounds <= maxiter + 1
    y, its, res = cg.result()
    return y, its, res, cg.rounds, cg.syncs


_batches = {}


def batch(n):
    """One batch per n, run once: (rows, y, counts, |r|, rounds, syncs)"""
    if n not in _batches:
        rows = rows_of(n, DEV)
        _batches[n] = (rows,) + run_batch(rows, DEV)
    return _batches[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_counts_and_residuals_equal_simple_pcg(gpu, n):
    rows, y, its, res, rounds, syncs = batch(n)
    cpu_rows = rows_of(n, "cpu")
    for i, ((name, M, d, b, expected, guard), (_, Mc, dc, bc, _, _)) in enumerate(zip(rows, cpu_rows)):
        yc, k = simple._pcg(Mc, bc, dc, 100, RELTOL)
        true_res = float(torch.linalg.norm(b - M(y[i]))) if not guard else float("nan")
        ref_res = float(torch.linalg.norm(bc - Mc(yc))) if not guard else float("nan")
        bnorm = float(torch.linalg.norm(bc))
        print(n, name, "count", int(its[i]), "_pcg", k, "true residual", true_res, "_pcg", ref_res, "tol", RELTOL * bnorm)
        assert its[i] == k, (name, its[i], k)
        if expected is not None:
            assert its[i] == expected, (name, its[i], expected)
        if guard:
            assert its[i] < 0 and float(y[i].abs().max()) == 0.0, name
        else:
            assert true_res <= max(RELTOL * bnorm, 2.0 * ref_res), (name, true_res, ref_res)
            assert res[i] <= RELTOL * bnorm
    # a bad diagonal ends its row in begin, the indefinite operators in the first round: the rounds are the largest count's
    assert rounds == its.max() and syncs == rounds + 2


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_a_row_alone_and_in_the_batch_agree_bit_for_bit(gpu, n):
    rows, y, its, _, _, _ = batch(n)
    for i in (0, 5, 11):          # scaled, a diagonal case, the scaled operator with another right-hand side
        y1, k1, _, _, _ = run_batch([rows[i]], DEV)
        assert k1[0] == its[i] and torch.equal(y1[0], y[i]), rows[i][0]
    # ... and the guard rows change nothing for their neighbours: the same bits in a batch without them
    good = [i for i, r in enumerate(rows) if not r[5]]
    yg, kg, _, _, _ = run_batch([rows[i] for i in good], DEV)
    assert np.array_equal(kg, its[good]) and torch.equal(yg, y[good])


@pytest.mark.gpu
@pytest.mark.parametrize("n", (5, 4097))
def test_rows_per_diag_equals_the_repeated_diagonal(gpu, n):
    b = t(MASTER[:n], DEV)
    M, d = scaled(n, DEV)
    Mk, dk = diagonal(n, 3, DEV)
    rows = [("a", M, d, b, None, False), ("b", M, d, torch.flip(b, dims=(0,)), None, False), ("c", M, d, b * b, None, False),
            ("d", Mk, dk, b, None, False), ("e", Mk, dk, torch.flip(b, dims=(0,)), None, False), ("f", Mk, dk, b * b, None, False)]
    y1, k1, r1, _, _ = run_batch(rows, DEV)
    y3, k3, r3, _, _ = run_batch(rows, DEV, rows_per_diag=3, diag=torch.stack([d, dk]))
    assert np.array_equal(k1, k3) and torch.equal(y1, y3) and np.array_equal(r1, r3)
    assert np.all(k1[3:] == 1) and np.all(k1[:3] > 1)
    cg = simple.CgBatch(DEV, 6, n)
    for bad in (dict(rows_per_diag=4), dict(rows_per_diag=0), dict(rows_per_diag=3, diag=torch.stack([d, dk, d]))):
        with pytest.raises(ValueError):
            cg.begin(torch.stack([r[3] for r in rows]), RELTOL, diag=bad.get("diag", torch.stack([d, dk])), rows_per_diag=bad["rows_per_diag"])


@pytest.mark.gpu
def test_maxiter_and_abstol(gpu):
    n = 257
    M, d = scaled(n, DEV)
    Mc, dc = scaled(n, "cpu")
    b, bc = t(MASTER[:n], DEV), t(MASTER[:n], "cpu")
    rows = [("scaled", M, d, b, None, False)]
    for kw in (dict(maxiter=0), dict(maxiter=3), dict(abstol=1e-4)):
        y, its, res, rounds, syncs = run_batch(rows, DEV, **kw)
        yc, k = simple._pcg(Mc, bc, dc, kw.get("maxiter", 100), RELTOL, kw.get("abstol", 0.0))
        assert its[0] == k and rounds == k and syncs == rounds + 2, (kw, its, k)
        np.testing.assert_allclose(y[0].cpu().numpy(), yc.numpy(), rtol=0, atol=1e-9 * float(yc.abs().max()) if k else 0.0)
    assert 0 < k < SCALED_COUNTS[n] and res[0] <= 1e-4


@pytest.mark.gpu
def test_a_batch_used_with_a_diagonal_and_then_without_gives_the_plain_bits(gpu):
    n = 257
    rows = [r for r in rows_of(n, DEV) if not r[5]]
    cg = simple.CgBatch(DEV, len(rows), n)
    run_batch(rows, DEV, cg=cg)
    y_after, k_after, r_after, rounds, syncs = run_batch(rows, DEV, cg=cg, use_diag=False)
    y_fresh, k_fresh, r_fresh, _, _ = run_batch(rows, DEV, use_diag=False)
    assert torch.equal(y_after, y_fresh) and np.array_equal(k_after, k_fresh) and np.array_equal(r_after, r_fresh)
    assert k_fresh[0] == 100 and rounds == 100       # the scaled row: plain CG stops at maxiter
