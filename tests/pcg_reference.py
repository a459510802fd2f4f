"""A numpy-longdouble restatement of diagonally preconditioned conjugate gradients for a GENERAL operator: IterativeSolvers' cg with
Pl = Diagonal(d), restated from its published algorithm and unrolled the way libmuse_lbfgs.so's muse_lbfgs_pcg_* takes it (the operator
applied between two rounds).  It imports nothing from the package.

    begin   y = 0, r = b, rr = b.b, rho = (b/d).b, tol = max(reltol |b|, abstol), p = b/d;  |b| <= tol or maxiter <= 0: count 0
    round   alpha = rho / (p.Mp) -- p.Mp not positive or not finite: count -1 - iterations, y as it was;  y += alpha p;  r -= alpha Mp;
            rr = r.r, rho' = (r/d).r;  count += 1;  stop at sqrt(rr) <= tol or count == maxiter;  p = r/d + (rho'/rho) p
    A diagonal with an entry that is not positive or not finite: count -1, y = 0 (unless the row needs no iteration: count 0).

solve() returns (y, count, history): history[k] = sqrt(rr) / tol after k iterations (history[0] = |b| / tol).
"""
import numpy as np

LD = np.longdouble
RELTOL_DEFAULT = float(np.sqrt(np.finfo(np.float64).eps))


def solve(M, b, d, *, maxiter=100, reltol=RELTOL_DEFAULT, abstol=0.0):
    """M: a function of a longdouble vector.  b, d: arrays (taken to longdouble)."""
    b = np.asarray(b).astype(LD)
    d = np.asarray(d).astype(LD)
    assert b.shape == d.shape and b.ndim == 1
    y, r = np.zeros_like(b), b.copy()
    rr = np.sum(b * b)
    tol = max(LD(reltol) * np.sqrt(rr), LD(abstol))
    history = [float(np.sqrt(rr) / tol) if tol > 0 else float("inf")]
    if maxiter <= 0 or np.sqrt(rr) <= tol:
        return y, 0, history
    if not np.all((d > 0) & np.isfinite(d)):
        return y, -1, history
    p = r / d
    rho = np.sum(p * r)
    count = 0
    while True:
        Mp = M(p)
        pMp = np.sum(p * Mp)
        if not (pMp > 0) or not np.isfinite(pMp):
            return y, -1 - count, history
        alpha = rho / pMp
        y = y + alpha * p
        r = r - alpha * Mp
        c = r / d
        rr, rho_new = np.sum(r * r), np.sum(c * r)
        count += 1
        history.append(float(np.sqrt(rr) / tol))
        if count == maxiter or np.sqrt(rr) <= tol:
            return y, count, history
        p = c + (rho_new / rho) * p
        rho = rho_new
