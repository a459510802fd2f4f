"""A numpy-longdouble restatement of the conjugate-gradient loop behind MUSE_IMPLICIT_PL_JACOBI (include/muse_hip.h) for a DIAGONAL
Hessian: IterativeSolvers' preconditioned iterable, restated from its published algorithm.  It imports neither the package nor the
oracle; the operands (the model's diagonal d = diag(A) < 0 and the right-hand side b) come from the caller -- tests/hp_reference.py
and tests/pair_implicit_reference.py have them in longdouble.

From x = 0, r = b, u = 0, rho = 1 an iteration is

    c = Pl \\ r;  rho' = rho, rho = c.r, beta = rho / rho';  u = c + beta u;  c = A u;  alpha = rho / (u.c);  x += alpha u;  r -= alpha c

and the loop stops at |r|_2 <= max(reltol |b|_2, abstol) -- the true residual -- or after maxiter iterations.  Pl = Diagonal(d) with
`jacobi`, else the identity (the recurrence is then plain CG).  Where d_i = 0 the preconditioner leaves c_i = 0, as the kernel's
select does for its phantom slots (a header that says ozz = 0 on a real element: include/muse_model.h).

Because A is diagonal the exact solve is b / d: solve() returns the loop's x, the exact one and the iteration count.
"""
import numpy as np

LD = np.longdouble
RELTOL_DEFAULT = float(np.sqrt(np.finfo(np.float64).eps))


def apply_pl(r, d):
    """c = Diagonal(d) \\ r with c_i = 0 where d_i = 0."""
    ok = d != 0
    return np.where(ok, r / np.where(ok, d, LD(1)), LD(0))


def solve(d, b, *, jacobi=True, maxiter=100, reltol=RELTOL_DEFAULT, abstol=0.0):
    """(x_cg, x_exact, iterations) for A = Diagonal(d); x_exact_i = b_i / d_i (0 where d_i = 0)."""
    d = np.asarray(d).astype(LD)
    b = np.asarray(b).astype(LD)
    assert d.shape == b.shape and d.ndim == 1
    x, r, u, rho = np.zeros_like(b), b.copy(), np.zeros_like(b), LD(1)
    tol = max(LD(reltol) * np.sqrt(np.sum(b * b)), LD(abstol))
    it = 0
    while it < maxiter and not np.sqrt(np.sum(r * r)) <= tol:
        c = apply_pl(r, d) if jacobi else r
        rho_prev, rho = rho, np.sum(c * r)
        u = c + (rho / rho_prev) * u
        c = d * u
        alpha = rho / np.sum(u * c)
        x = x + alpha * u
        r = r - alpha * c
        it += 1
    return x, apply_pl(b, d), it
