// pcg_control.hpp -- the SCALAR decisions of the diagonally (Jacobi) preconditioned lock-step conjugate gradients of libmuse_lbfgs.so
// (include/muse_lbfgs.h, muse_lbfgs_pcg_*), beside cg_control.hpp and in its style: written once for the host
// (tests/native/pcg_driver.cpp) and for the device (pcg_kernels.hpp); dot products come in, "stopped" / "finished" / alpha / beta go out.
//
// The order is that of IterativeSolvers' preconditioned iterable (tests/jacobi_reference.py, csrc/solver.hpp's jacobi_cg), unrolled for
// reverse communication.  With d the diagonal and c = r / d elementwise:
//   begin   y = 0, r = b, rr = b . b, rho = (b / d) . b, tol = max(reltol |b|, abstol), p = b / d
//   round   alpha = rho / (p . Mp) behind cg_step_length's guard;  y += alpha p, r -= alpha Mp;  rr' = r . r and rho' = (r / d) . r;
//           count += 1;  stop at sqrt(rr') <= tol or count == maxiter;  else beta = rho' / rho, p = r / d + beta p
// The stopping rule looks at |r|_2, not at rho: the same rule as plain CG, whatever the diagonal.  With d = 1 every value is plain CG's.
// The record is cg_control.hpp's (count, done and rr where the count and result kernels read them) with rho in its last field.
#pragma once
#include "cg_control.hpp"

namespace muse_lbfgs {

// one entry of the diagonal: Pl must be positive definite, as M must be
CG_HD bool pcg_bad_entry(double d) { return !(d > 0.0) || cg_is_inf(d); }

// begin: rr = b . b, rho = (b / d) . b, bad_diagonal = some entry of the row's diagonal is not positive or not finite.  Returns true
// while the row is active.  A row that needs no iteration (b = 0 or within the tolerance, maxiter <= 0) is finished with count 0 as in
// plain CG, its diagonal never used; any other row with a bad diagonal is stopped by the guard before its first iteration: count -1.
CG_HD bool pcg_init(CgRecord& c, double rr, double rho, bool bad_diagonal, double reltol, double abstol, int maxiter) {
    if (!cg_init(c, rr, reltol, abstol, maxiter)) return false;
    c.rho = rho;
    if (bad_diagonal) {
        c.count = -1;
        c.done = 1;
        return false;
    }
    return true;
}

// after pass 1 (pMp = p . M p): cg_step_length's guard, alpha = rho / p.Mp
CG_HD bool pcg_step_length(CgRecord& c, double pMp, double& alpha) {
    if (!(pMp > 0.0) || cg_is_inf(pMp)) {
        c.count = -1 - c.count;
        c.done = 1;
        return false;
    }
    alpha = c.rho / pMp;
    return true;
}

// after pass 2 (rr_new = r . r and rho_new = (r / d) . r of the updated residual): beta for the next direction, or false -- finished
CG_HD bool pcg_next(CgRecord& c, double rr_new, double rho_new, double& beta) {
    beta = rho_new / c.rho;
    c.rr = rr_new;
    c.rho = rho_new;
    c.count += 1;
    if (c.count == c.maxiter || cg_converged(c)) {
        c.done = 1;
        return false;
    }
    return true;
}

}  // namespace muse_lbfgs
