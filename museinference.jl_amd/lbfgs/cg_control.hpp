// cg_control.hpp -- every SCALAR decision of the lock-step conjugate-gradient solver of libmuse_lbfgs.so (include/muse_lbfgs.h,
// muse_lbfgs_cg_*): the record of one row -- one linear system M y = b whose operator is the CALLER's -- and what is decided between
// two applications of M.  Written once for the host (tests/native/cg_driver.cpp: naive loops for the vector work) and for the device
// (cg_kernels.hpp: one workgroup per row supplies the passes and the reductions).  No HIP types, as lbfgs_control.hpp: dot products
// come in, "stopped" / "finished" / alpha / beta go out.  Compiled without floating-point contraction on both sides.
//
// Plain CG in the order of simple._cg and of csrc/solver.hpp's plain_cg, with IterativeSolvers' stopping rule (solver.hpp's
// cg_tolerance): |r|_2 <= max(reltol |b|_2, abstol) on the recurrence residual, or maxiter iterations.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CG_HD __host__ __device__ __forceinline__
#else
#define CG_HD inline
#endif

namespace muse_lbfgs {

// One row's state between two rounds: r.r, the tolerance, the count.  `count` is the number of iterations taken, or -1 - iterations
// once the guard has stopped the row (p . M p not positive or not finite: M is not positive definite -- the convention of
// include/muse_hip.h's implicit get_H!, which muse.py reads).  `rho` is the preconditioned solver's (r / d) . r (pcg_control.hpp), which
// shares the record, the workspace and the count and result kernels; plain CG keeps it at zero and never reads it.
struct CgRecord {
    double rr, tol;
    int32_t count, maxiter, done, pad_;
    double rho;
};

CG_HD bool cg_is_inf(double v) { return __builtin_fabs(v) == __builtin_inf(); }

CG_HD double cg_tolerance(double rr, double reltol, double abstol) {
    const double tol_rel = reltol * __builtin_sqrt(rr);
    return tol_rel > abstol ? tol_rel : abstol;
}
CG_HD bool cg_converged(const CgRecord& c) { return __builtin_sqrt(c.rr) <= c.tol; }

// begin: rr = b . b.  Returns true while the row is active (a zero right-hand side or maxiter == 0 ends it at once, count 0, y = 0).
CG_HD bool cg_init(CgRecord& c, double rr, double reltol, double abstol, int maxiter) {
    c.rr = rr;
    c.tol = cg_tolerance(rr, reltol, abstol);
    c.count = 0;
    c.maxiter = maxiter;
    c.pad_ = 0;
    c.rho = 0.0;
    c.done = (maxiter <= 0 || cg_converged(c)) ? 1 : 0;
    return !c.done;
}

// after pass 1 (pMp = p . M p): the step length, or false -- the guard stopped the row, y stays at what it was
CG_HD bool cg_step_length(CgRecord& c, double pMp, double& alpha) {
    if (!(pMp > 0.0) || cg_is_inf(pMp)) {
        c.count = -1 - c.count;
        c.done = 1;
        return false;
    }
    alpha = c.rr / pMp;
    return true;
}

// after pass 2 (rr_new = r . r of the updated residual): beta for the next direction, or false -- the row has finished
CG_HD bool cg_next(CgRecord& c, double rr_new, double& beta) {
    beta = rr_new / c.rr;
    c.rr = rr_new;
    c.count += 1;
    if (c.count == c.maxiter || cg_converged(c)) {
        c.done = 1;
        return false;
    }
    return true;
}

}  // namespace muse_lbfgs
