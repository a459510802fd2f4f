// cg_advance.hpp -- one round of the reverse-communication conjugate gradients: everything between two applications of the caller's
// operator M, for ONE row, over a vector backend V.  Host and device: the device backend (cg_kernels.hpp) is a workgroup with strided
// passes and fixed-shape reductions, the host backend (tests/native/cg_driver.cpp) naive loops.
//
// V supplies the passes; every pass returns its reduction (the same value in every thread of a workgroup).  `Mp` is M applied by the
// caller to the direction p, which lives in the caller's evaluation row and nowhere else; y and r are V's.
//   start()                    y = 0, r = b, p = b;              returns b . b
//   dot_p_Mp()                                                   returns p . Mp
//   update(alpha)              y += alpha p, r -= alpha Mp;      returns r . r
//   next_direction(beta)       p = r + beta p
#pragma once
#include "cg_control.hpp"

namespace muse_lbfgs {

// Returns true while the row is active (p then holds the first direction, b itself).
template <class V>
CG_HD bool cg_begin_row(CgRecord& c, V& v, double reltol, double abstol, int maxiter) {
    return cg_init(c, v.start(), reltol, abstol, maxiter);
}

// Returns true while the row is active (p then holds the next direction); a finished row's p, y and record no longer change.
template <class V>
CG_HD bool cg_advance_row(CgRecord& c, V& v) {
    if (c.done) return false;
    double alpha, beta;
    if (!cg_step_length(c, v.dot_p_Mp(), alpha)) return false;
    if (!cg_next(c, v.update(alpha), beta)) return false;
    v.next_direction(beta);
    return true;
}

}  // namespace muse_lbfgs
