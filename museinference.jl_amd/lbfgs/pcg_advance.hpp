// pcg_advance.hpp -- one round of the reverse-communication PRECONDITIONED conjugate gradients (pcg_control.hpp): everything between
// two applications of the caller's operator M, for ONE row, over a vector backend V.  Host and device, as cg_advance.hpp: the device
// backend (pcg_kernels.hpp) is a workgroup with strided passes and fixed-shape reductions, the host backend
// (tests/native/pcg_driver.cpp) naive loops.
//
// V supplies the passes; every pass returns its reductions (the same values in every thread of a workgroup).  d is the row's diagonal,
// read-only and the caller's.  r / d is a division formed where it is used -- in update() and in next_direction() from the same r and d,
// so with the same bits -- and never stored: the passes are bound by their loads and stores (csrc/solver.hpp's jacobi_cg), and the
// workspace stays the plain solver's.
//   start(rr, rho, bad)             y = 0, r = b, p = b / d;          rr = b . b, rho = (b / d) . b, bad = entries of d not positive or
//                                                                     not finite (a count; zero: the diagonal is usable)
//   direction_is_rhs()              p = b                             (a row with a bad diagonal: the operator keeps seeing finite input)
//   dot_p_Mp()                                                        returns p . Mp
//   update(alpha, rr, rho)          y += alpha p, r -= alpha Mp;      rr = r . r, rho = (r / d) . r: ONE pass, one reduction of two values
//   next_direction(beta)            p = r / d + beta p
#pragma once
#include "pcg_control.hpp"

namespace muse_lbfgs {

// Returns true while the row is active (p then holds the first direction, b / d).
template <class V>
CG_HD bool pcg_begin_row(CgRecord& c, V& v, double reltol, double abstol, int maxiter) {
    double rr, rho, bad;
    v.start(rr, rho, bad);
    if (bad != 0.0) v.direction_is_rhs();
    return pcg_init(c, rr, rho, bad != 0.0, reltol, abstol, maxiter);
}

// Returns true while the row is active (p then holds the next direction); a finished row's p, y and record no longer change.
template <class V>
CG_HD bool pcg_advance_row(CgRecord& c, V& v) {
    if (c.done) return false;
    double alpha, beta, rr, rho;
    if (!pcg_step_length(c, v.dot_p_Mp(), alpha)) return false;
    v.update(alpha, rr, rho);
    if (!pcg_next(c, rr, rho, beta)) return false;
    v.next_direction(beta);
    return true;
}

}  // namespace muse_lbfgs
