// lbfgs_advance.hpp -- one round of the reverse-communication L-BFGS: everything optim.lbfgs does between two evaluations of the
// objective, for ONE problem, over a vector backend V.  Host and device: the device backend (lbfgs_kernels.hip) is a workgroup with
// strided passes and fixed-shape reductions, the host backend (tests/native/lbfgs_driver.cpp) naive loops.
//
// V supplies the vector passes; every pass returns its reductions (the same value in every thread of a workgroup).  `g` is the
// gradient the caller evaluated at the current evaluation point `z`; x, s, g_prev and the pairs dx_i / dg_i are V's.
//   intake(gs, absmax, nanc)              g . s,  max |g_e| (NaNs dropped),  the number of NaN elements of g
//   start()                               q = g (q lives in s's storage),  g_prev = g
//   write_trial(c)                        z = x + c s
//   step_to(c)                            z = x = x + c s
//   pass_accept(alpha, slot, ...)         dx = alpha s, x += dx, dg = g - g_prev -> pair `slot`;  g_prev = g, q = g;
//                                         max |x_new - x|,  dx . dg,  dg . dg,  dx . g  (the first dot product of the two-loop recursion)
//   stage_down(a, i, inext)               q -= a dg_i;                  returns dx_inext . q      (the next stage's dot, fused)
//   stage_down_last(a, i, scale)          q -= a dg_i;  s = scale q;    returns dg_i . s
//   stage_up(coef, i, inext)              s += dx_i coef;               returns dg_inext . s
//   stage_up_last(coef, i)                s += dx_i coef;  s = -s;      returns g . s
//   negate_first()                        s = -q;                       returns g . s             (no history)
//   steepest()                            s = -g;                       returns g . s
//   rho(i) / set_rho(i, v) / alpha(i) / set_alpha(i, v)                 the per-pair scalars (indexed at run time)
#pragma once
#include "lbfgs_control.hpp"

namespace muse_lbfgs {

// f: the objective at z.  Returns true while the problem is active (z then holds the next evaluation point); a finished problem's
// z is its final point and its record no longer changes.
template <class V>
LBFGS_HD bool advance_problem(Problem& p, V& v, double f) {
    enum { N_LS_DONE, N_ACCEPT, N_NEW_ITER };
    if (p.phase == PH_DONE) return false;
    p.f_calls += 1;
    double gs, absmax, nanc;
    v.intake(gs, absmax, nanc);
    int next;
    if (p.phase == PH_START) {
        if (!start_check(p, f, absmax, nanc)) { finish(p); return false; }
        v.start();
        next = N_NEW_ITER;
    } else if (p.phase == PH_TRIAL) {
        p.f_last = f;
        p.gnorm_last = gmax_of(absmax, nanc);
        if (hz_feed(p.hz, f, gs) == HZ_EVAL) { v.write_trial(p.hz.c); return true; }
        next = N_LS_DONE;
    } else {
        next = N_ACCEPT;   // PH_FINAL: the re-evaluation at the accepted step
    }
    double dot = 0.0;
    for (;;) {
        if (next == N_LS_DONE) {
            if (!p.hz.ok) {                       // (optim.py:252-257)
                v.step_to(p.hz.alpha);
                linesearch_failed(p);
                finish(p);
                return false;
            }
            if (p.hz.alpha != p.hz.last_c) {      // the accepted step was not the last trial: one more evaluation
                v.write_trial(p.hz.alpha);
                p.phase = PH_FINAL;
                return true;
            }
            next = N_ACCEPT;
        }
        if (next == N_ACCEPT) {
            double x_diff, dxdg, dgdg, rho_it;
            int slot;
            v.pass_accept(p.hz.alpha, slot_of(p.pseudo), x_diff, dxdg, dgdg, dot);
            const bool done = accept(p, f, x_diff, absmax, nanc, dxdg, dgdg, rho_it, slot);
            if (slot >= 0) v.set_rho(slot, rho_it);
            if (done) { finish(p); return false; }
        }
        // the next iteration: two-loop recursion, the direction's slope, the first trial (optim.py:225-251)
        int lo, hi;
        if (!iteration_begin(p, lo, hi)) { finish(p); return false; }
        double dphi_0;
        if (hi < lo) {
            dphi_0 = v.negate_first();
        } else {
            for (int index = hi; index >= lo; --index) {
                const int i = slot_of(index);
                const double a = v.rho(i) * dot;
                v.set_alpha(i, a);
                dot = index > lo ? v.stage_down(a, i, slot_of(index - 1)) : v.stage_down_last(a, i, p.gamma);
            }
            dphi_0 = 0.0;
            for (int index = lo; index <= hi; ++index) {
                const int i = slot_of(index);
                const double coef = v.alpha(i) - v.rho(i) * dot;
                if (index < hi) dot = v.stage_up(coef, i, slot_of(index + 1));
                else dphi_0 = v.stage_up_last(coef, i);
            }
        }
        if (dphi_0 >= 0.0) {                      // reset_search_direction!
            p.pseudo = 1;
            dphi_0 = v.steepest();
        }
        p.f_prev = p.f;
        f = p.f;
        if (hz_begin(p.hz, 1.0, p.f, dphi_0) == HZ_EVAL) {
            v.write_trial(p.hz.c);
            p.phase = PH_TRIAL;
            return true;
        }
        next = N_LS_DONE;   // nothing to evaluate: alpha = 0 (the point is then unchanged and the iteration ends the run)
    }
}

}  // namespace muse_lbfgs
