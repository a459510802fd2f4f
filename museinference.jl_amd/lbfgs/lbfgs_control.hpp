// lbfgs_control.hpp -- every SCALAR decision of optim.lbfgs (optim.py: L-BFGS m = 10, InitialStatic(1), HagerZhang), written once for the
// host (tests/native/lbfgs_driver.cpp: naive loops for the vector work) and for the device (lbfgs_kernels.hip: one workgroup per
// problem supplies the vector passes and the reductions).  No HIP types, as csrc/step.hpp: dot products and maxima come in,
// "evaluate at c" / "accepted" / "converged" / coefficients go out.  Compiled without floating-point contraction on both sides.
//
// The line search is optim._hagerzhang as a state machine around ONE evaluation site (the structure of csrc/solver.hpp's linesearch,
// restated here because this one must SUSPEND: the evaluation is the caller's closure, a launch away), its state a plain record.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LBFGS_HD __host__ __device__ __forceinline__
#else
#define LBFGS_HD inline
#endif

namespace muse_lbfgs {

constexpr int kM = 10;                 // history length (Optim's LBFGS() default)
constexpr double kDelta = 0.1, kSigma = 0.9, kRho = 5.0, kEpsilon = 1e-6, kGamma = 0.66, kPsi3 = 0.1;   // optim.py:20
constexpr int kLinesearchMax = 50, kIterFiniteMax = 52;
constexpr double kEps = 2.220446049250313e-16;

enum { STATUS_G_CONVERGED = 0, STATUS_X_CONVERGED, STATUS_F_CONVERGED, STATUS_MAXITER, STATUS_LINESEARCH_FAILED, STATUS_NONFINITE };

LBFGS_HD double f_abs(double v) { return __builtin_fabs(v); }
LBFGS_HD bool is_finite(double v) { return v - v == 0.0; }
LBFGS_HD bool is_inf(double v) { return f_abs(v) == __builtin_inf(); }
LBFGS_HD bool finite2(double p, double d) { return is_finite(p) && is_finite(d); }
LBFGS_HD double from_bits(int64_t b) { double v; __builtin_memcpy(&v, &b, 8); return v; }
LBFGS_HD int64_t to_bits(double v) { int64_t b; __builtin_memcpy(&b, &v, 8); return b; }
LBFGS_HD double eps_of(double b) {          // nextafter(|b|, inf) - |b|
    const double ab = f_abs(b);
    return from_bits(to_bits(ab) + 1) - ab;
}
LBFGS_HD double nextup(double v) {          // nextafter(v, inf) for finite v
    if (v == 0.0) return 4.9406564584124654e-324;
    const int64_t b = to_bits(v);
    return from_bits(v > 0.0 ? b + 1 : b - 1);
}

struct HzPoint {
    double a, v, d;   // alpha, phi(alpha), dphi(alpha)
    int id, pad_;     // evaluation sequence number (0: the point alpha = 0)
};

// The suspended line search: seven points, five doubles, five counters, the result.
struct HzState {
    HzPoint P0, A, B, C, prev, a0, b0;
    double alphamax, cold, fail_alpha, c, last_c;
    double alpha;     // the result, once hz_* returns HZ_DONE
    int state, cont, iter, iterfinite, nid, ok;
};

enum { HZ_EVAL = 0, HZ_DONE = 1 };
enum { S_INIT, S_EXPAND, S_BIS, S_SEC1, S_SEC2, S_MID };
enum { CONT_BRACKET, CONT_UPD1, CONT_UPD2, CONT_UPD3 };

LBFGS_HD bool hz_wolfe(double c, double phi_c, double dphi_c, double phi_0, double dphi_0, double phi_lim) {
    const bool w1 = (kDelta * dphi_0 >= (phi_c - phi_0) / c) && (dphi_c >= kSigma * dphi_0);
    const bool w2 = ((2.0 * kDelta - 1.0) * dphi_0 >= dphi_c) && (dphi_c >= kSigma * dphi_0) && (phi_c <= phi_lim);
    return w1 || w2;
}
LBFGS_HD HzPoint hz_pick(bool c, const HzPoint& p, const HzPoint& q) {
    return HzPoint{c ? p.a : q.a, c ? p.v : q.v, c ? p.d : q.d, c ? p.id : q.id, 0};
}
LBFGS_HD double hz_secant(const HzPoint& p, const HzPoint& q) { return (p.a * q.d - q.a * p.d) / (q.d - p.d); }

// Start a search from the trial step c0 at a point with value phi_0 and slope dphi_0.  HZ_EVAL: evaluate at h.c and call hz_feed;
// HZ_DONE: nothing to evaluate, h.alpha / h.ok are the result (ok 0: LineSearches' exception, the caller stops).
// h.last_c = 0: the point evaluated last is the search's origin.
LBFGS_HD int hz_begin(HzState& h, double c0, double phi_0, double dphi_0) {
    const HzPoint p0{0.0, phi_0, dphi_0, 0, 0};
    h.P0 = h.A = h.B = h.C = h.prev = h.a0 = h.b0 = p0;
    h.alphamax = __builtin_inf();
    h.cold = 0.0;
    h.fail_alpha = 0.0;
    h.c = c0;
    h.last_c = 0.0;
    h.alpha = 0.0;
    h.state = S_INIT;
    h.cont = CONT_BRACKET;
    h.iter = 1;
    h.iterfinite = 1;
    h.nid = 1;
    h.ok = 1;
    if (!finite2(phi_0, dphi_0) || dphi_0 >= kEps * f_abs(phi_0)) { h.ok = 0; return HZ_DONE; }   // not a descent direction
    if (dphi_0 >= 0.0 || c0 <= kEps) return HZ_DONE;                                               // alpha = 0, nothing evaluated
    return HZ_EVAL;
}

// The value phi and slope dphi at h.c have been evaluated.  HZ_EVAL: evaluate at the new h.c; HZ_DONE: h.alpha / h.ok.
// (the caller re-evaluates at h.alpha when h.ok and h.alpha != h.last_c: optim._Objective's cache)
LBFGS_HD int hz_feed(HzState& h, double phi, double dphi) {
    const double phi_0 = h.P0.v, dphi_0 = h.P0.d;
    const double phi_lim = phi_0 + kEpsilon * f_abs(phi_0);
    const bool fin = finite2(phi, dphi);
    const double c = h.c;
    h.last_c = c;
    switch (h.state) {
        case S_INIT:
            if (!fin) {
                if (h.iterfinite < kIterFiniteMax) { h.iterfinite += 1; h.c = c * kPsi3; return HZ_EVAL; }
                h.alpha = 0.0;
                return HZ_DONE;
            }
            h.C = HzPoint{c, phi, dphi, h.nid++, 0};
            goto L_BRACKET_TOP;
        case S_EXPAND:
            if (!fin) {
                if (c > nextup(h.cold) && h.iterfinite < kIterFiniteMax) {
                    h.alphamax = c;
                    h.iterfinite += 1;
                    h.c = (h.cold + c) / 2.0;
                    return HZ_EVAL;
                }
                h.alpha = h.cold;
                return HZ_DONE;
            }
            h.C = HzPoint{c, phi, dphi, h.nid++, 0};
            h.iter += 1;
            goto L_BRACKET_TOP;
        case S_BIS: {
            if (!fin) goto L_FAIL;
            const HzPoint D{c, phi, dphi, h.nid++, 0};
            if (D.d >= 0.0) { h.B = D; goto L_BISECT_RETURN; }
            const bool low = D.v <= phi_lim;     // (selected by value: a choice between two destinations keeps the record in memory)
            h.A = hz_pick(low, D, h.A);
            h.B = hz_pick(low, h.B, D);
            goto L_BISECT_TOP;
        }
        case S_SEC1:
            if (!fin) goto L_FAIL;
            h.C = HzPoint{c, phi, dphi, h.nid++, 0};
            if (hz_wolfe(c, phi, dphi, phi_0, dphi_0, phi_lim)) { h.alpha = c; return HZ_DONE; }
            h.cont = CONT_UPD1;
            goto L_UPDATE;
        case S_SEC2:
            if (!fin) goto L_FAIL;
            h.C = HzPoint{c, phi, dphi, h.nid++, 0};
            if (hz_wolfe(c, phi, dphi, phi_0, dphi_0, phi_lim)) { h.alpha = c; return HZ_DONE; }
            h.cont = CONT_UPD2;
            goto L_UPDATE;
        default:  // S_MID
            if (!fin) goto L_FAIL;
            h.C = HzPoint{c, phi, dphi, h.nid++, 0};
            h.cont = CONT_UPD3;
            goto L_UPDATE;
    }
L_BRACKET_TOP:
    if (!(h.iter < kLinesearchMax)) { h.alpha = 0.0; goto L_FAIL_KEEP; }   // never bracketed
    if (h.C.d >= 0.0) {
        h.A = h.prev;    // the latest point with phi <= phi_lim (and dphi < 0)
        h.B = h.C;
        h.iter += 1;
        goto L_MAIN_TOP;
    } else if (h.C.v > phi_lim) {
        h.A = h.P0;
        h.B = h.C;
        h.cont = CONT_BRACKET;
        h.fail_alpha = 0.0;
        goto L_BISECT_ENTER;
    } else {
        h.cold = h.C.a;
        if (nextup(h.cold) >= h.alphamax) { h.alpha = h.cold; return HZ_DONE; }
        h.prev = h.C;
        double cn = h.cold * kRho;
        if (cn > h.alphamax) cn = h.alphamax;
        h.c = cn;
        h.iterfinite = 1;
        h.state = S_EXPAND;
        return HZ_EVAL;
    }
L_UPDATE:   // HZ stages U0-U3 on (A, B) with the new point C
    if (!(h.A.d < 0.0 && h.A.v <= phi_lim && h.B.d >= 0.0 && h.B.a > h.A.a)) goto L_FAIL;
    if (h.C.a < h.A.a || h.C.a > h.B.a) goto L_UPDATE_RETURN;
    {   // U1: dphi(C) >= 0 -> B = C;  U2: phi(C) <= phi_lim -> A = C;  U3: B = C and bisect  (selected by value, as in S_BIS)
        const bool up = h.C.d >= 0.0, low = h.C.v <= phi_lim;
        const bool to_a = !up && low;
        h.A = hz_pick(to_a, h.C, h.A);
        h.B = hz_pick(to_a, h.B, h.C);
        if (up || low) goto L_UPDATE_RETURN;
    }
L_BISECT_ENTER:
    if (!(h.A.d < 0.0 && h.A.v <= phi_lim && h.B.d < 0.0 && h.B.v > phi_lim && h.B.a > h.A.a)) goto L_FAIL;
L_BISECT_TOP:
    if (h.B.a - h.A.a > eps_of(h.B.a)) {
        h.c = (h.A.a + h.B.a) / 2.0;
        h.state = S_BIS;
        return HZ_EVAL;
    }
L_BISECT_RETURN:
    if (h.cont == CONT_BRACKET) { h.iter += 1; goto L_MAIN_TOP; }
L_UPDATE_RETURN:
    if (h.cont == CONT_UPD1) {
        const bool updB = (h.B.id == h.C.id), updA = (h.A.id == h.C.id);
        const double sB = hz_secant(h.b0, h.B), sA = hz_secant(h.a0, h.A);   // (both formed, one used: no choice between addresses)
        const double c2 = updB ? sB : (updA ? sA : h.C.a);
        if ((updA || updB) && h.A.a <= c2 && c2 <= h.B.a) {
            h.c = c2;
            h.state = S_SEC2;
            return HZ_EVAL;
        }
    }
    if (h.cont == CONT_UPD3) { h.iter += 1; goto L_MAIN_TOP; }
    // after secant2 (CONT_UPD1 without a second step, or CONT_UPD2)
    if (!(h.B.a > h.A.a)) { h.alpha = h.A.a; goto L_FAIL_KEEP; }
    if (h.B.a - h.A.a < kGamma * (h.b0.a - h.a0.a)) {
        if (nextup(h.a0.v) >= h.b0.v && nextup(h.A.v) >= h.B.v) { h.alpha = h.A.a; return HZ_DONE; }   // flat
        h.iter += 1;
        goto L_MAIN_TOP;
    }
    h.fail_alpha = h.A.a;
    h.c = (h.A.a + h.B.a) / 2.0;
    h.state = S_MID;
    return HZ_EVAL;
L_MAIN_TOP:
    if (!(h.iter < kLinesearchMax)) { h.alpha = h.A.a; goto L_FAIL_KEEP; }
    h.a0 = h.A;
    h.b0 = h.B;
    if (!(h.b0.a > h.a0.a)) { h.alpha = h.a0.a; goto L_FAIL_KEEP; }
    if (h.b0.a - h.a0.a <= eps_of(h.b0.a)) { h.alpha = h.a0.a; return HZ_DONE; }
    h.fail_alpha = h.a0.a;
    if (!(h.a0.d < 0.0 && h.b0.d >= 0.0)) goto L_FAIL;
    {
        const double cs = hz_secant(h.a0, h.b0);
        if (!is_finite(cs)) goto L_FAIL;
        h.c = cs;
    }
    h.state = S_SEC1;
    return HZ_EVAL;
L_FAIL:
    h.alpha = h.fail_alpha;
L_FAIL_KEEP:
    h.ok = 0;
    return HZ_DONE;
}

// ---- the L-BFGS bookkeeping between two evaluations ----------------------------------------------------------------------------
// One problem's record.  The vectors (x, s, g_prev, the m pairs dx_i / dg_i) are the caller's.
enum { PH_START = 0, PH_TRIAL = 1, PH_FINAL = 2, PH_DONE = 3 };

struct Problem {
    HzState hz;
    double f, f_prev, gnorm, g_tol;
    double gamma;                // (dx . dg) / (dg . dg) of the newest pair: the two-loop recursion's scaling
    double f_last, gnorm_last;   // the value / gradient maximum of the point evaluated last (what a failed search reports)
    int phase, pseudo, iterations, f_calls, status, counter_f, maxiter, pad_;
};

LBFGS_HD void problem_init(Problem& p, double g_tol, int maxiter) {
    p.gamma = 1.0;
    p.f = p.f_prev = p.gnorm = p.f_last = p.gnorm_last = __builtin_nan("");
    p.g_tol = g_tol;
    p.phase = PH_START;
    p.pseudo = 0;
    p.iterations = 0;
    p.f_calls = 0;
    p.status = STATUS_MAXITER;
    p.counter_f = 0;
    p.maxiter = maxiter;
    p.pad_ = 0;
    hz_begin(p.hz, 1.0, 0.0, 0.0);
}

// torch's v.abs().max(): NaN if any element is, else the maximum (an infinity included)
LBFGS_HD double gmax_of(double absmax, double nan_count) { return nan_count != 0.0 ? __builtin_nan("") : absmax; }
LBFGS_HD bool all_finite(double absmax, double nan_count) { return nan_count == 0.0 && absmax < __builtin_inf(); }

// The first evaluation (optim.py:216-223).  true: go on to the first iteration.
LBFGS_HD bool start_check(Problem& p, double f, double absmax, double nan_count) {
    p.f = p.f_last = f;
    p.gnorm = p.gnorm_last = gmax_of(absmax, nan_count);
    if (!is_finite(f) || !all_finite(absmax, nan_count)) { p.status = STATUS_NONFINITE; return false; }
    if (p.gnorm <= p.g_tol) { p.status = STATUS_G_CONVERGED; return false; }
    return true;
}

// Top of an iteration (optim.py:225-228).  false: maxiter reached.  lo .. hi: the history indices of the two-loop recursion
// (none when hi < lo); slot(index) = (index - 1) % m.
LBFGS_HD bool iteration_begin(Problem& p, int& lo, int& hi) {
    if (!(p.iterations < p.maxiter)) return false;
    p.iterations += 1;
    p.pseudo += 1;
    const int lower = p.pseudo - kM;
    hi = p.pseudo - 1;
    lo = lower > 1 ? lower : 1;
    return true;
}
LBFGS_HD int slot_of(int index) { return (index - 1) % kM; }
LBFGS_HD double twoloop_scale(double dxdg, double dgdg) { return dxdg / dgdg; }

// After the accepted point's evaluation (optim.py:258-280): x_diff = max|x - x_prev|, (absmax, nan_count) of the new gradient,
// dxdg = dx . (g - g_prev).  true: stop.  The pair goes into slot_of(pseudo as it was) -- the caller has already written it there: a
// reset history (pseudo = 0) is refilled from slot 0 before any of it is read again.
// slot >= 0: rho[slot] = rho_it is the caller's to store (the rho_i live with the vectors' owner: they are indexed at run time).
LBFGS_HD bool accept(Problem& p, double f, double x_diff, double absmax, double nan_count, double dxdg, double dgdg, double& rho_it, int& slot) {
    const double f_prev = p.f_prev;
    p.f = p.f_last = f;
    p.gnorm = p.gnorm_last = gmax_of(absmax, nan_count);
    const bool x_conv = x_diff <= 0.0;
    const bool f_conv = f_abs(f - f_prev) <= 0.0;
    const bool g_conv = p.gnorm <= p.g_tol;
    p.counter_f = f_conv ? p.counter_f + 1 : 0;
    bool done = x_conv || g_conv || p.counter_f > 1;
    if (g_conv) p.status = STATUS_G_CONVERGED;
    else if (x_conv) p.status = STATUS_X_CONVERGED;
    else if (p.counter_f > 1) p.status = STATUS_F_CONVERGED;
    p.gamma = twoloop_scale(dxdg, dgdg);
    rho_it = dxdg == 0.0 ? __builtin_inf() : 1.0 / dxdg;
    slot = -1;
    if (is_inf(rho_it)) p.pseudo = 0;
    else slot = slot_of(p.pseudo);
    if (!all_finite(absmax, nan_count)) { p.status = STATUS_NONFINITE; done = true; }
    return done;
}

// The end (optim.py:281-282).
LBFGS_HD void finish(Problem& p) {
    if (p.status <= STATUS_F_CONVERGED && !is_finite(p.f)) p.status = STATUS_NONFINITE;
    p.phase = PH_DONE;
}
// A failed line search (optim.py:254-257): the value and gradient reported are those of the point evaluated last.
LBFGS_HD void linesearch_failed(Problem& p) {
    p.status = STATUS_LINESEARCH_FAILED;
    p.f = p.f_last;
    p.gnorm = p.gnorm_last;
}

}  // namespace muse_lbfgs
