/* exp_probe.h -- a TEST header (tests/test_gpu_model_exp.py): the funnel whose draw returns  x_i = muse_model_exp(P(i)),  P a run-time
 * constant vector (include/muse_model.h, muse_const) -- what reads the device's per-element exponential (csrc/model_math.hpp) back
 * through the sampler, argument by argument, with no solve.  The engine accepts finite constants only, so a second vector selects
 * the three non-finite arguments: Q(i) = 1: +inf, 2: -inf, 3: NaN, anything else: P(i). */
#define MUSE_MODEL_NCONST 2
#include "muse_model.h"
#define MUSE_MODEL_NAME "exp_probe"

MUSE_MODEL_FN void muse_model_sample(double sd, double n1, double n2, double* z, double* x, long i) {
    (void)n2;
    const double q = muse_const(1, i), p = muse_const(0, i);
    const double a = q == 1.0 ? (double)INFINITY : q == 2.0 ? -(double)INFINITY : q == 3.0 ? (double)NAN : p;
    *z = sd * n1;
    *x = muse_model_exp(a);
}
MUSE_MODEL_FN double muse_model_grad(double iv, double x, double z, double* acc, long i) {
    (void)i;
    const double r = x - z, t = iv * z;
    *acc = fma(t, z, fma(r, r, *acc));
    return t - r;
}
MUSE_MODEL_FN double muse_model_score_term(double x, double z, long i) {
    (void)i;
    (void)x;
    return z * z;
}
