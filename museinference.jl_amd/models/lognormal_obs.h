/* lognormal_obs.h -- a model of the one-parameter family (include/muse_model.h) whose per-element functions call muse_model_exp:
 * a funnel seen through an EXPONENTIAL observation function,
 *     z_i ~ N(0, e^theta_k),   x_i ~ N(h(z_i), 1),   h(z) = 2 (e^(z/2) - 1)        (h(0) = 0, h'(z) = e^(z/2) > 0, h'(0) = 1)
 * so that  -logLike = 1/2 sum_i [ (x_i - h(z_i))^2 + e^-theta_k z_i^2 ] + 1/2 sum_k n_k theta_k :  A = (x - h(z))^2, B = z^2, and the
 * pad element (x = z = 0) contributes nothing.  (The plain e^z - 1 makes the MAP objective so stiff that L-BFGS needs hundreds of
 * iterations per solve; this h keeps the curvature of a unit-slope link at the origin.)  Equivalently
 *     ElementwiseModel.from_expressions(name, A="(x - 2*(exp(z/2) - 1))**2", B="z**2", z="sd*n1", x="2*(exp(z/2) - 1) + n2"). */
#include "muse_model.h"
#define MUSE_MODEL_NAME "lognormal_obs"
#define MUSE_MODEL_SECOND 1

MUSE_MODEL_FN void muse_model_sample(double sd, double n1, double n2, double* z, double* x, long i) {
    (void)i;
    const double zi = sd * n1;
    *z = zi;
    *x = fma(2.0, muse_model_exp(0.5 * zi), n2 - 2.0);
}
/* one exponential: e = e^(z/2) is h' and, as 2 e - 2, h */
MUSE_MODEL_FN double muse_model_grad(double iv, double x, double z, double* acc, long i) {
    (void)i;
    const double e = muse_model_exp(0.5 * z);
    const double r = fma(-2.0, e, x + 2.0);     /* x - h(z) */
    *acc = fma(iv, z * z, fma(r, r, *acc));
    return fma(iv, z, -(r * e));                /* iv z - (x - h) h'(z) */
}
MUSE_MODEL_FN double muse_model_score_term(double x, double z, long i) {
    (void)i;
    (void)x;
    return z * z;
}
/* With o = 1/2 [(x - h)^2 + iv z^2]:  d2o/dz2 = iv + h'^2 - (x - h) h'',  d2o/dzdx = -h'  (h'' = e^(z/2) / 2);
 * B = z^2: dB/dz = 2 z, dB/dx = 0;  x = h(sd n1) + n2: dx/dsd = h'(sd n1) n1. */
MUSE_MODEL_FN void muse_model_second(double iv, double x, double z, double* ozz, double* ozx, double* bz, double* bx, long i) {
    (void)i;
    const double e = muse_model_exp(0.5 * z);
    const double r = fma(-2.0, e, x + 2.0);
    *ozz = fma(e, e, fma(-0.5, e * r, iv));
    *ozx = -e;
    *bz = 2.0 * z;
    *bx = 0.0;
}
MUSE_MODEL_FN double muse_model_dx_dsd(double sd, double n1, double n2, long i) {
    (void)i;
    (void)n2;
    return muse_model_exp(0.5 * (sd * n1)) * n1;
}
