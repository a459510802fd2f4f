/* saturating_response.h -- a response behind the stencil operator (include/muse_model.h, MUSE_MODEL_RESPONSE): a detector that
 * saturates,
 *     z_i ~ N(0, e^theta_k),   u = A z,   x_i = phi(u_i) + sd_i n_i,   phi(u) = u / sqrt(1 + (p0 u)^2)      (|phi| < 1 / |p0|)
 * -- no polynomial states it, which is what the family is for.  With s = p0 u and q = 1 + s^2:
 *     phi = u / sqrt(q),   phi' = 1 / (q sqrt(q)) in (0, 1],   phi'' = -3 p0 s / (q^2 sqrt(q)).
 * p1 is not used.  At p0 = 0: q = 1, sqrt(q) = 1, phi = u / 1 = u, phi' = 1 / 1 = 1 and phi'' = -0 exactly -- the context gives the
 * bytes of the stencil model without a response. */
#define MUSE_MODEL_RESPONSE 1
#define MUSE_MODEL_RESPONSE_SECOND 1
#include "muse_model.h"
#define MUSE_MODEL_NAME "saturating_response"

MUSE_MODEL_FN void muse_model_response(double u, const double* p, double* phi, double* dphi) {
    const double s = p[0] * u;
    const double q = fma(s, s, 1.0);
    const double rt = sqrt(q);
    *phi = u / rt;
    *dphi = 1.0 / (q * rt);
}
MUSE_MODEL_FN double muse_model_response_second(double u, const double* p) {
    const double s = p[0] * u;
    const double q = fma(s, s, 1.0);
    const double rt = sqrt(q);
    return -(3.0 * p[0] * s) / ((q * q) * rt);
}
