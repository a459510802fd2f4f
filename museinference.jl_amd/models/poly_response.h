/* poly_response.h -- a response behind the stencil operator (include/muse_model.h, MUSE_MODEL_RESPONSE): the cubic of muse_set_link,
 *     z_i ~ N(0, e^theta_k),   u = A z,   x_i = phi(u_i) + sd_i n_i,   phi(u) = u + p0 u^2 + p1 u^3,
 * written in the expressions of the built-in link (csrc/models.hpp: link_value, link_slope), operand for operand.  After inlining the
 * kernels of this library evaluate the built-in's rounded operations: a context of it gives the bytes of a "smooth" context with
 * set_link((p0, p1)) -- what tests/test_gpu_response.py holds the header seam to -- and at p = (0, 0) those of the context without
 * a link.  phi'' makes the implicit-differentiation get_H! available, which the built-in link context refuses. */
#define MUSE_MODEL_RESPONSE 1
#define MUSE_MODEL_RESPONSE_SECOND 1
#include "muse_model.h"
#define MUSE_MODEL_NAME "poly_response"

MUSE_MODEL_FN void muse_model_response(double u, const double* p, double* phi, double* dphi) {
    *phi = fma(u * fma(p[1], u, p[0]), u, u);              /* u + u^2 (p0 + p1 u) */
    *dphi = fma(u, fma(3.0 * p[1], u, 2.0 * p[0]), 1.0);   /* 1 + u (2 p0 + 3 p1 u) */
}
MUSE_MODEL_FN double muse_model_response_second(double u, const double* p) {
    return fma(6.0 * p[1], u, 2.0 * p[0]);                 /* 2 p0 + 6 p1 u */
}
