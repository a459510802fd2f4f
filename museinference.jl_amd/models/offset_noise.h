/* offset_noise.h -- a model of the TWO-PARAMETER family (include/muse_model.h, MUSE_MODEL_PAIR) whose parameters both sit in the
 * DATA factor, with its second derivatives (MUSE_MODEL_PAIR_SECOND: both get_H! branches),
 *
 *     z_i ~ N(0, 1),   x_i ~ N(z_i + mu_k, e^tau_k)      k = the element's block, theta = (mu_0 .. mu_{K-1}, tau_0 .. tau_{K-1})
 *
 * -logLike = 1/2 sum_i [ z_i^2 + e^-tau_k (x_i - z_i - mu_k)^2 ] + 1/2 sum_k n_k tau_k.  The latent field integrates out in closed
 * form (x_i ~ N(mu_k, 1 + e^tau_k) independently: the marginal of models/normal_mean_var.h), so MUSE's estimate can be compared with
 * the exact marginal posterior.  Unlike that model the score depends on x directly: H1 of the implicit-differentiation get_H!
 * (src/muse.jl:353-358) is not zero here.  As a SimpleMuseProblem of the reference (src/simple.jl:79-95) this is
 *     sample_x_z = (rng, th) -> (z = randn(rng, N); x = z .+ th.mu .+ exp.(th.tau ./ 2) .* randn(rng, N); (; x, z))
 *     logLike    = (x, z, th) -> -(sum(z.^2) + sum(exp.(-th.tau) .* (x .- z .- th.mu).^2) + N * th.tau) / 2
 * with one block. */
#define MUSE_MODEL_PAIR 1
#define MUSE_MODEL_PAIR_SECOND 1
#include "muse_model.h"
#define MUSE_MODEL_NAME "offset_noise"

/* c = { mu, sd = e^(tau/2), iv = e^-tau, (unused) };  the block's constant per element: C = tau */
MUSE_MODEL_FN double muse_model_coefs(double mu, double tau, double* c) {
    c[0] = mu;
    c[1] = muse_model_exp(0.5 * tau);
    c[2] = muse_model_exp(-tau);
    c[3] = 0.0;
    return tau;
}
MUSE_MODEL_FN void muse_model_sample(const double* c, double n1, double n2, double* z, double* x, long i) {
    (void)i;
    *z = n1;
    *x = fma(c[1], n2, n1 + c[0]);
}
/* d(1/2 o)/dz = z - iv (x - z - mu);  o = z^2 + iv (x - z - mu)^2 */
MUSE_MODEL_FN double muse_model_grad(const double* c, double x, double z, double* acc, long i) {
    (void)i;
    const double r = (x - z) - c[0], t = c[2] * r;
    *acc = fma(z, z, fma(t, r, *acc));
    return z - t;
}
MUSE_MODEL_FN void muse_model_score_terms(const double* c, double x, double z, double* t0, double* t1, long i) {
    (void)i;
    const double r = (x - z) - c[0];
    *t0 = r;
    *t1 = r * r;
}
/* d logLike / d mu = iv sum (x - z - mu);   d logLike / d tau = 1/2 (iv sum (x - z - mu)^2 - n) */
MUSE_MODEL_FN void muse_model_score(const double* c, double S0, double S1, double n, double* ga, double* gb) {
    *ga = c[2] * S0;
    *gb = 0.5 * (c[2] * S1 - n);
}
/* With g = d(1/2 o)/dz = z - iv r, sa = -1/2 do/dmu = iv r, sb = -1/2 do/dtau = 1/2 iv r^2 (r = x - z - mu; d iv / d tau = -iv):
 * ozz = dg/dz, ozx = dg/dx, gza = dg/dmu, gzb = dg/dtau, sxa = d sa / dx, sxb = d sb / dx */
MUSE_MODEL_FN void muse_model_pair_second(const double* c, double x, double z, double* ozz, double* ozx, double* gza, double* gzb,
                                          double* sxa, double* sxb, long i) {
    (void)i;
    const double r = (x - z) - c[0], t = c[2] * r;
    *ozz = 1.0 + c[2];
    *ozx = -c[2];
    *gza = c[2];
    *gzb = t;
    *sxa = c[2];
    *sxb = t;
}
/* x = z + mu + sd n2 at fixed normals: dx/dmu = 1, dx/dtau = 1/2 sd n2 */
MUSE_MODEL_FN void muse_model_pair_dx(const double* c, double n1, double n2, double* xa, double* xb, long i) {
    (void)i; (void)n1;
    *xa = 1.0;
    *xb = 0.5 * (c[1] * n2);
}
