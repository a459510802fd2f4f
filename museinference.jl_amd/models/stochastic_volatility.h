/* stochastic_volatility.h -- Neal's funnel proper, a model of the TWO-PARAMETER family (include/muse_model.h, MUSE_MODEL_PAIR) whose
 * per-element functions call muse_model_exp: the latent log-variance of every element is drawn around the block's level,
 *
 *     z_i ~ N(mu_k, e^tau_k),   x_i ~ N(0, e^z_i)          k = the element's block, theta = (mu_0 .. mu_{K-1}, tau_0 .. tau_{K-1})
 *
 * -logLike = 1/2 sum_i [ x_i^2 e^-z_i + z_i + e^-tau_k (z_i - mu_k)^2 ] + 1/2 sum_k n_k tau_k: nothing integrates out in closed form
 * and the posterior of z is far from Gaussian.  As a SimpleMuseProblem of the reference (src/simple.jl:79-95), with one block,
 *     sample_x_z = (rng, th) -> (z = th.mu .+ exp(th.tau / 2) .* randn(rng, N); x = exp.(z ./ 2) .* randn(rng, N); (; x, z))
 *     logLike    = (x, z, th) -> -(sum(x.^2 .* exp.(-z) .+ z) + exp(-th.tau) * sum((z .- th.mu).^2) + N * th.tau) / 2
 * The header is also what ElementwiseModel.from_pair_expressions writes from
 *     coefs = ["a", "exp(b/2)", "exp(-b)", "1"], C = "b", o = "x**2*exp(-z) + c3*z + c2*(z - c0)**2", z = "c0 + c1*n1", x = "exp(z/2)*n2". */
#define MUSE_MODEL_PAIR 1
#define MUSE_MODEL_PAIR_SECOND 1
#include "muse_model.h"
#define MUSE_MODEL_NAME "stochastic_volatility"

/* c = { mu, sd = e^(tau/2), iv = e^-tau, 1 };  the block's constant per element: C = tau.  c[3] multiplies what would otherwise
 * contribute at the pad element (x = z = 0 with ZERO coefficients): the z of o and hence the 1/2 of its gradient. */
MUSE_MODEL_FN double muse_model_coefs(double mu, double tau, double* c) {
    c[0] = mu;
    c[1] = muse_model_exp(0.5 * tau);
    c[2] = muse_model_exp(-tau);
    c[3] = 1.0;
    return tau;
}
MUSE_MODEL_FN void muse_model_sample(const double* c, double n1, double n2, double* z, double* x, long i) {
    (void)i;
    const double zi = fma(c[1], n1, c[0]);
    *z = zi;
    *x = muse_model_exp(0.5 * zi) * n2;
}
/* o = x^2 e^-z + c3 z + iv (z - mu)^2;   d(1/2 o)/dz = 1/2 (c3 - x^2 e^-z) + iv (z - mu): one exponential for both */
MUSE_MODEL_FN double muse_model_grad(const double* c, double x, double z, double* acc, long i) {
    (void)i;
    const double w = muse_model_exp(-z) * (x * x);
    const double d = c[0] - z;
    *acc = fma(c[2], d * d, fma(c[3], z, w + *acc));
    return fma(0.5, c[3], -0.5 * w) - c[2] * d;
}
MUSE_MODEL_FN void muse_model_score_terms(const double* c, double x, double z, double* t0, double* t1, long i) {
    (void)x; (void)i;
    const double d = c[3] * (z - c[0]);
    *t0 = d;
    *t1 = d * d;
}
/* d logLike / d mu = iv sum (z - mu);   d logLike / d tau = 1/2 (iv sum (z - mu)^2 - n) */
MUSE_MODEL_FN void muse_model_score(const double* c, double S0, double S1, double n, double* ga, double* gb) {
    *ga = c[2] * S0;
    *gb = 0.5 * (c[2] * S1 - n);
}
/* g = 1/2 (c3 - x^2 e^-z) + iv (z - mu):  dg/dz = 1/2 x^2 e^-z + iv,  dg/dx = -x e^-z,  dg/dmu = -iv,  dg/dtau = -iv (z - mu);
 * the score terms do not depend on x;  x = e^(z/2) n2 with z = mu + sd n1:  dx/dmu = x / 2,  dx/dtau = x / 2 * (sd n1 / 2). */
MUSE_MODEL_FN void muse_model_pair_second(const double* c, double x, double z, double* ozz, double* ozx, double* gza, double* gzb,
                                          double* sxa, double* sxb, long i) {
    (void)i;
    const double xe = x * muse_model_exp(-z);
    *ozz = fma(0.5 * x, xe, c[2]);
    *ozx = -xe;
    *gza = -c[2];
    *gzb = -(c[2] * (z - c[0]));
    *sxa = 0.0;
    *sxb = 0.0;
}
MUSE_MODEL_FN void muse_model_pair_dx(const double* c, double n1, double n2, double* xa, double* xb, long i) {
    (void)i;
    const double hx = 0.5 * (muse_model_exp(0.5 * fma(c[1], n1, c[0])) * n2);
    *xa = hx;
    *xb = hx * (0.5 * (c[1] * n1));
}
