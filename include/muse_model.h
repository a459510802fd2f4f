/*
 * muse_model.h -- the contract of a USER-SUPPLIED elementwise model (MUSE_MODEL_USER of muse_hip.h).
 *
 * The reference takes a model as closures: SimpleMuseProblem(x, sample_x_z, logLike, logPrior), differentiated by AD
 * (src/simple.jl:79-95).  Closures cannot cross a C ABI and nothing differentiates device code here, so a user model
 * is a small C header with three functions that is COMPILED INTO an engine library of its own (`libmuse_hip_model_<name>.so`,
 * museinference.jl_amd/build.py build_model_library; Python: museinference_jl_amd.ElementwiseModel) -- every instantiation
 * of the solver kernel (register/LDS-resident, streaming, workgroup clusters), the sampler, the finite-difference and
 * multi-map launches, the native muse! loop: the whole C ABI of muse_hip.h, for that model.
 *
 * The family.  With theta_k the parameter of block k (muse_hip.h: ntheta contiguous equal blocks of the N elements),
 * n_k its number of elements, sd_k = exp(theta_k / 2) and iv_k = exp(-theta_k):
 *
 *     -logLike(x, z, theta) = 1/2 sum_i [ A(x_i, z_i) + iv_k(i) B(x_i, z_i) ] + 1/2 sum_k n_k theta_k
 *     (x_i, z_i) ~ P(x, z | theta):  a function of sd_k(i) and two independent standard normals
 *
 * i.e. theta_k is the log-variance of ONE Gaussian factor of the elementwise joint density and everything else --
 * the observation function, the other factor -- is arbitrary (non-Gaussian, non-linear).  MUSE_MODEL_FUNNEL is the
 * member A = (x - z)^2, B = z^2, z = sd n1, x = z + n2; MUSE_MODEL_NOISE is A = z^2, B = (x - z)^2, z = n1, x = z + sd n2.
 * The score follows from the family:  d logLike / d theta_k = 1/2 (iv_k sum_{i in k} B(x_i, z_i) - n_k).
 *
 * The header defines (MUSE_MODEL_FN is supplied by the includer: host + device, inlined; plain C, doubles only, every
 * operation an IEEE + - * / sqrt or fma(), or the contract's exponential muse_model_exp(x) -- see EXPONENTIALS below --; the
 * engine and its CPU checker compile the SAME text without floating-point contraction, which is what makes their results
 * comparable bit for bit):
 *
 *     #define MUSE_MODEL_NAME "cubic"
 *     MUSE_MODEL_FN void   muse_model_sample(double sd, double n1, double n2, double* z, double* x, long i);
 *         the joint draw (src/interface.jl:92-99) of one element from the block's sd and two standard normals
 *     MUSE_MODEL_FN double muse_model_grad(double iv, double x, double z, double* acc, long i);
 *         returns d(-logLike)/dz_i = 1/2 d(A + iv B)/dz and ADDS A(x, z) + iv B(x, z) to *acc -- the running sum of
 *         the elements a thread owns, so the additions may be folded into fma()s as the built-in models do
 *         (src/interface.jl:68-83 with the sign Optim minimises, src/interface.jl:163)
 *     MUSE_MODEL_FN double muse_model_score_term(double x, double z, long i);
 *         B(x, z) (src/interface.jl:41-58: the engine assembles grad_theta logLike from its block sums)
 *
 * `i` is the element's index, 0 <= i < N -- and i >= N for the zero pad element of an odd-length vector and the phantom slots
 * behind it (x = z = 0 there: the functions must stay finite; the accessors of from_source's tables clamp the index): what lets a model
 * depend on the element through constants of its own (a known spectrum P_i: z_i ~ N(0, e^theta P_i); a noise-variance map; a
 * mask), as a table compiled into the header -- `static const double P[N + 1] = {...};`, which
 * ElementwiseModel.from_source(name, source, constants={"P": array}) writes for you -- or as a formula in i: what a closure of
 * the reference's SimpleMuseProblem would capture.  A model that does not need it ignores it.
 *
 * RUN-TIME constants (round 4).  A table compiled into the header fixes its values at build time: a new spectrum is a new
 * header, a 40-second build and a library of its own.  A header that says
 *     #define MUSE_MODEL_NCONST 2                      (before including this file; at most MUSE_MODEL_MAX_CONST)
 * may instead read  muse_const(k, i),  k < MUSE_MODEL_NCONST:  element i of constant vector k as the caller last set it --
 * muse_set_constants(ctx, k, values, count) on the engine (muse_hip.h), mo_set_constants on the CPU checker -- and 1.0 for
 * i >= count (the pad element and the phantom slots, as the compiled tables do) and while the vector has not been set (the
 * engine's contract check evaluates the functions before any constant exists).  The values live in device memory and are read
 * through one pointer per vector, and the pointers travel WITH EVERY LAUNCH (round 5: in its kernel-argument block, which
 * muse_const reads through the kernarg segment pointer) -- contexts of one library with different constants may have launches in
 * flight at the same time; only the host-side evaluation (muse_model_eval, the contract check) goes through one set per process.
 * ElementwiseModel.from_source(name, source, runtime_constants=["P", ...]) writes the #define and an accessor P(i) per name.
 *
 * Requirements the engine checks when a context is created (it evaluates the functions on the host):
 *     muse_model_grad(iv, 0, 0, &acc, N) == 0 leaving acc as it was, and muse_model_score_term(0, 0, N) == 0
 *         (vectors are padded to an even length with one zero element, which must not contribute).
 * Nothing differentiates the header: that muse_model_grad IS the derivative of the objective term and that muse_model_score_term
 * IS its B is the author's statement -- museinference_jl_amd.check_model_consistency(prob, theta) checks both against finite
 * differences of logLike through the problem's own operators (what AD guarantees in the reference, src/simple.jl:84-85).
 *
 * SECOND DERIVATIVES (round 4, optional).  The implicit-differentiation get_H! (src/muse.jl:335-405; muse_implicit_H_* of
 * muse_hip.h) differentiates the gradients once more: the reference does so by nested AD, a header says them.  A header that
 * says   #define MUSE_MODEL_SECOND 1   also defines, with o_i(x, z) = 1/2 [A(x, z) + iv B(x, z)] the element's objective term,
 *     MUSE_MODEL_FN void   muse_model_second(double iv, double x, double z, double* ozz, double* ozx, double* bz, double* bx, long i);
 *         *ozz = d2 o / dz2,  *ozx = d2 o / dz dx,  *bz = dB / dz,  *bx = dB / dx        (finite at x = z = 0, i >= N)
 *     MUSE_MODEL_FN double muse_model_dx_dsd(double sd, double n1, double n2, long i);
 *         d x / d sd of muse_model_sample at fixed normals (the reference re-draws x(theta) from a copy of the rng, src/muse.jl:353-371)
 * from which the engine forms, elementwise (k = the element's block, t_i = dx_i / dtheta_k = 1/2 sd_k dx/dsd),
 *     Hessian_z logLike w        = -ozz_i w_i                      (src/muse.jl:373-379; CG as in the reference although it is diagonal)
 *     d/dtheta_k grad_z logLike  = 1/2 iv_k bz_i                   (:361-365)
 *     d/dtheta_k grad_z logLike(x(theta), zhat, theta0) = -ozx_i t_i      (:366-371)
 *     H1[k][k] = 1/2 iv_k sum_{i in k} bx_i t_i                    (:353-358)
 * (the funnel: ozz = 1 + iv, ozx = -1, bz = 2 z, bx = 0, dx/dsd = n1).  Without MUSE_MODEL_SECOND the implicit entries refuse
 * the model and get_H! runs by finite differences (muse_fd_*: model-agnostic).  muse_model_eval of muse_hip.h evaluates the
 * header's functions on the host for one element -- what check_model_consistency differentiates numerically.
 * With MUSE_IMPLICIT_PL_JACOBI (muse_hip.h; of both families) CG is preconditioned by that diagonal, c_i = r_i / (-ozz_i): one
 * iteration solves a column.  That relies on ozz having ONE sign over the run (A negative definite: ozz > 0 at every MAP, as CG
 * itself does).  The kernel treats ozz_i = 0 as a phantom slot -- the pad element and the slots behind the vector are such -- so a
 * header that says ozz = 0 on a real element gets c_i = 0 there, not inf: that component of the solve is then simply never updated.
 *
 * TWO PARAMETERS PER BLOCK (round 6: location-type parameters).  In the family above a block has ONE parameter, the log-variance
 * of one Gaussian factor, and the engine knows how it enters: through exp(theta/2) in the draw, exp(-theta) in the objective,
 * 1/2 (iv sum B - n) in the score.  A header that says
 *     #define MUSE_MODEL_PAIR 1                        (before including this file)
 * states all of that itself, for blocks with TWO parameters acting on the same elements -- a mean AND a log-variance, a slope and a
 * scale, ...: ntheta = 2 K (at most MUSE_MAX_THETA = 8), the N elements in K contiguous equal blocks, block k's parameters
 * a_k = theta[k] and b_k = theta[K + k], and with c_k[0..3] FOUR coefficients the header forms from them,
 *
 *     -logLike(x, z, theta) = 1/2 sum_i o(c_k(i); x_i, z_i) + 1/2 sum_k n_k C(a_k, b_k)
 *     (x_i, z_i) ~ P(x, z | theta):  a function of c_k(i)[0], c_k(i)[1] and two independent standard normals
 *
 *     MUSE_MODEL_FN double muse_model_coefs(double a, double b, double* c);
 *         fills c[0..3] and returns C(a, b).  Evaluated on the host, once per theta; exponentials through muse_model_exp(x), the
 *         engine's fixed-sequence exp (the CPU checker evaluates the same sequence), every other operation an IEEE + - * / sqrt, fma
 *     MUSE_MODEL_FN void   muse_model_sample(const double* c, double n1, double n2, double* z, double* x, long i);
 *         the joint draw; may read c[0] and c[1] ONLY (a finite-difference get_H! re-draws at perturbed parameters and
 *         carries just those two per block)
 *     MUSE_MODEL_FN double muse_model_grad(const double* c, double x, double z, double* acc, long i);
 *         returns d(1/2 o)/dz_i and ADDS o(c; x, z) to *acc
 *     MUSE_MODEL_FN void   muse_model_score_terms(const double* c, double x, double z, double* t0, double* t1, long i);
 *         the element's terms of the block's TWO sums S0 = sum t0, S1 = sum t1
 *     MUSE_MODEL_FN void   muse_model_score(const double* c, double S0, double S1, double n, double* ga, double* gb);
 *         *ga = d logLike / d a_k, *gb = d logLike / d b_k from the block's coefficients, sums and element count
 *         (the d/d theta of the constant term included)
 * The pad element of an odd-length vector and the phantom slots behind it are given ZERO coefficients (a location parameter has a
 * gradient at x = z = 0): with c = {0, 0, 0, 0} and x = z = 0, muse_model_grad must return 0 leaving *acc as it was and
 * muse_model_score_terms must give 0, 0 -- the engine checks that when a context is created.
 * models/normal_mean_var.h is the shipped member: z_i ~ N(mu_k, e^tau_k), x_i ~ N(z_i, 1); c = {mu, e^(tau/2), e^-tau, 0}, C = tau,
 * o = (x - z)^2 + e^-tau (z - mu)^2, t0 = z - mu, t1 = (z - mu)^2, ga = e^-tau S0, gb = 1/2 (e^-tau S1 - n).
 * Everything of the C ABI applies -- batched maps in every placement (register/LDS resident, streaming, workgroup clusters, an
 * element split), multi-map launches, lanes, the native muse! loops (muse_run, muse_run_device: the step between two iterations
 * calls muse_model_coefs on the device -- the same statements as on the host, the same bits --, muse_run_sharded), both exchanges
 * between ranks, the finite-difference get_H! -- except more than MUSE_MAX_THETA parameters, and the implicit-differentiation get_H!
 * for a header that states its second derivatives:
 *
 * SECOND DERIVATIVES OF THE TWO-PARAMETER FAMILY (optional).  A header that says
 *     #define MUSE_MODEL_PAIR_SECOND 1                 (names of their own: MUSE_MODEL_SECOND / muse_model_second are the one-parameter
 *                                                       family's, with another signature)
 * also defines, with g = d(1/2 o)/dz the gradient, sa = -1/2 do/da and sb = -1/2 do/db the element's full score terms -- derivatives
 * in a and b taken THROUGH the coefficients and written in the coefficients, as the score is --,
 *     MUSE_MODEL_FN void muse_model_pair_second(const double* c, double x, double z, double* ozz, double* ozx, double* gza, double* gzb,
 *                                               double* sxa, double* sxb, long i);
 *         *ozz = dg/dz, *ozx = dg/dx, *gza = dg/da, *gzb = dg/db, *sxa = d sa / dx, *sxb = d sb / dx
 *     MUSE_MODEL_FN void muse_model_pair_dx(const double* c, double n1, double n2, double* xa, double* xb, long i);
 *         dx/da, dx/db of muse_model_sample at fixed normals (reads c[0], c[1] only, like the draw)
 * both finite for c = {0, 0, 0, 0} at x = z = 0 and for i >= N (checked when a context is created).  The engine forms, elementwise at
 * (x, zhat, theta0), for column j of H -- block j mod K, parameter q = a for j < K and b otherwise --
 *     Hessian_z logLike w = -ozz_i w_i,     d/dp grad_z logLike = -gzp_i,     d/dq grad_z logLike(x(theta), zhat, theta0) = -ozx_i xq_i,
 *     H1[p][j] = sum_{i in the column's block} sxp_i xq_i   for p that block's two parameters, 0 for every other p
 * (src/muse.jl:353-379), and muse_implicit_H_* accept the library (muse_model_has_second() = 1).  models/offset_noise.h is the shipped
 * member: z_i ~ N(0, 1), x_i ~ N(z_i + mu_k, e^tau_k); ozz = 1 + iv, ozx = -iv, gza = sxa = iv, gzb = sxb = iv (x - z - mu), xa = 1,
 * xb = 1/2 sd n2.  (For normal_mean_var's terms: ozz = 1 + iv, ozx = -1, gza = -iv, gzb = -iv (z - mu), sxa = sxb = 0, xa = 1,
 * xb = 1/2 sd n1; models/normal_mean_var.h itself states none and runs get_H! by finite differences.)
 * museinference_jl_amd.ElementwiseModel.from_pair_expressions writes both functions from the model's terms; muse_model_eval_pair_second
 * of muse_hip.h evaluates them on the host, which is what check_model_consistency differentiates numerically.
 *
 * EXPONENTIALS.  The per-element functions of the elementwise families may call  muse_model_exp(x)  -- and nothing else beyond
 * + - * / sqrt fma: no log, no pow, no trigonometric function --:
 *     one-parameter family:  muse_model_sample, muse_model_grad, muse_model_score_term, muse_model_second, muse_model_dx_dsd
 *     two-parameter family:  muse_model_coefs (as before), muse_model_sample, muse_model_grad, muse_model_score_terms,
 *                            muse_model_score, muse_model_pair_second, muse_model_pair_dx
 * (a response header, MUSE_MODEL_RESPONSE below, may not).  What lets a latent enter through its exponential per element and per
 * evaluation: x_i ~ N(0, e^z_i) (models/stochastic_volatility.h), x_i ~ N(2 (e^(z_i/2) - 1), 1) (models/lognormal_obs.h).  The macro
 * is defined by whoever includes the header, and resolves to
 *     on the host (muse_engine.cpp: the contract check, muse_model_eval, muse_model_coefs once per theta)   muse::muse_exp, csrc/step.hpp:
 *         fdlibm's reduction and polynomial as one fixed sequence of IEEE operations, below 1 ulp;
 *     in the CPU checker (oracle/muse_oracle.c)   mo_exp: that sequence restated;
 *     in device code, in muse_model_coefs (the step of the loop kernel)   muse::muse_exp;
 *     in device code, in every other function   muse::model_exp, csrc/model_math.hpp: the same reduction and polynomial as a
 *         branch-free body -- the quotient by a refined reciprocal with one fused residual correction (the correctly rounded quotient,
 *         as the IEEE division gives), the scaling by ldexp (one rounding, where the two-step product of muse_exp has one), the
 *         special results selected at the end --
 * and all four return THE SAME BITS for every double argument: NaN, +-inf, +-0, both cut-offs (above 709.78... +inf, below
 * -745.13... +0) and subnormal results included (tests/test_gpu_model_exp.py compares the device's with the checker's over every
 * exponent boundary).  A plain compile of the header by itself gets libm's exp (below).  One call costs about thirty double-precision
 * operations: share it among the values of a function body (e^(z/2) is h' and, doubled, h), as the generator does
 * (museinference_jl_amd.symbolic: `exp` in the terms of from_expressions / from_pair_expressions).
 *
 * A RESPONSE BEHIND THE STENCIL OPERATOR (the coupled family).  The three families above are elementwise.  A header that says
 *     #define MUSE_MODEL_RESPONSE 1                    (before including this file)
 * states instead the pointwise response of the coupled stencil model (MUSE_MODEL_SMOOTH of muse_hip.h with run-time weights, noise
 * map and mask):  z_i ~ N(0, e^theta_k),  u = A z the periodic (w1, w0, w1) stencil,
 *     x_i = phi(u_i; p) + sd_i n_i   where the element is observed,
 * and the whole of the header is
 *     #define MUSE_MODEL_NAME "saturating_response"
 *     MUSE_MODEL_FN void   muse_model_response(double u, const double* p, double* phi, double* dphi);
 *         *phi = phi(u; p) and *dphi = d phi / d u from ONE function, so that the two may share sub-expressions; p[0] and p[1] are
 *         two run-time numbers of the context (muse_set_link of muse_hip.h; (0, 0) until they are set), uniform over a launch
 *     #define MUSE_MODEL_RESPONSE_SECOND 1             (optional)
 *     MUSE_MODEL_FN double muse_model_response_second(double u, const double* p);
 *         d2 phi / d u2: what the implicit-differentiation get_H! of this family needs (muse_model_has_second() = 1 with it; without
 *         it the implicit entries refuse the library and get_H! runs by finite differences)
 * under the rules of every family: plain C, doubles only, IEEE + - * / sqrt fma only, finite for every finite u -- u = 0 included,
 * which the engine evaluates on the host when a context is created.  There is no element index: what varies per element travels in
 * x, in the noise map and in the mask (muse_set_noise).  -logLike = 1/2 sum_i omega_i (x_i - phi(u_i))^2 + 1/2 sum_i e^-theta_k z_i^2 +
 * 1/2 sum_k n_k theta_k; its gradient in z is e^-theta z - A' (omega phi'(u) r); the score is the stencil model's.  The family cannot
 * be combined with MUSE_MODEL_PAIR or MUSE_MODEL_NCONST: the constant slots of a launch carry the noise vectors.  Such a library
 * holds the model under MUSE_MODEL_USER, runs in the streaming and cluster placements as MUSE_MODEL_SMOOTH does, takes
 * muse_set_stencil / muse_set_noise / muse_set_link, and muse_model_eval reads (iv, sd) as (p[0], p[1]) and x as u:
 * out[0..2] = phi, phi', phi'' (NaN without MUSE_MODEL_RESPONSE_SECOND), zeros behind.  models/poly_response.h (the cubic of
 * muse_set_link, in its expressions: the built-in link's bits) and models/saturating_response.h (u / sqrt(1 + (p0 u)^2)) are the
 * shipped members; museinference_jl_amd.ResponseModel.from_expression writes phi' and phi'' from phi.
 */
#ifndef MUSE_MODEL_H
#define MUSE_MODEL_H
#ifndef MUSE_MODEL_FN
#define MUSE_MODEL_FN static inline
#endif
#define MUSE_MODEL_MAX_CONST 4
#ifdef MUSE_MODEL_RESPONSE
#ifdef MUSE_MODEL_PAIR
#error "MUSE_MODEL_RESPONSE cannot be combined with MUSE_MODEL_PAIR: the response family is the stencil model's, one parameter per block"
#endif
#ifdef MUSE_MODEL_NCONST
#error "MUSE_MODEL_RESPONSE cannot be combined with MUSE_MODEL_NCONST: the constant slots of a launch carry the stencil model's noise vectors"
#endif
#endif
#ifndef muse_model_exp
/* The exponential of a header's functions (EXPONENTIALS above).  The engine and its CPU checker define it before they include the
 * header -- one fixed sequence of IEEE operations, the same bits on host, device and checker; a plain compile of the header by
 * itself (a syntax check, an editor) gets libm's. */
#include <math.h>
#define muse_model_exp(x) exp(x)
#endif
#ifdef MUSE_MODEL_NCONST
#if MUSE_MODEL_NCONST < 1 || MUSE_MODEL_NCONST > MUSE_MODEL_MAX_CONST
#error "MUSE_MODEL_NCONST must be in [1, MUSE_MODEL_MAX_CONST]"
#endif
/* the vectors: defined once per program that compiles a model header (the engine's muse_engine.cpp / muse_kernels.hip,
 * the checker's muse_oracle.c) */
#ifdef __cplusplus
extern "C" {
#endif
extern const double* muse_host_consts[MUSE_MODEL_MAX_CONST];
extern long muse_host_const_len[MUSE_MODEL_MAX_CONST];
#ifdef __cplusplus
}
#endif
MUSE_MODEL_FN double muse_const(int k, long i) {
#if defined(__HIP_DEVICE_COMPILE__)
    /* the launch's own vectors: every kernel of the engine takes its argument block (csrc/args.hpp, BatchArgs) as its FIRST
     * parameter, and MUSE_KERNARG_CONSTS (csrc/user_model.hpp) is the offset of {pointers[4], lengths[4]} in it -- uniform
     * scalar loads from the kernel-argument segment, no state shared between launches */
    const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr() + MUSE_KERNARG_CONSTS;
    const long n = ((const long*)(ka + MUSE_MODEL_MAX_CONST * sizeof(const double*)))[k];
    return i < n ? ((const double* const*)ka)[k][i] : 1.0;
#else
    const long n = muse_host_const_len[k];
    return i < n ? muse_host_consts[k][i] : 1.0;
#endif
}
#endif
#endif
