// models.hpp -- the compiled-in models, the storage policies (placements) and the HagerZhang point type (see muse_kernels.hip).
#pragma once
#include <type_traits>

#include "step.hpp"
#include "user_model.hpp"
#include "vec.hpp"

namespace muse {

// ------------------------------------------------------------------------------------------------
// Models.  grad() returns d(-logLike)/dz_i and adds the element's share of -2 logLike (without the
// constant) to facc; the score is assembled from per-block sums of score_term().
template <int MAXB = kMaxTheta>
__device__ __forceinline__ int block_of(const BatchArgs& a, int i) {
    int k = 0;
#pragma unroll
    for (int b = 1; b < MAXB; ++b) k += (i >= a.bnd32[b]) ? 1 : 0;  // bnd32[b] = INT_MAX for b >= ntheta
    return k;
}

// (block_of_big, the big tier's block index by arithmetic: step.hpp -- host and device, checked exhaustively on the host)

template <int MAXB_>
struct FunnelModel {  // z_i ~ N(0, e^theta_k), x_i ~ N(z_i, 1)
    static constexpr int MAXB = MAXB_;
    static constexpr bool kPair = false;   // one parameter per block: the coefficients are plain doubles
    using SCoef = double; using GCoef = double;
    static constexpr bool kStencil = false;
    static constexpr int kId = MUSE_MODEL_FUNNEL;
    __device__ static __forceinline__ void sample(double sd, double n1, double n2, double& z, double& x, int) {
        z = sd * n1;
        x = z + n2;
    }
    __device__ static __forceinline__ double grad(double iv, double x, double z, double& facc, int) {
        const double r = x - z, t = iv * z;
        facc = fma(t, z, fma(r, r, facc));
        return t - r;
    }
    __device__ static __forceinline__ double score_term(double, double z, int) { return z * z; }
};
struct NoiseModel {  // z_i ~ N(0,1), x_i ~ N(z_i, e^theta)
    static constexpr int MAXB = 1;
    static constexpr bool kPair = false;   // one parameter per block: the coefficients are plain doubles
    using SCoef = double; using GCoef = double;
    static constexpr bool kStencil = false;
    static constexpr int kId = MUSE_MODEL_NOISE;
    __device__ static __forceinline__ void sample(double sd, double n1, double n2, double& z, double& x, int) {
        z = n1;
        x = n1 + sd * n2;
    }
    __device__ static __forceinline__ double grad(double iv, double x, double z, double& facc, int) {
        const double r = x - z, t = iv * r;
        facc = fma(z, z, fma(t, r, facc));
        return z - t;
    }
    __device__ static __forceinline__ double score_term(double x, double z, int) {
        const double r = x - z;
        return r * r;
    }
};
template <int MAXB_>
struct SmoothModel {  // z as funnel, x = A z + n, A = periodic (1/4, 1/2, 1/4); streaming policy only
    static constexpr int MAXB = MAXB_;
    static constexpr bool kPair = false;   // one parameter per block: the coefficients are plain doubles
    using SCoef = double; using GCoef = double;
    static constexpr bool kStencil = true;
    static constexpr int kId = MUSE_MODEL_SMOOTH;
    static constexpr bool kNoise = false;   // unit noise variance, every element observed
    static constexpr bool kLink = false;    // x = A z + n: no response function behind the operator
    __device__ static __forceinline__ double w0() { return 0.5; }
    __device__ static __forceinline__ double w1() { return 0.25; }
    __device__ static __forceinline__ double score_term(double, double z, int) { return z * z; }
};
// The same model with the operator's weights as context state (muse_set_stencil): A = periodic (w1, w0, w1), read as wavefront-uniform
// scalars from the launch's own kernel-argument block (args.hpp, BatchArgs::taps), so that contexts with different weights may have
// launches in flight together.  Every stencil expression is stencil_apply's, in the built-in's shape and operand order: at
// (1/2, 1/4) these kernels give the built-in's bits.
typedef __attribute__((address_space(4))) const double* kernarg_f64;
template <int MAXB_>
struct SmoothTapsModel {
    static constexpr int MAXB = MAXB_;
    static constexpr bool kPair = false;
    using SCoef = double; using GCoef = double;
    static constexpr bool kStencil = true;
    static constexpr int kId = MUSE_MODEL_SMOOTH;
    static constexpr bool kNoise = false;
    static constexpr bool kLink = false;
    __device__ static __forceinline__ double w0() { return ((kernarg_f64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, taps) / 8]; }
    __device__ static __forceinline__ double w1() { return ((kernarg_f64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, taps) / 8 + 1]; }
    __device__ static __forceinline__ double score_term(double, double z, int) { return z * z; }
};
// ... and with the noise as context state too (muse_set_noise): x_i = (A z)_i + s_i n2_i, -logLike = 1/2 sum_i omega_i r_i^2 + ...,
// omega_i = 1 / sd_i^2 and s_i = sd_i where the element is observed, both 0 where it is masked.  The two vectors ([ld], the pad
// element 0) are the launching context's; their pointers travel in the kernarg-only tail of the argument block, in the first two
// slots of BatchArgs::consts, which the library of the built-in models does not use otherwise (a launch that carries no noise
// carries the weights (1/2, 1/4) of the built-in stencil in BatchArgs::taps: the engine's set_launch_constants).  omega enters
// every expression through noise_weigh below; at omega = s = 1 these kernels give SmoothTapsModel's bits.
typedef __attribute__((address_space(4))) const int64_t* kernarg_i64;
template <int MAXB_>
struct SmoothNoiseModel : SmoothTapsModel<MAXB_> {
    static constexpr bool kNoise = true;
    // k = 0: omega, k = 1: s
    __device__ static __forceinline__ const double* noise_ptr(int k) {
        return (const double*)((kernarg_i64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, consts) / 8 + k];
    }
    __device__ static __forceinline__ int64_t noise_ld() { return ((kernarg_i64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, ld) / 8]; }
};
// ... and with a pointwise response behind the operator (muse_set_link): u = A z, x_i = phi(u_i) + s_i n2_i,
// phi(u) = u + a2 u^2 + a3 u^3, -logLike = 1/2 sum_i omega_i r_i^2 + ..., r = x - phi(A z), grad_z = e^-theta z - A' (omega phi'(u) r).
// The two coefficients are the launching context's, wavefront-uniform scalars read from the kernarg-only tail of the argument block
// (BatchArgs::link, behind the weights in the place of the constants' lengths), so contexts with different links may have launches
// in flight together.  phi enters through link_value, phi' through link_slope / link_rho below, each the identity (1) for every
// model without a link.  Every expression is written so that at (a2, a3) = (0, 0) it rounds as SmoothNoiseModel's does:
// fma(u h, u, u) with h = fma(a3, u, a2) = 0 is u, phi' = fma(u, fma(3 a3, u, 2 a2), 1) is 1, q 1 = q -- these kernels then give the
// bits of the context without a link (for finite u: z is finite wherever the solver evaluates).
template <int MAXB_>
struct SmoothLinkModel : SmoothNoiseModel<MAXB_> {
    static constexpr bool kLink = true;
    __device__ static __forceinline__ double a2() { return ((kernarg_f64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, link) / 8]; }
    __device__ static __forceinline__ double a3() { return ((kernarg_f64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, link) / 8 + 1]; }
};
#if defined(MUSE_USER_MODEL_HEADER) && defined(MUSE_MODEL_RESPONSE)
// ... and with the response a USER'S header states (include/muse_model.h, MUSE_MODEL_RESPONSE): phi and phi' from
// muse_model_response(u, p, .), p the same two wavefront-uniform scalars of the launch (BatchArgs::link).  kLink selects every fork
// SmoothLinkModel takes -- stencil_pairs, stencil_grad_linked, the sampler's second pass, loglike_kernel, the finish kernel --, whose
// text knows phi through link_value / link_slope / link_rho alone; those three call the header for this type.  The pair is handed
// over as two values in registers, so that after inlining a header that restates the built-in's expressions IS the built-in's
// expression tree: the same rounded operations, the same bits.
template <int MAXB_>
struct UserResponseModel : SmoothNoiseModel<MAXB_> {
    static constexpr bool kLink = true;
    static constexpr bool kResponse = true;
    __device__ static __forceinline__ double p0() { return ((kernarg_f64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, link) / 8]; }
    __device__ static __forceinline__ double p1() { return ((kernarg_f64)__builtin_amdgcn_kernarg_segment_ptr())[offsetof(BatchArgs, link) / 8 + 1]; }
    __device__ static __forceinline__ void response(double u, double& phi, double& dphi) {
        const double p[2] = {p0(), p1()};
        muse_model_response(u, p, &phi, &dphi);
    }
#ifdef MUSE_MODEL_RESPONSE_SECOND   // (the operand of the implicit-differentiation get_H!, the response fork of Solver::run_implicit)
    __device__ static __forceinline__ double second(double u) {
        const double p[2] = {p0(), p1()};
        return muse_model_response_second(u, p);
    }
#endif
};
#endif
template <class Model, class = void>
struct has_response : std::false_type {};
template <class Model>
struct has_response<Model, std::void_t<decltype(Model::kResponse)>> : std::true_type {};
template <class Model>
constexpr bool response_model() { return has_response<Model>::value; }
template <class Model>
constexpr bool link_model() {
    if constexpr (Model::kStencil) return Model::kLink;
    else return false;
}
// phi(u) = u + u^2 (a2 + a3 u): three rounded operations beside the load of the coefficients
// (a user's response: the header's, of whose two results the unused one is dead code behind the inlining)
template <class Model>
__device__ __forceinline__ double link_value(double u) {
    if constexpr (response_model<Model>()) {
        double phi, dphi;
        Model::response(u, phi, dphi);
        return phi;
    } else
    if constexpr (link_model<Model>()) return fma(u * fma(Model::a3(), u, Model::a2()), u, u);
    else return u;
}
// phi'(u) = 1 + u (2 a2 + 3 a3 u) (the two products of the coefficients are scalar work)
template <class Model>
__device__ __forceinline__ double link_slope(double u) {
    if constexpr (response_model<Model>()) {
        double phi, dphi;
        Model::response(u, phi, dphi);
        return dphi;
    } else
    if constexpr (link_model<Model>()) return fma(u, fma(3.0 * Model::a3(), u, 2.0 * Model::a2()), 1.0);
    else return 1.0;
}
// rho = q phi'(u), the gradient's operand from the weighted residual q = omega r: gradient t - stencil_apply(rho_m, rho_0, rho_p);
// the objective's share stays fma(t, z0, fma(q0, r0, facc)) -- q, not rho.  q itself for every model without a link.
template <class Model>
__device__ __forceinline__ double link_rho(double q, double u) {
    if constexpr (link_model<Model>()) return q * link_slope<Model>(u);
    else return q;
}
template <class Model>
constexpr bool noise_model() {
    if constexpr (Model::kStencil) return Model::kNoise;
    else return false;
}
// rho = omega r, the weighted residual of a stencil model with run-time noise -- and r itself for every other model, whose
// code therefore does not change: gradient t - stencil_apply(rho_m, rho_0, rho_p), objective share fma(t, z0, fma(rho0, r0, facc))
template <class Model>
__device__ __forceinline__ double noise_weigh(double omega, double r) {
    if constexpr (noise_model<Model>()) return omega * r;
    else return r;
}
// ... and the residual itself as the expressions above may see it: r where the element is observed, 0 where it is masked
// (omega = 0), whatever the data vector holds there.  r = x - (A z) of a masked element is formed from an x that the model never
// reads -- NaN and inf are the usual fill of masked pixels -- and 0 * NaN is NaN, so the product alone would not drop it: the
// select does, before noise_weigh and before the objective's fma(rho0, r0, .).  Where omega != 0 it returns r unchanged, so
// at omega = 1 the bits are SmoothTapsModel's; for every other model it is r.
template <class Model>
__device__ __forceinline__ double noise_residual(double omega, double r) {
    if constexpr (noise_model<Model>()) return omega != 0.0 ? r : 0.0;
    else return r;
}
// One of the two noise vectors as a pass reads it (K = 0: omega, K = 1: s): a range-checked descriptor over the context's vector,
// made from the kernel-argument segment where the pass begins (scalar work, nothing held across the kernel).  Read-only inside a
// launch, so neighbours' elements need no coherent loads.  For the models without run-time noise: no state, the value 1.
template <class Model, int K, bool ON = noise_model<Model>()>
struct NoiseVec {
    __device__ __forceinline__ double get1(int) const { return 1.0; }
    __device__ __forceinline__ void own_pair(int, double& a, double& b) const { a = 1.0; b = 1.0; }
    __device__ __forceinline__ double get(int, int) const { return 1.0; }
};
template <class Model, int K>
struct NoiseVec<Model, K, true> {
    rsrc_t rsrc;
    mutable double c1;
    __device__ __forceinline__ NoiseVec() : rsrc(make_rsrc(Model::noise_ptr(K), Model::noise_ld() * 8)) {}
    __device__ __forceinline__ double get1(int i) const { return load_f64(rsrc, i); }
    __device__ __forceinline__ void own_pair(int i0, double& a, double& b) const { load_f64x2(rsrc, i0, a, b); }
    // element loop (vec.hpp, for_elems): the thread's pair with one 16-byte load at the even element, its second half at the odd one
    __device__ __forceinline__ double get(int jj, int i) const {
        if ((jj & 1) == 0) {
            double d0;
            load_f64x2(rsrc, i, d0, c1);
            return d0;
        }
        return c1;
    }
};
// (A z)_i of a stencil model from the element and its two neighbours: w1 (zl + zr) + w0 z0, the product rounded, then ONE fma
// (stencil_fma: from the neighbours' sum, for a caller that loads the centre element behind it)
template <class Model>
__device__ __forceinline__ double stencil_fma(double zlr, double z0) {
    if constexpr (Model::kStencil) return fma(Model::w1(), zlr, Model::w0() * z0);
    else return 0.0;   // (never called: the elementwise models have no operator)
}
template <class Model>
__device__ __forceinline__ double stencil_apply(double zl, double z0, double zr) { return stencil_fma<Model>(zl + zr, z0); }

// Coefficients of an element's block for the models with TWO parameters per block (include/muse_model.h, MUSE_MODEL_PAIR): what the
// draw takes (c[0], c[1]) and what the objective takes (all four).  The tables hold a block's coefficients side by side:
// ThetaSet::sd and ::iv read as ONE array of [block][4] (pair_table), a sampling entry (SampleSd) as [block][2].
// One block (the tier of two components): plain values -- they are workgroup-uniform and live in scalar registers; the pad element
// gets zeros.  Several blocks: a POINTER to the block's record in LDS and the element's validity -- four doubles per element in
// vector registers (two elements of a pair in flight) were 500 spilled registers in the LDS-resident kernel; the model's functions
// read what they use where they use it, and the pad element's contribution is dropped behind the call.
struct PairS { double c[2]; };
struct PairGv { double c[4]; };
struct PairGp { const double* p; bool valid; };
__host__ __device__ __forceinline__ const double* pair_table(const ThetaSet& t) { return &t.sd[0]; }
static_assert(offsetof(ThetaSet, iv) == offsetof(ThetaSet, sd) + kMaxTheta * sizeof(double), "sd and iv as one [block][4] table");

#if defined(MUSE_USER_MODEL_HEADER) && !defined(MUSE_MODEL_RESPONSE)   // (a response header: UserResponseModel above, no elementwise model)
#ifndef MUSE_MODEL_PAIR
template <int MAXB_>
struct UserModel {  // include/muse_model.h: the three functions of the user's header behind the elementwise model concept
    static constexpr int MAXB = MAXB_;
    static constexpr bool kStencil = false;
    static constexpr int kId = MUSE_MODEL_USER;
    static constexpr bool kPair = false;
    using SCoef = double; using GCoef = double;
    __device__ static __forceinline__ void sample(double sd, double n1, double n2, double& z, double& x, int i) {
        muse_model_sample(sd, n1, n2, &z, &x, (long)i);
    }
    __device__ static __forceinline__ double grad(double iv, double x, double z, double& facc, int i) {
        return muse_model_grad(iv, x, z, &facc, (long)i);
    }
    __device__ static __forceinline__ double score_term(double x, double z, int i) { return muse_model_score_term(x, z, (long)i); }
#ifdef MUSE_MODEL_SECOND  // (include/muse_model.h: the operands of the implicit-differentiation get_H!, Solver::run_implicit)
    __device__ static __forceinline__ void second(double iv, double x, double z, double& ozz, double& ozx, double& bz, double& bx, int i) {
        muse_model_second(iv, x, z, &ozz, &ozx, &bz, &bx, (long)i);
    }
    // dx_i / dtheta_k at fixed normals: sd = exp(theta / 2)
    __device__ static __forceinline__ double dx_dtheta(double sd, double n1, double n2, int i) {
        return 0.5 * (sd * muse_model_dx_dsd(sd, n1, n2, (long)i));
    }
#endif
};
#else
// A header of the two-parameter family (include/muse_model.h, "TWO PARAMETERS PER BLOCK"): K = ntheta / 2 blocks, block k's parameters
// theta[k] and theta[K + k], four coefficients per block, two block sums per block, the score assembled by the header.
template <int MAXB_>
struct UserModel {
    static_assert(MAXB_ % 2 == 0, "two parameters per block");
    static constexpr int MAXB = MAXB_;
    static constexpr bool kStencil = false;
    static constexpr int kId = MUSE_MODEL_USER;
    static constexpr bool kPair = true;
    using SCoef = PairS;
    using GCoef = typename std::conditional<MAXB_ == 2, PairGv, PairGp>::type;
    __device__ static __forceinline__ void sample(const PairS& c, double n1, double n2, double& z, double& x, int i) {
        muse_model_sample(c.c, n1, n2, &z, &x, (long)i);
    }
    __device__ static __forceinline__ double grad(const PairGv& c, double x, double z, double& facc, int i) {
        return muse_model_grad(c.c, x, z, &facc, (long)i);
    }
    __device__ static __forceinline__ void score_terms(const PairGv& c, double x, double z, double& t0, double& t1, int i) {
        muse_model_score_terms(c.c, x, z, &t0, &t1, (long)i);
    }
    __device__ static __forceinline__ double grad(const PairGp& c, double x, double z, double& facc, int i) {
        double a2 = facc;
        const double g = muse_model_grad(c.p, x, z, &a2, (long)i);
        facc = c.valid ? a2 : facc;     // (the pad element and the phantom slots: no contribution, whatever the model's location)
        return c.valid ? g : 0.0;
    }
    __device__ static __forceinline__ void score_terms(const PairGp& c, double x, double z, double& t0, double& t1, int i) {
        muse_model_score_terms(c.p, x, z, &t0, &t1, (long)i);
        t0 = c.valid ? t0 : 0.0;
        t1 = c.valid ? t1 : 0.0;
    }
    __device__ static __forceinline__ void score(const double* c, double s0, double s1, double n, double& ga, double& gb) {
        muse_model_score(c, s0, s1, n, &ga, &gb);
    }
#ifdef MUSE_MODEL_PAIR_SECOND  // (include/muse_model.h: the operands of the implicit-differentiation get_H!, Solver::run_implicit)
    // q[0..5] = {ozz, ozx, gza, gzb, sxa, sxb}; the pad element and the phantom slots: all zero (no contribution, a zero Hessian
    // entry that only ever multiplies a zero direction)
    __device__ static __forceinline__ void second(const PairGv& c, double x, double z, double* q, int i) {
        muse_model_pair_second(c.c, x, z, &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], (long)i);
    }
    __device__ static __forceinline__ void second(const PairGp& c, double x, double z, double* q, int i) {
        muse_model_pair_second(c.p, x, z, &q[0], &q[1], &q[2], &q[3], &q[4], &q[5], (long)i);
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k] = c.valid ? q[k] : 0.0;
    }
    // dx_i / da_k, dx_i / db_k at fixed normals, from the block's coefficients at the theta of the draw
    __device__ static __forceinline__ void dx(const PairGv& c, double n1, double n2, double& xa, double& xb, int i) {
        muse_model_pair_dx(c.c, n1, n2, &xa, &xb, (long)i);
    }
    __device__ static __forceinline__ void dx(const PairGp& c, double n1, double n2, double& xa, double& xb, int i) {
        muse_model_pair_dx(c.p, n1, n2, &xa, &xb, (long)i);
    }
#endif
};
#endif
#endif

// ------------------------------------------------------------------------------------------------
// Storage policies.
template <int T_, bool CLUSTER = false, int U_ = 4, bool COH = false, bool LDS_S = false>
struct PlaceStreaming {
    static constexpr bool kCoherent = COH;  // stencil model in a cluster: see vec.hpp, kCoherent
    static constexpr bool kLdsS = LDS_S;    // the search direction in LDS (vec.hpp, LdsMirror)
    static constexpr int T = T_, EPT = 0, U = U_;  // U pairs of a thread per trip of a streaming pass
    // two waves per SIMD: 2 workgroups of 256 threads (cluster mode sizes its grid from that) or 1 of 512 per CU,
    // i.e. a budget of 256 registers per lane
    static constexpr int kWavesPerEu = 2;
    static constexpr bool kResident = false, kXgLds = false, kCluster = CLUSTER;
    using VX = BufChunk<U_, COH>;
    using VG = VX; using VZ = VX;
    using VS = typename std::conditional<LDS_S, LdsMirror<U_, T_>, VX>::type;
    using VH = VX;
};
// CLUSTER (registers only): csize workgroups share one element, thread pairs (crank*T + tid) + j*csize*T -- the
// per-GPU share of a strongly scaled map, where a launch has fewer elements than the GPU has compute units.
template <int T_, int EPT_, bool XG_LDS, bool CLUSTER = false>
struct PlaceResident {
    static_assert(!(XG_LDS && CLUSTER), "the LDS layout addresses x and g by global element index");
    static constexpr int T = T_, EPT = EPT_, U = 1;
    static constexpr int kWavesPerEu = 1;  // no lower bound beyond the launch bounds
    static constexpr bool kResident = true, kXgLds = XG_LDS, kCluster = CLUSTER, kCoherent = false, kLdsS = false;
    using VX = typename std::conditional<XG_LDS, LdsVec, RegVec<2 * EPT_>>::type;
    using VG = VX;
    using VZ = RegVec<2 * EPT_>; using VS = RegVec<2 * EPT_>;
    using VH = BufVec2;  // history vectors and zhat in HBM: 16-byte accesses
};

struct HzPoint {
    double a, v, d;  // alpha, phi(alpha), dphi(alpha)
    int id;          // evaluation sequence number (0 = the point alpha=0)
};


}  // namespace muse
