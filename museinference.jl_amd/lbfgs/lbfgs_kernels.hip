// lbfgs_kernels.hip -- libmuse_lbfgs.so (include/muse_lbfgs.h): lock-step L-BFGS/HagerZhang for a batch of closure problems.
// The objective is the caller's (a torch closure, evaluated once per round for the whole [B, N] batch); everything between two
// evaluations runs here for all B problems in ONE launch, one workgroup per problem, all solver state in the caller's workspace.
//
// Workspace:  records [nprob] (Record: the suspended scalar machine, lbfgs_control.hpp, and the rho_i)
//             vectors [nprob][3 + 2 m][n] doubles: x, s (also q of the two-loop recursion), g_prev, dx_0 .. dx_{m-1}, dg_0 .. dg_{m-1}
// Rows have stride n: with odd n a row's base is only 8-byte aligned, so every access is one double (coalesced: lane l of a pass
// touches element l + k T of every vector, always the same elements -- a thread re-reads from memory only what it stored itself, and
// the threads of a workgroup meet only in the reductions).
// The workgroup size is a function of n alone and every reduction has a fixed shape (reduce.hpp: block_allreduce), so a problem's
// result depends on its own inputs only, not on the batch or its place in it.  No workgroup waits for another: no spin, no tag, no atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc/reduce.hpp"
#include "lbfgs_advance.hpp"
#include "../../include/muse_lbfgs.h"

namespace muse_lbfgs {

struct Record {
    Problem p;
    double rho[kM];
};
constexpr int kVectors = 3 + 2 * kM;
constexpr int kSmallT = 256, kLargeT = 1024;
constexpr int64_t kSmallMaxN = 4096;      // n <= this: 256 threads (up to 16 elements each); above: 1024

__host__ __device__ inline size_t records_bytes(int64_t nprob) { return ((size_t)nprob * sizeof(Record) + 255) / 256 * 256; }

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the record, field by field through v_readfirstlane: every field is workgroup-uniform and the machine's branches compile scalar
// (field by field, not as words: a copy through an array leaves the record in scratch memory)
__device__ __forceinline__ HzPoint load_point(const HzPoint& s) {
    return HzPoint{muse::uniform(s.a), muse::uniform(s.v), muse::uniform(s.d), uniform_i(s.id), 0};
}
__device__ __forceinline__ void load_problem(Problem& d, const Problem& s) {
    d.hz.P0 = load_point(s.hz.P0);
    d.hz.A = load_point(s.hz.A);
    d.hz.B = load_point(s.hz.B);
    d.hz.C = load_point(s.hz.C);
    d.hz.prev = load_point(s.hz.prev);
    d.hz.a0 = load_point(s.hz.a0);
    d.hz.b0 = load_point(s.hz.b0);
    d.hz.alphamax = muse::uniform(s.hz.alphamax);
    d.hz.cold = muse::uniform(s.hz.cold);
    d.hz.fail_alpha = muse::uniform(s.hz.fail_alpha);
    d.hz.c = muse::uniform(s.hz.c);
    d.hz.last_c = muse::uniform(s.hz.last_c);
    d.hz.alpha = muse::uniform(s.hz.alpha);
    d.hz.state = uniform_i(s.hz.state);
    d.hz.cont = uniform_i(s.hz.cont);
    d.hz.iter = uniform_i(s.hz.iter);
    d.hz.iterfinite = uniform_i(s.hz.iterfinite);
    d.hz.nid = uniform_i(s.hz.nid);
    d.hz.ok = uniform_i(s.hz.ok);
    d.f = muse::uniform(s.f);
    d.f_prev = muse::uniform(s.f_prev);
    d.gnorm = muse::uniform(s.gnorm);
    d.g_tol = muse::uniform(s.g_tol);
    d.gamma = muse::uniform(s.gamma);
    d.f_last = muse::uniform(s.f_last);
    d.gnorm_last = muse::uniform(s.gnorm_last);
    d.phase = uniform_i(s.phase);
    d.pseudo = uniform_i(s.pseudo);
    d.iterations = uniform_i(s.iterations);
    d.f_calls = uniform_i(s.f_calls);
    d.status = uniform_i(s.status);
    d.counter_f = uniform_i(s.counter_f);
    d.maxiter = uniform_i(s.maxiter);
    d.pad_ = 0;
}

template <int T>
struct DeviceVectors {
    const int tid;
    const int64_t n;
    const double* __restrict__ g;
    double* __restrict__ z;
    double *x, *s, *gp, *dx, *dg;     // dx + i n: pair i
    double* rho_g;                    // the record's rho_i (memory); sh_rho: their copy in LDS
    double *red, *sh_rho, *sh_alpha;
    int parity;

    __device__ __forceinline__ double sum1(double a) {
        double sm[1] = {a}, mx[1] = {0.0};
        muse::block_allreduce<T, 1, 0>(sm, mx, red, parity, tid);
        return sm[0];
    }
    __device__ __forceinline__ void intake(double& gs, double& absmax, double& nanc) {
        double sm[2] = {0.0, 0.0}, mx[1] = {0.0};
        for (int64_t e = tid; e < n; e += T) {
            const double ge = g[e];
            sm[0] += ge * s[e];
            sm[1] += ge != ge ? 1.0 : 0.0;
            mx[0] = muse::absmax(mx[0], ge);
        }
        muse::block_allreduce<T, 2, 1>(sm, mx, red, parity, tid);
        gs = sm[0];
        nanc = sm[1];
        absmax = mx[0];
    }
    __device__ __forceinline__ void start() {
        for (int64_t e = tid; e < n; e += T) {
            const double ge = g[e];
            s[e] = ge;
            gp[e] = ge;
        }
    }
    __device__ __forceinline__ void write_trial(double c) {
        for (int64_t e = tid; e < n; e += T) z[e] = x[e] + c * s[e];
    }
    __device__ __forceinline__ void step_to(double c) {
        for (int64_t e = tid; e < n; e += T) {
            const double xn = x[e] + c * s[e];
            x[e] = xn;
            z[e] = xn;
        }
    }
    __device__ __forceinline__ void pass_accept(double alpha, int slot, double& x_diff, double& dxdg, double& dgdg, double& dxg) {
        double sm[3] = {0.0, 0.0, 0.0}, mx[1] = {0.0};
        double* dxi = dx + slot * n;
        double* dgi = dg + slot * n;
        for (int64_t e = tid; e < n; e += T) {
            const double ge = g[e], xe = x[e];
            const double d = alpha * s[e];
            const double xn = xe + d;
            const double y = ge - gp[e];
            mx[0] = muse::absmax(mx[0], xn - xe);
            sm[0] += d * y;
            sm[1] += y * y;
            sm[2] += d * ge;
            x[e] = xn;
            dxi[e] = d;
            dgi[e] = y;
            gp[e] = ge;
            s[e] = ge;
        }
        muse::block_allreduce<T, 3, 1>(sm, mx, red, parity, tid);
        dxdg = sm[0];
        dgdg = sm[1];
        dxg = sm[2];
        x_diff = mx[0];
    }
    __device__ __forceinline__ double stage_down(double a, int i, int inext) {
        const double* dgi = dg + i * n;
        const double* dxn = dx + inext * n;
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double q = s[e] - a * dgi[e];
            s[e] = q;
            acc += dxn[e] * q;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double stage_down_last(double a, int i, double scale) {
        const double* dgi = dg + i * n;
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double y = dgi[e];
            const double q = s[e] - a * y;
            const double se = scale * q;
            s[e] = se;
            acc += y * se;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double stage_up(double coef, int i, int inext) {
        const double* dxi = dx + i * n;
        const double* dgn = dg + inext * n;
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double se = s[e] + dxi[e] * coef;
            s[e] = se;
            acc += dgn[e] * se;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double stage_up_last(double coef, int i) {
        const double* dxi = dx + i * n;
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double se = -(s[e] + dxi[e] * coef);
            s[e] = se;
            acc += g[e] * se;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double negate_first() {
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double se = -s[e];
            s[e] = se;
            acc += g[e] * se;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double steepest() {
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double ge = g[e];
            const double se = -ge;
            s[e] = se;
            acc += ge * se;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double rho(int i) const { return muse::uniform(sh_rho[i]); }
    __device__ __forceinline__ double alpha(int i) const { return muse::uniform(sh_alpha[i]); }
    // (one thread writes; the barrier orders the write before the other wavefronts' reads: no reduction lies between accept's rho_i and
    //  its first use.  alpha_i is read only in the second loop, at least one reduction -- a barrier -- after it was written)
    __device__ __forceinline__ void set_rho(int i, double v) {
        if (tid == 0) {
            sh_rho[i] = v;
            rho_g[i] = v;
        }
        __syncthreads();
    }
    __device__ __forceinline__ void set_alpha(int i, double v) {
        if (tid == 0) sh_alpha[i] = v;
    }
};

template <int T>
__global__ __launch_bounds__(T) void advance_kernel(char* ws, int64_t nprob, int64_t n, const double* __restrict__ f,
                                                    const double* __restrict__ g, double* __restrict__ z_eval) {
    __shared__ double red[2 * (T / 64) * 8];
    __shared__ double sh_rho[kM], sh_alpha[kM];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    Record* rec = reinterpret_cast<Record*>(ws) + b;
    if (uniform_i(rec->p.phase) == PH_DONE) return;   // a finished problem: its record and its z_eval row stay as they are
    if (tid < kM) sh_rho[tid] = rec->rho[tid];
    __syncthreads();
    Problem p;
    load_problem(p, rec->p);
    double* vec = reinterpret_cast<double*>(ws + records_bytes(nprob)) + (int64_t)b * kVectors * n;
    DeviceVectors<T> v{tid, n, g + (int64_t)b * n, z_eval + (int64_t)b * n, vec, vec + n, vec + 2 * n, vec + 3 * n, vec + (3 + kM) * n,
                       rec->rho, red, sh_rho, sh_alpha, 0};
    advance_problem(p, v, muse::uniform(f[b]));
    if (tid == 0) rec->p = p;
}

// the first evaluation point is z0 itself
template <int T>
__global__ __launch_bounds__(T) void begin_kernel(char* ws, int64_t nprob, int64_t n, const double* __restrict__ z0, double g_tol,
                                                  int maxiter, double* __restrict__ z_eval) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    Record* rec = reinterpret_cast<Record*>(ws) + b;
    double* vec = reinterpret_cast<double*>(ws + records_bytes(nprob)) + (int64_t)b * kVectors * n;
    for (int64_t e = tid; e < n; e += T) {
        const double ze = z0[(int64_t)b * n + e];
        vec[e] = ze;                        // x
        vec[n + e] = 0.0;                   // s
        z_eval[(int64_t)b * n + e] = ze;
    }
    if (tid == 0) {
        Problem p;
        problem_init(p, g_tol, maxiter);
        rec->p = p;
        for (int i = 0; i < kM; ++i) rec->rho[i] = 0.0;
    }
}

// how many problems are still active: one wavefront, a sum of fixed shape, one store to the caller's (pinned host) word
__global__ __launch_bounds__(64) void count_kernel(const char* ws, int64_t nprob, int* active_out) {
    const Record* rec = reinterpret_cast<const Record*>(ws);
    double c = 0.0;
    for (int64_t b = threadIdx.x; b < nprob; b += 64) c += rec[b].p.phase != PH_DONE ? 1.0 : 0.0;
    c = muse::wave_total<false>(c);
    if (threadIdx.x == 0) *active_out = (int)c;
}

struct InfoRecord {          // _capi.INFO_DTYPE
    int32_t iterations, f_calls, status, hist_words;
    double f_min, gnorm;
};

template <int T>
__global__ __launch_bounds__(T) void result_kernel(const char* ws, int64_t nprob, int64_t n, double* __restrict__ z_out,
                                                   InfoRecord* __restrict__ info_out) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const Record* rec = reinterpret_cast<const Record*>(ws) + b;
    const double* vec = reinterpret_cast<const double*>(ws + records_bytes(nprob)) + (int64_t)b * kVectors * n;
    for (int64_t e = tid; e < n; e += T) z_out[(int64_t)b * n + e] = vec[e];
    if (tid == 0) info_out[b] = InfoRecord{rec->p.iterations, rec->p.f_calls, rec->p.status, 0, rec->p.f, rec->p.gnorm};
}

static int check_shape(int64_t nprob, int64_t n, int m) {
    if (nprob < 1 || nprob > 0x7fffffff || n < 1 || n > (int64_t)1 << 40 || m != kM) return MUSE_LBFGS_BAD_ARGUMENT;
    return 0;
}
static int launched() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e - 100;
}

}  // namespace muse_lbfgs

using namespace muse_lbfgs;

extern "C" {

int64_t muse_lbfgs_workspace_bytes(int64_t nprob, int64_t n, int m) {
    if (check_shape(nprob, n, m)) return MUSE_LBFGS_BAD_ARGUMENT;
    return (int64_t)records_bytes(nprob) + nprob * kVectors * n * (int64_t)sizeof(double);
}

int muse_lbfgs_begin(void* ws, int64_t nprob, int64_t n, int m, const double* z0, double g_tol, int maxiter, double* z_eval, void* stream) {
    if (check_shape(nprob, n, m) || !ws || !z0 || !z_eval) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(begin_kernel<kSmallT>, dim3((unsigned)nprob), dim3(kSmallT), 0, st, (char*)ws, nprob, n, z0, g_tol, maxiter, z_eval);
    else hipLaunchKernelGGL(begin_kernel<kLargeT>, dim3((unsigned)nprob), dim3(kLargeT), 0, st, (char*)ws, nprob, n, z0, g_tol, maxiter, z_eval);
    return launched();
}

int muse_lbfgs_advance(void* ws, int64_t nprob, int64_t n, int m, const double* f, const double* g, double* z_eval, int* active_out,
                       void* stream) {
    if (check_shape(nprob, n, m) || !ws || !f || !g || !z_eval || !active_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(advance_kernel<kSmallT>, dim3((unsigned)nprob), dim3(kSmallT), 0, st, (char*)ws, nprob, n, f, g, z_eval);
    else hipLaunchKernelGGL(advance_kernel<kLargeT>, dim3((unsigned)nprob), dim3(kLargeT), 0, st, (char*)ws, nprob, n, f, g, z_eval);
    hipLaunchKernelGGL(count_kernel, dim3(1), dim3(64), 0, st, (const char*)ws, nprob, active_out);
    return launched();
}

int muse_lbfgs_result(void* ws, int64_t nprob, int64_t n, int m, double* z_out, void* info_out, void* stream) {
    if (check_shape(nprob, n, m) || !ws || !z_out || !info_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(result_kernel<kSmallT>, dim3((unsigned)nprob), dim3(kSmallT), 0, st, (const char*)ws, nprob, n, z_out, (InfoRecord*)info_out);
    else hipLaunchKernelGGL(result_kernel<kLargeT>, dim3((unsigned)nprob), dim3(kLargeT), 0, st, (const char*)ws, nprob, n, z_out, (InfoRecord*)info_out);
    return launched();
}

int muse_lbfgs_workgroup_size(int64_t n) { return n <= kSmallMaxN ? kSmallT : kLargeT; }

}  // extern "C"

// muse_lbfgs_cg_*: the lock-step conjugate gradients, kernels and entry points (the same workgroup sizes, shape limits and helpers)
#include "cg_kernels.hpp"

// muse_lbfgs_pcg_*: the same solver with a diagonal preconditioner (the record, the workspace, the count and result kernels are shared)
#include "pcg_kernels.hpp"

// muse_lbfgs_normals: the engine's normal stream for all rows of a map in one launch (the batched closure problems' draws)
#include "normals_kernels.hpp"
