// cg_kernels.hpp -- the device side of muse_lbfgs_cg_* (include/muse_lbfgs.h): lock-step conjugate gradients for a batch of rows whose
// operator is the caller's.  Included by lbfgs_kernels.hip, after its helpers (records' alignment, uniform_i, check_shape, launched).
//
// Workspace:  records [nrows] (CgRecord, cg_control.hpp)
//             vectors [nrows][2][n] doubles: y, r.   The direction p lives in the caller's p_eval row and nowhere else.
// As the L-BFGS kernels: rows have stride n (one double per access), lane l of a pass touches element l + k T of every vector, the
// threads of a workgroup meet only in the reductions, the workgroup size is a function of n alone and every reduction is reduce.hpp's
// fixed-shape block_allreduce -- a row's bits depend on its own inputs and n, not on the batch or its place in it.  No atomics, no
// workgroup waits for another, no spin.
#pragma once
#include "cg_advance.hpp"

namespace muse_lbfgs {

__host__ __device__ inline size_t cg_records_bytes(int64_t nrows) { return ((size_t)nrows * sizeof(CgRecord) + 255) / 256 * 256; }

// the record, field by field through v_readfirstlane: the round's branches compile scalar
__device__ __forceinline__ void load_cg_record(CgRecord& d, const CgRecord& s) {
    d.rr = muse::uniform(s.rr);
    d.tol = muse::uniform(s.tol);
    d.count = uniform_i(s.count);
    d.maxiter = uniform_i(s.maxiter);
    d.done = uniform_i(s.done);
    d.pad_ = 0;
    d.rho = 0.0;
}

template <int T>
struct CgDeviceVectors {
    const int tid;
    const int64_t n;
    const double* __restrict__ b;      // begin: the right-hand side;  a round: M p
    double* __restrict__ p;            // the caller's evaluation row
    double *y, *r;
    double* red;
    int parity;

    __device__ __forceinline__ double sum1(double a) {
        double sm[1] = {a}, mx[1] = {0.0};
        muse::block_allreduce<T, 1, 0>(sm, mx, red, parity, tid);
        return sm[0];
    }
    __device__ __forceinline__ double start() {
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            const double be = b[e];
            y[e] = 0.0;
            r[e] = be;
            p[e] = be;
            acc += be * be;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ double dot_p_Mp() {
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) acc += p[e] * b[e];
        return sum1(acc);
    }
    __device__ __forceinline__ double update(double alpha) {
        double acc = 0.0;
        for (int64_t e = tid; e < n; e += T) {
            y[e] = y[e] + alpha * p[e];
            const double re = r[e] - alpha * b[e];
            r[e] = re;
            acc += re * re;
        }
        return sum1(acc);
    }
    __device__ __forceinline__ void next_direction(double beta) {
        for (int64_t e = tid; e < n; e += T) p[e] = r[e] + beta * p[e];
    }
};

template <int T>
__device__ __forceinline__ CgDeviceVectors<T> cg_vectors(char* ws, int64_t nrows, int64_t n, int b, int tid, const double* in, double* p_eval,
                                                         double* red) {
    double* vec = reinterpret_cast<double*>(ws + cg_records_bytes(nrows)) + (int64_t)b * 2 * n;
    return CgDeviceVectors<T>{tid, n, in + (int64_t)b * n, p_eval + (int64_t)b * n, vec, vec + n, red, 0};
}

// y = 0, r = p = b, rr = b . b, the tolerance; a row that needs no iteration is finished here
template <int T>
__global__ __launch_bounds__(T) void cg_begin_kernel(char* ws, int64_t nrows, int64_t n, const double* __restrict__ rhs, double reltol,
                                                     double abstol, int maxiter, double* __restrict__ p_eval) {
    __shared__ double red[2 * (T / 64) * 8];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    CgDeviceVectors<T> v = cg_vectors<T>(ws, nrows, n, b, tid, rhs, p_eval, red);
    CgRecord c;
    cg_begin_row(c, v, reltol, abstol, maxiter);
    if (tid == 0) reinterpret_cast<CgRecord*>(ws)[b] = c;
}

// one round of every active row: consumes M p, leaves the next direction in p_eval
template <int T>
__global__ __launch_bounds__(T) void cg_step_kernel(char* ws, int64_t nrows, int64_t n, const double* __restrict__ Mp,
                                                    double* __restrict__ p_eval) {
    __shared__ double red[2 * (T / 64) * 8];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    CgRecord* rec = reinterpret_cast<CgRecord*>(ws) + b;
    if (uniform_i(rec->done)) return;   // a finished row: its record, its y and its p_eval row stay as they are
    CgRecord c;
    load_cg_record(c, *rec);
    CgDeviceVectors<T> v = cg_vectors<T>(ws, nrows, n, b, tid, Mp, p_eval, red);
    cg_advance_row(c, v);
    if (tid == 0) *rec = c;
}

// how many rows are still active: one wavefront, a sum of fixed shape, one store to the caller's (pinned host) word
__global__ __launch_bounds__(64) void cg_count_kernel(const char* ws, int64_t nrows, int* active_out) {
    const CgRecord* rec = reinterpret_cast<const CgRecord*>(ws);
    double c = 0.0;
    for (int64_t b = threadIdx.x; b < nrows; b += 64) c += rec[b].done ? 0.0 : 1.0;
    c = muse::wave_total<false>(c);
    if (threadIdx.x == 0) *active_out = (int)c;
}

template <int T>
__global__ __launch_bounds__(T) void cg_result_kernel(const char* ws, int64_t nrows, int64_t n, double* __restrict__ y_out,
                                                      int32_t* __restrict__ iterations_out, double* __restrict__ resnorm_out) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const CgRecord* rec = reinterpret_cast<const CgRecord*>(ws) + b;
    const double* y = reinterpret_cast<const double*>(ws + cg_records_bytes(nrows)) + (int64_t)b * 2 * n;
    for (int64_t e = tid; e < n; e += T) y_out[(int64_t)b * n + e] = y[e];
    if (tid == 0) {
        iterations_out[b] = rec->count;
        resnorm_out[b] = __builtin_sqrt(rec->rr);
    }
}

}  // namespace muse_lbfgs

extern "C" {

int64_t muse_lbfgs_cg_workspace_bytes(int64_t nrows, int64_t n) {
    using namespace muse_lbfgs;
    if (check_shape(nrows, n, kM)) return MUSE_LBFGS_BAD_ARGUMENT;
    return (int64_t)cg_records_bytes(nrows) + nrows * 2 * n * (int64_t)sizeof(double);
}

int muse_lbfgs_cg_begin(void* ws, int64_t nrows, int64_t n, const double* b, double reltol, double abstol, int maxiter, double* p_eval,
                        int* active_out, void* stream) {
    using namespace muse_lbfgs;
    if (check_shape(nrows, n, kM) || !ws || !b || !p_eval || !active_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(cg_begin_kernel<kSmallT>, dim3((unsigned)nrows), dim3(kSmallT), 0, st, (char*)ws, nrows, n, b, reltol, abstol, maxiter, p_eval);
    else hipLaunchKernelGGL(cg_begin_kernel<kLargeT>, dim3((unsigned)nrows), dim3(kLargeT), 0, st, (char*)ws, nrows, n, b, reltol, abstol, maxiter, p_eval);
    hipLaunchKernelGGL(cg_count_kernel, dim3(1), dim3(64), 0, st, (const char*)ws, nrows, active_out);
    return launched();
}

int muse_lbfgs_cg_advance(void* ws, int64_t nrows, int64_t n, const double* Mp, double* p_eval, int* active_out, void* stream) {
    using namespace muse_lbfgs;
    if (check_shape(nrows, n, kM) || !ws || !Mp || !p_eval || !active_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(cg_step_kernel<kSmallT>, dim3((unsigned)nrows), dim3(kSmallT), 0, st, (char*)ws, nrows, n, Mp, p_eval);
    else hipLaunchKernelGGL(cg_step_kernel<kLargeT>, dim3((unsigned)nrows), dim3(kLargeT), 0, st, (char*)ws, nrows, n, Mp, p_eval);
    hipLaunchKernelGGL(cg_count_kernel, dim3(1), dim3(64), 0, st, (const char*)ws, nrows, active_out);
    return launched();
}

int muse_lbfgs_cg_result(void* ws, int64_t nrows, int64_t n, double* y_out, int32_t* iterations_out, double* resnorm_out, void* stream) {
    using namespace muse_lbfgs;
    if (check_shape(nrows, n, kM) || !ws || !y_out || !iterations_out || !resnorm_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(cg_result_kernel<kSmallT>, dim3((unsigned)nrows), dim3(kSmallT), 0, st, (const char*)ws, nrows, n, y_out, iterations_out, resnorm_out);
    else hipLaunchKernelGGL(cg_result_kernel<kLargeT>, dim3((unsigned)nrows), dim3(kLargeT), 0, st, (const char*)ws, nrows, n, y_out, iterations_out, resnorm_out);
    return launched();
}

}  // extern "C"
