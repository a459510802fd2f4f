// pcg_kernels.hpp -- the device side of muse_lbfgs_pcg_* (include/muse_lbfgs.h): the lock-step conjugate gradients of cg_kernels.hpp
// with a diagonal (Jacobi) preconditioner.  Included by lbfgs_kernels.hip after cg_kernels.hpp, whose record, workspace layout, count
// kernel and result kernel it shares: the workspace is muse_lbfgs_cg_workspace_bytes (records, y, r) and nothing more -- r / d is
// formed where it is used and never stored (pcg_advance.hpp), and the direction lives in the caller's p_eval row alone.
//
// The diagonal is the caller's device memory, [nrows / rows_per_diag][n]: row b reads diagonal row b / rows_per_diag (in get_H! the nθ
// columns of one simulation share one Hessian).  Otherwise as the plain kernels: one workgroup per row, strided passes, every reduction
// reduce.hpp's fixed-shape block_allreduce, the record through uniform / uniform_i -- a row's bits depend on its own inputs and n only.
// Whether a row's diagonal is usable is ONE workgroup-uniform value, a sum formed in begin's own pass over d: no atomics, no second
// kernel.
#pragma once
#include "pcg_advance.hpp"

namespace muse_lbfgs {

__device__ __forceinline__ void load_pcg_record(CgRecord& d, const CgRecord& s) {
    load_cg_record(d, s);
    d.rho = muse::uniform(s.rho);
}

template <int T>
struct PcgDeviceVectors {
    const int tid;
    const int64_t n;
    const double* __restrict__ b;      // begin: the right-hand side;  a round: M p
    const double* __restrict__ d;      // the row's diagonal
    double* __restrict__ p;            // the caller's evaluation row
    double *y, *r;
    double* red;
    int parity;

    __device__ __forceinline__ void start(double& rr, double& rho, double& bad) {
        double sm[3] = {0.0, 0.0, 0.0}, mx[1] = {0.0};
        for (int64_t e = tid; e < n; e += T) {
            const double be = b[e], de = d[e];
            const double ce = be / de;
            y[e] = 0.0;
            r[e] = be;
            p[e] = ce;
            sm[0] += be * be;
            sm[1] += ce * be;
            sm[2] += pcg_bad_entry(de) ? 1.0 : 0.0;
        }
        muse::block_allreduce<T, 3, 0>(sm, mx, red, parity, tid);
        rr = sm[0];
        rho = sm[1];
        bad = sm[2];
    }
    __device__ __forceinline__ void direction_is_rhs() {
        for (int64_t e = tid; e < n; e += T) p[e] = b[e];
    }
    __device__ __forceinline__ double dot_p_Mp() {
        double sm[1] = {0.0}, mx[1] = {0.0};
        for (int64_t e = tid; e < n; e += T) sm[0] += p[e] * b[e];
        muse::block_allreduce<T, 1, 0>(sm, mx, red, parity, tid);
        return sm[0];
    }
    __device__ __forceinline__ void update(double alpha, double& rr, double& rho) {
        double sm[2] = {0.0, 0.0}, mx[1] = {0.0};
        for (int64_t e = tid; e < n; e += T) {
            y[e] = y[e] + alpha * p[e];
            const double re = r[e] - alpha * b[e];
            r[e] = re;
            sm[0] += re * re;
            sm[1] += (re / d[e]) * re;
        }
        muse::block_allreduce<T, 2, 0>(sm, mx, red, parity, tid);
        rr = sm[0];
        rho = sm[1];
    }
    __device__ __forceinline__ void next_direction(double beta) {
        for (int64_t e = tid; e < n; e += T) p[e] = r[e] / d[e] + beta * p[e];
    }
};

template <int T>
__device__ __forceinline__ PcgDeviceVectors<T> pcg_vectors(char* ws, int64_t nrows, int64_t n, int b, int tid, const double* in,
                                                           const double* diag, int64_t rows_per_diag, double* p_eval, double* red) {
    double* vec = reinterpret_cast<double*>(ws + cg_records_bytes(nrows)) + (int64_t)b * 2 * n;
    return PcgDeviceVectors<T>{tid, n, in + (int64_t)b * n, diag + ((int64_t)b / rows_per_diag) * n, p_eval + (int64_t)b * n, vec, vec + n, red, 0};
}

// y = 0, r = b, p = b / d, rr, rho, the tolerance; a row that needs no iteration, or whose diagonal is not usable, is finished here
template <int T>
__global__ __launch_bounds__(T) void precond_start_kernel(char* ws, int64_t nrows, int64_t n, const double* __restrict__ rhs,
                                                          const double* __restrict__ diag, int64_t rows_per_diag, double reltol,
                                                          double abstol, int maxiter, double* __restrict__ p_eval) {
    __shared__ double red[2 * (T / 64) * 8];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    PcgDeviceVectors<T> v = pcg_vectors<T>(ws, nrows, n, b, tid, rhs, diag, rows_per_diag, p_eval, red);
    CgRecord c;
    pcg_begin_row(c, v, reltol, abstol, maxiter);
    if (tid == 0) reinterpret_cast<CgRecord*>(ws)[b] = c;
}

// one round of every active row: consumes M p, leaves the next direction in p_eval
template <int T>
__global__ __launch_bounds__(T) void precond_round_kernel(char* ws, int64_t nrows, int64_t n, const double* __restrict__ Mp,
                                                          const double* __restrict__ diag, int64_t rows_per_diag,
                                                          double* __restrict__ p_eval) {
    __shared__ double red[2 * (T / 64) * 8];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    CgRecord* rec = reinterpret_cast<CgRecord*>(ws) + b;
    if (uniform_i(rec->done)) return;   // a finished row: its record, its y and its p_eval row stay as they are
    CgRecord c;
    load_pcg_record(c, *rec);
    PcgDeviceVectors<T> v = pcg_vectors<T>(ws, nrows, n, b, tid, Mp, diag, rows_per_diag, p_eval, red);
    pcg_advance_row(c, v);
    if (tid == 0) *rec = c;
}

static int check_diag(int64_t nrows, const double* diag, int64_t rows_per_diag) {
    if (!diag || rows_per_diag < 1 || nrows % rows_per_diag != 0) return MUSE_LBFGS_BAD_ARGUMENT;
    return 0;
}

}  // namespace muse_lbfgs

extern "C" {

int muse_lbfgs_pcg_begin(void* ws, int64_t nrows, int64_t n, const double* b, const double* diag, int64_t rows_per_diag, double reltol,
                         double abstol, int maxiter, double* p_eval, int* active_out, void* stream) {
    using namespace muse_lbfgs;
    if (check_shape(nrows, n, kM) || check_diag(nrows, diag, rows_per_diag) || !ws || !b || !p_eval || !active_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(precond_start_kernel<kSmallT>, dim3((unsigned)nrows), dim3(kSmallT), 0, st, (char*)ws, nrows, n, b, diag, rows_per_diag, reltol, abstol, maxiter, p_eval);
    else hipLaunchKernelGGL(precond_start_kernel<kLargeT>, dim3((unsigned)nrows), dim3(kLargeT), 0, st, (char*)ws, nrows, n, b, diag, rows_per_diag, reltol, abstol, maxiter, p_eval);
    hipLaunchKernelGGL(cg_count_kernel, dim3(1), dim3(64), 0, st, (const char*)ws, nrows, active_out);
    return launched();
}

int muse_lbfgs_pcg_advance(void* ws, int64_t nrows, int64_t n, const double* Mp, const double* diag, int64_t rows_per_diag, double* p_eval,
                           int* active_out, void* stream) {
    using namespace muse_lbfgs;
    if (check_shape(nrows, n, kM) || check_diag(nrows, diag, rows_per_diag) || !ws || !Mp || !p_eval || !active_out) return MUSE_LBFGS_BAD_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n <= kSmallMaxN) hipLaunchKernelGGL(precond_round_kernel<kSmallT>, dim3((unsigned)nrows), dim3(kSmallT), 0, st, (char*)ws, nrows, n, Mp, diag, rows_per_diag, p_eval);
    else hipLaunchKernelGGL(precond_round_kernel<kLargeT>, dim3((unsigned)nrows), dim3(kLargeT), 0, st, (char*)ws, nrows, n, Mp, diag, rows_per_diag, p_eval);
    hipLaunchKernelGGL(cg_count_kernel, dim3(1), dim3(64), 0, st, (const char*)ws, nrows, active_out);
    return launched();
}

}  // extern "C"
