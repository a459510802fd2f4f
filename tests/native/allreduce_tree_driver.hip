// block_allreduce (csrc/reduce.hpp) alone: one workgroup per launch that does nothing but reduce, every thread's result written out.
//   allreduce_tree_driver <in.f64> <out.f64> <nsets>
// The cases, in this order: T in {64, 128, 256, 512, 1024} x (KS, KM) in {(1,0), (0,1), (3,1), (4,2), (7,1), (8,0)}.  A case's
// input is nsets x K x T doubles (set, value, thread; the KS sums first, then the KM maxima), its output has the same shape: what
// thread t holds for value k after the reduction of set s.  The output file holds the cases twice: first with the row totals
// combined in vector registers (block_allreduce's default), then with the v_readlane form (ROW_BCAST = false).  The sets of a case
// go through ONE launch, one reduction after the other, so the parity buffer alternates as it does in the solver.
// (tests/test_gpu_allreduce_tree.py writes the input and checks the bits.)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reduce.hpp"

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            std::fprintf(stderr, "%s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);      \
            std::exit(2);                                                                            \
        }                                                                                            \
    } while (0)

template <int T, int KS, int KM, bool ROW_BCAST>
__global__ __launch_bounds__(T) void allreduce_kernel(const double* __restrict__ in, double* __restrict__ out, int nsets) {
    constexpr int K = KS + KM;
    __shared__ double red[2 * (T / 64) * 8];   // two parities x waves x 8 values
    const int tid = (int)threadIdx.x;
    int parity = 0;
    for (int set = 0; set < nsets; ++set) {
        const size_t base = (size_t)set * K * T;
        double s[KS > 0 ? KS : 1] = {0.0}, m[KM > 0 ? KM : 1] = {0.0};
        for (int k = 0; k < KS; ++k) s[k] = in[base + (size_t)k * T + tid];
        for (int k = 0; k < KM; ++k) m[k] = in[base + (size_t)(KS + k) * T + tid];
        muse::block_allreduce<T, KS, KM, false, ROW_BCAST>(s, m, red, parity, tid);
        for (int k = 0; k < KS; ++k) out[base + (size_t)k * T + tid] = s[k];
        for (int k = 0; k < KM; ++k) out[base + (size_t)(KS + k) * T + tid] = m[k];
    }
}

template <int T, int KS, int KM, bool RB>
static size_t run_case(const double* d_in, double* d_out, size_t offset, size_t total, int nsets) {
    const size_t n = (size_t)nsets * (KS + KM) * T;
    if (offset + n > total) {
        std::fprintf(stderr, "input too short for case T=%d KS=%d KM=%d\n", T, KS, KM);
        std::exit(2);
    }
    hipLaunchKernelGGL((allreduce_kernel<T, KS, KM, RB>), dim3(1), dim3(T), 0, 0, d_in + offset, d_out + offset, nsets);
    CHECK(hipGetLastError());
    return offset + n;
}

template <int T, bool RB>
static size_t run_T(const double* d_in, double* d_out, size_t offset, size_t total, int nsets) {
    offset = run_case<T, 1, 0, RB>(d_in, d_out, offset, total, nsets);
    offset = run_case<T, 0, 1, RB>(d_in, d_out, offset, total, nsets);
    offset = run_case<T, 3, 1, RB>(d_in, d_out, offset, total, nsets);
    offset = run_case<T, 4, 2, RB>(d_in, d_out, offset, total, nsets);
    offset = run_case<T, 7, 1, RB>(d_in, d_out, offset, total, nsets);
    offset = run_case<T, 8, 0, RB>(d_in, d_out, offset, total, nsets);
    return offset;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s in.f64 out.f64 nsets\n", argv[0]);
        return 2;
    }
    const int nsets = std::atoi(argv[3]);
    if (nsets < 1 || nsets > 64) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    const size_t total = (size_t)std::ftell(f) / sizeof(double);
    std::fseek(f, 0, SEEK_SET);
    std::vector<double> host(total);
    if (std::fread(host.data(), sizeof(double), total, f) != total) return 2;
    std::fclose(f);

    double *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, total * sizeof(double)));
    CHECK(hipMalloc(&d_out, 2 * total * sizeof(double)));
    CHECK(hipMemcpy(d_in, host.data(), total * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xff, 2 * total * sizeof(double)));
    size_t offset = 0;
    offset = run_T<64, true>(d_in, d_out, offset, total, nsets);
    offset = run_T<128, true>(d_in, d_out, offset, total, nsets);
    offset = run_T<256, true>(d_in, d_out, offset, total, nsets);
    offset = run_T<512, true>(d_in, d_out, offset, total, nsets);
    offset = run_T<1024, true>(d_in, d_out, offset, total, nsets);
    size_t offset2 = 0;
    offset2 = run_T<64, false>(d_in, d_out + total, offset2, total, nsets);
    offset2 = run_T<128, false>(d_in, d_out + total, offset2, total, nsets);
    offset2 = run_T<256, false>(d_in, d_out + total, offset2, total, nsets);
    offset2 = run_T<512, false>(d_in, d_out + total, offset2, total, nsets);
    offset2 = run_T<1024, false>(d_in, d_out + total, offset2, total, nsets);
    CHECK(hipDeviceSynchronize());
    if (offset != total || offset2 != total) {
        std::fprintf(stderr, "input holds %zu doubles, the cases take %zu\n", total, offset);
        return 2;
    }
    host.resize(2 * total);
    CHECK(hipMemcpy(host.data(), d_out, 2 * total * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(host.data(), sizeof(double), 2 * total, f) != 2 * total) return 2;
    std::fclose(f);
    std::printf("allreduce_tree_driver: %zu values\n", total);
    return 0;
}
