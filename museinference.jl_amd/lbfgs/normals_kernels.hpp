// normals_kernels.hpp -- the device side of muse_lbfgs_normals (include/muse_lbfgs.h): the engine's normal stream (csrc/rng.hpp:
// Philox4x32-10 keyed by the seed, counter (element, sim), fixed-sequence Box-Muller) evaluated for all rows of a map in ONE launch.
// Included by lbfgs_kernels.hip, after its helpers (launched).  rng.hpp is included as it is: the stream's bits are its, and this
// translation unit is compiled with -ffp-contract=off like the engine's.
//
// The stream of (seed, sim) as a sequence: e_{2i} = n1(i), e_{2i+1} = n2(i), (n1, n2) = normal_pair(seed, sim, i).  Row r of `out`
// holds e_{2 pair_offset} .. e_{2 pair_offset + count - 1} of stream (seed, sims[r]): ceil(count / 2) pairs, the last n2 of an odd
// count not stored.  The stream is a pure function of (seed, sim, i): nothing is advanced, a row's bits do not depend on the batch.
//
// Work split: a workgroup of T lanes takes one chunk of T K consecutive pairs of one row; lane t takes pairs t + j T (j < K), NOT K
// consecutive ones, so that the lanes of a wavefront store neighbouring pairs: 16 bytes per lane, 1 KiB per wave instruction.  The K
// pairs of a lane are K independent chains through the generator (rng.hpp: why they must be interleaved).  A row's base is
// out + r count: with an odd count, or an `out` that is only 8-byte aligned, its pairs are 8-byte aligned only -- such a row (the
// test is uniform over the workgroup) stores n1 and n2 as two doubles; an aligned row stores them as one 16-byte word.  (hipcc merges
// the two doubles into one 16-byte store as well: gfx950's global stores ask for the element's alignment only.)
// The grid is flat and one-dimensional over (row, chunk): nrows alone can exceed the 65 535 of the other dimensions.
#pragma once
#include "../csrc/rng.hpp"

namespace muse_lbfgs {

constexpr int kNormalsT = 256, kNormalsK = 4;
constexpr int64_t kNormalsChunk = (int64_t)kNormalsT * kNormalsK;       // pairs per workgroup

template <int T, int K>
__global__ __launch_bounds__(T) void normals_kernel(double* __restrict__ out, int64_t count, uint64_t seed, const int64_t* __restrict__ sims,
                                                    uint64_t pair_offset, uint32_t chunks) {
    const uint32_t row = blockIdx.x / chunks;
    const uint32_t chunk = blockIdx.x - row * chunks;
    const int64_t npairs = (count + 1) >> 1;
    const int64_t p0 = (int64_t)chunk * (T * K) + threadIdx.x;          // this lane's first pair of the row; the others: p0 + j T
    if (p0 >= npairs) return;                                           // (past the row's end, and so is every later pair of the lane)
    const uint64_t sim = (uint64_t)sims[row];
    uint64_t i[K];
#pragma unroll
    for (int j = 0; j < K; ++j) i[j] = pair_offset + (uint64_t)(p0 + (int64_t)j * T);      // 64-bit: the carry reaches the counter's high word
    muse::NormalPair np[K];
    muse::normal_pairs<K>(seed, sim, i, np);
    double* rowp = out + (int64_t)row * count;
    const bool wide = (reinterpret_cast<uintptr_t>(rowp) & 15) == 0;   // uniform over the workgroup
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int64_t p = p0 + (int64_t)j * T;
        if (p >= npairs) continue;
        double* dst = rowp + 2 * p;
        if (2 * p + 1 >= count) {
            dst[0] = np[j].n1;                                          // the last pair of an odd row: n2 is discarded
        } else if (wide) {
            *reinterpret_cast<double2*>(dst) = make_double2(np[j].n1, np[j].n2);
        } else {
            dst[0] = np[j].n1;
            dst[1] = np[j].n2;
        }
    }
}

}  // namespace muse_lbfgs

extern "C" {

int muse_lbfgs_normals(double* out, int64_t nrows, int64_t count, uint64_t seed, const int64_t* sims, int64_t pair_offset, void* stream) {
    using namespace muse_lbfgs;
    if (!out || !sims || nrows < 1 || count < 1 || pair_offset < 0) return MUSE_LBFGS_BAD_ARGUMENT;
    const int64_t npairs = (count >> 1) + (count & 1);
    const int64_t chunks = (npairs + kNormalsChunk - 1) / kNormalsChunk;
    // one workgroup per (row, chunk) in a flat grid; the counter pair_offset + i stays below 2^63
    if (nrows > 0x7fffffff / chunks || pair_offset > INT64_MAX - npairs) return MUSE_LBFGS_BAD_ARGUMENT;
    hipLaunchKernelGGL((normals_kernel<kNormalsT, kNormalsK>), dim3((unsigned)(nrows * chunks)), dim3(kNormalsT), 0, static_cast<hipStream_t>(stream),
                       out, count, seed, sims, (uint64_t)pair_offset, (uint32_t)chunks);
    return launched();
}

}  // extern "C"
