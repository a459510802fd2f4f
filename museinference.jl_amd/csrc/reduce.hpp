// reduce.hpp -- workgroup-uniform scalars and the fixed-shape workgroup all-reduce (see muse_kernels.hip).
#pragma once
#include "args.hpp"

namespace muse {

// Maxima are taken with v_max_f64 (one instruction; a NaN operand is DROPPED), on |values| that start from 0.
// NaN propagation -- Julia's maximum(abs, g) is NaN if any element is -- comes from the sums reduced in the same
// pass: a NaN element makes the pass's objective / directional-derivative sum NaN, and the caller then replaces
// the maximum by NaN (nan_if).  (The explicit compare/select form cost 6 instructions per element and per
// reduction step.)
__device__ __forceinline__ double absmax(double a, double b) { return __builtin_fmax(a, __builtin_fabs(b)); }
__device__ __forceinline__ double nan_if(bool c, double v) { return c ? __builtin_nan("") : v; }

// Tell the compiler a value is workgroup-uniform (it is: every lane holds the same bits).  Control
// flow that depends on it then compiles to scalar branches and its live state to SGPRs.
__device__ __forceinline__ double uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- fixed-shape all-reduce over the workgroup: KS sums and KM NaN-dropping maxima ---------------
// Within a wave: four DPP exchange steps (xor 1, xor 2, half-row mirror, row mirror -- full-rate VALU
// moves, no LDS crossbar) leave each 16-lane row's total in all of its lanes; the four row totals r0..r3 are
// combined as (r0 + r1) + (r2 + r3) by two more DPP steps towards the wave's LAST lane (row_bcast:15 into
// rows 1 and 3, row_bcast:31 into rows 2 and 3), whose register then holds the wave total.
// Across waves: lane 63 of each wave stores its total to LDS, ONE barrier, then lane l of every wave
// reads wave (l mod NW)'s total and a DPP butterfly over NW lanes + v_readfirstlane leaves the
// workgroup total in SGPRs of every wave.  The tree is the same for every thread, launch and GPU.
//
// ORDER OF EMISSION.  Each value has a butterfly and a tree of its own, and one value's reduction is ONE chain of
// dependent instructions (~11 cycles each for a wave; both waves of a SIMD are in the same reduction, so neither
// hides the other's).  The K = KS + KM values of a reduction are therefore written SIDE BY SIDE, as rng.hpp writes
// its MUSE_K chains: an array of K and one source statement per step -- exchange step 1 of all K values, then
// step 2 of all, ... -- so that K independent instructions stand next to each other.  Per value the operations,
// their operands and their order are those of a single value's chain: nothing is packed or transposed.
template <int CTRL, int ROWS = 0xf, bool BOUND = true>
__device__ __forceinline__ double dpp_move(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), CTRL, ROWS, 0xf, BOUND);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, ROWS, 0xf, BOUND);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
__device__ __forceinline__ double read_lane(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
constexpr int kDppXor1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror: lane i <-> 7-i within 8
constexpr int kDppMirror = 0x140;      // row_mirror:      lane i <-> 15-i within 16
constexpr int kDppRowBcast15 = 0x142;  // row_bcast:15:    lane 15 of a row -> every lane of the next row
constexpr int kDppRowBcast31 = 0x143;  // row_bcast:31:    lane 31 -> every lane of rows 2 and 3

// The maximum of a reduction step: the bare instruction.  __builtin_fmax on a bit pattern that came through a DPP move or
// a v_readlane is preceded by a canonicalising v_max_f64 x, x, x (the compiler cannot know that the pattern is no
// signalling NaN); the operands here are results of arithmetic and fabs, never signalling.  Not volatile: the scheduler
// places it like any other VALU instruction (and the hazard recogniser still sees the register it writes: a DPP move
// that reads it right away gets its two wait states).
__device__ __forceinline__ double max_bare(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (row totals read into SGPRs: a gfx9 VOP3 reads ONE scalar operand; the other goes through a vector register, as for the sums)
__device__ __forceinline__ double max_bare_sv(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "s"(a), "v"(b));
    return r;
}
// One exchange step of K values (the first KS are sums, the others maxima): all the moves, then all the combinations.
template <int KS, int CTRL, int K>
__device__ __forceinline__ void dpp_step(double (&v)[K]) {
    double t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = dpp_move<CTRL>(v[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = k < KS ? v[k] + t[k] : max_bare(v[k], t[k]);
}
// The same with an exchange that only the rows of the mask ROWS receive; what arrives is the LEFT operand (the lower rows' total).
template <int KS, int CTRL, int ROWS, int K>
__device__ __forceinline__ void dpp_step_up(double (&v)[K]) {
    double t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = dpp_move<CTRL, ROWS, false>(v[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = k < KS ? t[k] + v[k] : max_bare(t[k], v[k]);
}
// The wave totals of K values, (r0 + r1) + (r2 + r3) over the four rows' totals, left in lane kTotalLane<ROW_BCAST>.
// ROW_BCAST (the default): the row totals stay in vector registers -- row_bcast:15 leaves r0 + r1 in row 1 and r2 + r3 in
// row 3, row_bcast:31 adds lane 31's r0 + r1 to rows 2 and 3: six full-rate instructions per value, and lane 63 stores its
// own register (the other lanes hold partial results nobody reads).  Without it, the form this code had before: eight
// v_readlane per value into SGPRs, the combination on scalar operands (with the moves the one-scalar-operand limit
// forces) -- every lane then holds the total.  An entry point that the vector form costs registers keeps this one
// (solver.hpp, row_broadcast()).
template <bool ROW_BCAST>
constexpr int kTotalLane = ROW_BCAST ? 63 : 0;
template <int KS, bool ROW_BCAST, int K>
__device__ __forceinline__ void wave_totals(double (&v)[K]) {
    dpp_step<KS, kDppXor1>(v);
    dpp_step<KS, kDppXor2>(v);
    dpp_step<KS, kDppHalfMirror>(v);
    dpp_step<KS, kDppMirror>(v);
    if constexpr (ROW_BCAST) {
        dpp_step_up<KS, kDppRowBcast15, 0xa>(v);
        dpp_step_up<KS, kDppRowBcast31, 0xc>(v);
    } else {
        double r0[K], r1[K], r2[K], r3[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            r0[k] = read_lane(v[k], 0);
            r1[k] = read_lane(v[k], 16);
            r2[k] = read_lane(v[k], 32);
            r3[k] = read_lane(v[k], 48);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            r0[k] = k < KS ? r0[k] + r1[k] : max_bare_sv(r0[k], r1[k]);
            r2[k] = k < KS ? r2[k] + r3[k] : max_bare_sv(r2[k], r3[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = k < KS ? r0[k] + r2[k] : max_bare(r0[k], r2[k]);
    }
}
// The butterfly over the first NW (<= 16) lanes of a row, K values side by side.
template <int KS, int NW, int K>
__device__ __forceinline__ void lanes_totals(double (&v)[K]) {
    if constexpr (NW >= 2) dpp_step<KS, kDppXor1>(v);
    if constexpr (NW >= 4) dpp_step<KS, kDppXor2>(v);
    if constexpr (NW >= 8) dpp_step<KS, kDppHalfMirror>(v);
    if constexpr (NW >= 16) dpp_step<KS, kDppMirror>(v);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = uniform(v[k]);
}
// One value alone (the per-wave statistics of kernels.hpp and step.hpp): the same tree, the total as a scalar.
template <bool IS_MAX>
__device__ __forceinline__ double wave_total(double v) {
    double a[1] = {v};
    wave_totals<IS_MAX ? 0 : 1, true>(a);
    return read_lane(a[0], kTotalLane<true>);
}

// RAW: the barrier alone (s_waitcnt lgkmcnt(0) + s_barrier) instead of __syncthreads(), whose fence also drains the
// vector-memory counter -- every store of the pass (the MAP going out in a solve's last pass: 80 KB per workgroup) and
// every LDS-DMA prefetch in flight would have to complete before the reduction could (measured at configs[1]: 48.9 -> 36.6 us
// per 512-sim step).  For code whose threads only ever meet through LDS and re-read from memory only what they stored
// themselves (the elementwise models); the stencil model's passes read what other threads stored.
template <bool RAW>
__device__ __forceinline__ void wg_barrier() {
    if constexpr (RAW) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
}
template <int T, int KS, int KM, bool RAW = false, bool ROW_BCAST = true>
__device__ __forceinline__ void block_allreduce(double (&s)[KS > 0 ? KS : 1], double (&m)[KM > 0 ? KM : 1],
                                                double* red, int& parity, int tid) {
    constexpr int NW = T / 64, K = KS + KM;
    // (laundered: otherwise the LDS addresses derived from tid are computed once per kernel, live -- and, in the
    // register-bound placements, spilled to scratch -- across the persistent loop, and every reduction waits for a
    // scratch reload before its LDS write)
    asm volatile("" : "+v"(tid));
    static_assert(NW == 1 || NW == 2 || NW == 4 || NW == 8 || NW == 16, "workgroup must be 2^k waves");
    static_assert(K >= 1 && K <= 8, "reduction scratch holds 8 values per wave");
    double v[K];   // the sums, then the maxima: the order of the LDS slots
#pragma unroll
    for (int k = 0; k < KS; ++k) v[k] = s[k];
#pragma unroll
    for (int k = 0; k < KM; ++k) v[KS + k] = m[k];
    wave_totals<KS, ROW_BCAST>(v);
    double* buf = red + parity * (NW * 8);
    const int wave = tid >> 6;
    if ((tid & 63) == kTotalLane<ROW_BCAST>) {
#pragma unroll
        for (int k = 0; k < K; ++k) buf[wave * K + k] = v[k];
    }
    __syncthreads();
    const int src = (tid & (NW - 1)) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = buf[src + k];
    lanes_totals<KS, NW>(v);
#pragma unroll
    for (int k = 0; k < KS; ++k) s[k] = v[k];
#pragma unroll
    for (int k = 0; k < KM; ++k) m[k] = v[KS + k];
    parity ^= 1;
}


}  // namespace muse
