// What probe.hip, gmm.hip and pca.hip share: the shapes of their float32-MFMA tiles (v_mfma_f32_32x32x2_f32) and the accumulator's row
// map, the k-octet packing of an operand, the float64 sums over row ranges (column sums, row-scalar sums, the ascending sum of the
// ranges' partials) and the host's side (padding, shape checks, the range plans, the dispatch of the forward kernel by tiles per wave).
// docs/design/probe.md, docs/design/gmm.md and docs/design/pca.md have the semantics and the error models.
//
// The forward kernels (32 rows against all packed rows, the row softmax in registers) and the chained A^T B kernels stay written out
// in each unit, on these constants: as inline templates they compiled to other schedules and register allocations, bit-equal but up
// to a tenth slower on an MI355X (the last section of profiles/f32mm_isa.md), and a shared form is kept only where it costs nothing.
//
// The contract every client's error model and tests rest on, here and in the units' kernels:
//   - the order of k.  A forward kernel sums over k ascending from a zero accumulator, the MFMA being a k-ordered fmaf chain: octets of
//     k ascend, and inside an octet stream 0's eight products come first (k ascending), then stream 1's eight (k ascending; gmm's x^2
//     against C).  f32mm_pack lays the operand out for that order.  A bias is added after the last product.
//   - the chain rule.  An A^T B kernel sums rows ascending from a zero float32 accumulator over chains of at most F32MM_CHAIN rows,
//     counted from the range's first row; each chain's tile is added into float64 registers.  Ranges are whole numbers of chains
//     (f32mm_ranges) and are added in ascending order (f32mm_range_sum).  Column sums and row-scalar sums are float64 throughout.
//   - determinism.  Every tile, range and order depends on the shape (n, d, c) alone, and nothing here uses a floating-point atomic:
//     two calls return the same bits on any device.
//   - include only from units built with the plain flags (scd_amd/build.py): the error models charge the library forms of expf, logf,
//     sqrtf and the division, and contraction must stay at the compiler's default.
//
// tests/f32mm_plan.py restates the host side below in plain Python: f32mm_ranges, f32mm_colsum_ranges, f32mm_fwd_dispatch, each unit's
// tile count and its workspace layout.  tests/test_f32mm_plan_host.py holds the four scd_*_ws_bytes to it (they depend on R and RB, so
// they pin the plans the kernels are launched with) and names the regime of every device case: the cap of 32 ranges, a last range of
// one row, the column sums' cap of 64 ranges, NT = 2 and NT = 8 with phantom tiles.  A change to a plan here is a change there.
#pragma once
#include <type_traits>

#include "common.h"

#define F32MM_RT 32                             // rows of a forward block
#define F32MM_BK 64                             // k of an X chunk in LDS
#define F32MM_XLD 65                            // its row stride in floats
#define F32MM_THREADS 256
#define F32MM_DMAX 1024                         // the largest d, and the largest width (classes, components, columns) of an operand
#define F32MM_WMAX 1024
#define F32MM_CHAIN 256                         // rows of a float32 accumulation chain of A^T B
#define F32MM_GT 128                            // tile of A^T B: columns of A and columns of B
#define F32MM_GK 32                             // rows of A and B per LDS stage
#define F32MM_GLD 160                           // LDS row stride in floats: the two lane halves (rows k, k + 1) read distinct banks
#define F32MM_CS_ROWS 2048                      // rows per range of the column sums, at most F32MM_CS_RANGES ranges
#define F32MM_CS_RANGES 64

// row of the 32 x 32 MFMA result a lane holds in accumulator register reg (lane half h); its column is lane & 31
__device__ __forceinline__ int f32mm_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// rows [lo, hi) of range blockIdx.y
__device__ __forceinline__ void f32mm_range(long long rows_per_range, long long n, long long& lo, long long& hi) {
    lo = (long long)blockIdx.y * rows_per_range;
    hi = lo + rows_per_range < n ? lo + rows_per_range : n;
}

__host__ __device__ constexpr int f32mm_log2(int v) { return v <= 1 ? 0 : 1 + f32mm_log2(v >> 1); }

// ------------------------------------------------------------------------------------------------ packing
// S operands [rows, d] -> out [rp, S dp] (rp = rows up to 32, dp = d up to 8, zero filled), interleaved by k-octet: 8 S floats per
// octet, stream after stream, the 8 values of a stream stored as k+0, k+2, k+4, k+6, k+1, k+3, k+5, k+7.  Lane half h of the MFMA
// reads its four k values (k + 2 j + h) of a stream with one 16-byte load, and the streams of an octet share one segment.  One thread
// per element of out, 256 a block.
template <int S>
__device__ __forceinline__ void f32mm_pack(const float* const (&src)[S], int rows, int d, int rp, int dp, float* __restrict__ out) {
    static_assert((S & (S - 1)) == 0, "the streams of an octet are told apart by bits");
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= rp * S * dp) return;
    const int row = e / (S * dp), q = e % (S * dp);
    const int w = q & (8 * S - 1), pos = w & 7;
    const int k = (q >> (3 + f32mm_log2(S))) * 8 + 2 * (pos & 3) + (pos >> 2);
    const float* s = src[0];
#pragma unroll
    for (int i = 1; i < S; ++i)
        if ((w >> 3) == i) s = src[i];
    out[e] = (row < rows && k < d) ? s[(size_t)row * d + k] : 0.f;
}

// ------------------------------------------------------------------------------------------------ float64 sums over a row range
// column tid & 31 of 32 columns: val(g) over rows [lo, hi), eight row groups, then the groups in ascending order.  Threads 0 ... 31
// return their column's sum.  sh: F32MM_THREADS doubles.
template <class Val>
__device__ __forceinline__ double f32mm_colsum(long long lo, long long hi, const Val& val, double* sh) {
    const int tid = threadIdx.x, rsub = tid >> 5;
    double a = 0.0;
    for (long long g = lo + rsub; g < hi; g += 8) a += (double)val(g);
    sh[tid] = a;
    __syncthreads();
    double t = 0.0;
    if (tid < 32) {
        t = sh[tid];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += sh[tid + 32 * q];
    }
    return t;
}

// the sum of v[lo ... hi) by the whole block, a tree over the threads' strided sums; thread 0 returns it.  sh may be in use on entry.
template <class T>
__device__ __forceinline__ double f32mm_rowsum(const T* __restrict__ v, long long lo, long long hi, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    double a = 0.0;
    for (long long g = lo + tid; g < hi; g += F32MM_THREADS) a += (double)v[g];
    sh[tid] = a;
    __syncthreads();
    for (int o = F32MM_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}

// element e of R range partials `stride` apart, added in ascending order
__device__ __forceinline__ double f32mm_range_sum(const double* __restrict__ part, size_t stride, size_t e, int R) {
    double a = 0.0;
    for (int q = 0; q < R; ++q) a += part[q * stride + e];
    return a;
}

// ------------------------------------------------------------------------------------------------ host
static inline int f32mm_pad(int v, int to) { return (int)scd_cdiv(v, to) * to; }

static inline bool f32mm_shape_ok(int64_t n, int d, int w, int wmin) {
    return n >= 1 && n < (1ll << 31) && d >= 1 && d <= F32MM_DMAX && w >= wmin && w <= F32MM_WMAX;
}

// the checks of an entry point's n and d, of a width w (classes, components, columns) and of its workspace ws
#define F32MM_ND_REQUIRE(who, n, d)                                                                             \
    SCD_REQUIRE((n) >= 1 && (n) < (1ll << 31), who ": n = %lld outside [1, 2^31)", (long long)(n));             \
    SCD_REQUIRE((d) >= 1 && (d) <= F32MM_DMAX, who ": d = %d outside [1, %d]", (d), F32MM_DMAX)
#define F32MM_WIDTH_REQUIRE(who, name, w, wmin) \
    SCD_REQUIRE(w >= wmin && w <= F32MM_WMAX, who ": " name " = %d outside [%d, %d]", w, wmin, F32MM_WMAX)
#define F32MM_WS_REQUIRE(who, ws) SCD_REQUIRE((uintptr_t)(ws) % 16 == 0, who ": workspace not 16-byte aligned")

// row ranges of A^T B over `tiles` tiles: at least four chains each, at most 32, about target_blocks blocks; a whole number of chains
// per range
static inline void f32mm_ranges(int64_t n, long long tiles, long long target_blocks, int& R, long long& rows_per_range) {
    const long long chains = scd_cdiv(n, F32MM_CHAIN);
    long long r = chains / 4, cap = scd_cdiv(target_blocks, tiles);
    if (cap > 32) cap = 32;
    if (r > cap) r = cap;
    if (r < 1) r = 1;
    rows_per_range = scd_cdiv(chains, r) * F32MM_CHAIN;
    R = (int)scd_cdiv(n, rows_per_range);
}

// row ranges of the column sums: F32MM_CS_ROWS rows each, at most F32MM_CS_RANGES ranges
static inline void f32mm_colsum_ranges(int64_t n, int& RB, long long& rows_per_range) {
    long long r = scd_cdiv(n, F32MM_CS_ROWS);
    if (r > F32MM_CS_RANGES) r = F32MM_CS_RANGES;
    rows_per_range = scd_cdiv(n, r);
    RB = (int)scd_cdiv(n, rows_per_range);
}

// launch(grid, NT) for the forward kernel of n rows against rp packed rows: NT (a std::integral_constant) = the 32-row tiles of a
// wave, rp / 32 tiles over four waves, rounded up to 1, 2, 4 or 8
template <class Launch>
static inline void f32mm_fwd_dispatch(int64_t n, int rp, const Launch& launch) {
    const int per = (int)scd_cdiv(rp / 32, 4);
    const unsigned grid = (unsigned)scd_cdiv(n, F32MM_RT);
    if (per <= 1) launch(grid, std::integral_constant<int, 1>());
    else if (per <= 2) launch(grid, std::integral_constant<int, 2>());
    else if (per <= 4) launch(grid, std::integral_constant<int, 4>());
    else launch(grid, std::integral_constant<int, 8>());
}
