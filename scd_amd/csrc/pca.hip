// Principal component analysis on gfx950: the centred Gram matrix of a feature cache and the projection onto its components, without a
// centred or float64 copy of the rows (scikit-learn 1.7's PCA(svd_solver='covariance_eigh'); the eigensolver of the d x d matrix runs on
// the host).  docs/design/pca.md has the semantics, the error model and the resources.
//
// Every kernel sees the rows as c_ij = fl32(x_ij - shift_j): one IEEE float32 subtraction in a register, as the value is staged.
//
//   scd_pca_colsum      float64 column sums of c: pca_colsum_kernel over RB row ranges of fixed size -> colpart [RB, d];
//                       pca_colsum_finish_kernel adds the ranges in ascending order.
//   scd_pca_gram        G = c^T c in float64: pca_gram_kernel on 128 x 128 tiles of (dim, dim), upper-triangle tiles only, times R row
//                       ranges; both operands go through LDS 32 rows at a time, the float32 MFMA (v_mfma_f32_32x32x2_f32) runs over
//                       chains of at most PC_CHAIN = 256 rows, each chain's tile is added into float64 registers; a range's float64 tile
//                       -> part [R, d, d].  pca_gram_finish_kernel adds the ranges in ascending order and writes G[j][l] and G[l][j]
//                       (j <= l) from the same sum: G is bit-symmetric.
//   scd_pca_transform   y_ik = sum_j c_ij W_kj: pca_pack_kernel packs W [m, d] by k-octet (probe.hip's packing); pca_fwd_kernel: a block
//                       owns PC_RT = 32 rows and all m columns (up to 32), wave w the 32-column tiles w, w + 4, ... in up to 8 accumulator
//                       tiles; c goes through LDS in chunks of 64 j, the packed W streams from L2; the sum over j ascends from a zero
//                       accumulator.  unit: the float32 sum of squares over the real m columns (lanes by shuffles, waves through LDS in
//                       wave order), sqrtf and a division, both correctly rounded; a row of norm 0 is written as zeros.
//
// No floating-point atomics (the info counters and the row flags are integers).  R, RB and every tile depend on (n, d, m) alone: two
// calls return the same bits on any device.
#include "common.h"

#define PC_RT 32                                // rows of a projection block
#define PC_BK 64                                // j of a chunk of c in LDS
#define PC_XLD 65                               // its row stride in floats
#define PC_THREADS 256
#define PC_DMAX 1024
#define PC_MMAX 1024
#define PC_CHAIN 256                            // rows of a float32 accumulation chain in the Gram matrix
#define PC_GT 128                               // Gram tile: dims and dims
#define PC_GK 32                                // rows of c per LDS stage
#define PC_GLD 160                              // LDS row stride in floats: the two lane halves (rows k, k + 1) read distinct banks
#define PC_CS_ROWS 2048                         // rows per range of the column-sum kernel, at most PC_CS_RANGES ranges
#define PC_CS_RANGES 64

// row of the 32 x 32 MFMA result a lane holds in accumulator register reg (lane half h); its column is lane & 31
__device__ __forceinline__ int pc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------------------ column sums
// grid (d up to 32 / 32, RB): float64 column sums of c over a row range -> colpart [RB, dp32]
__global__ void __launch_bounds__(PC_THREADS) pca_colsum_kernel(const float* __restrict__ X, const float* __restrict__ shift, long long n, int d,
                                                                int dp32, long long rows_per_range, double* __restrict__ colpart) {
    __shared__ double sh[PC_THREADS];
    const long long lo = (long long)blockIdx.y * rows_per_range;
    const long long hi = lo + rows_per_range < n ? lo + rows_per_range : n;
    const int tid = threadIdx.x, cl = tid & 31, rsub = tid >> 5;
    const int col = blockIdx.x * 32 + cl, cc = col < d ? col : d - 1;
    const float sv = shift[cc];
    double a = 0.0;
    for (long long g = lo + rsub; g < hi; g += 8) a += (double)(X[(size_t)g * d + cc] - sv);
    sh[tid] = a;
    __syncthreads();
    if (tid < 32) {
        double t = sh[tid];
#pragma unroll
        for (int q = 1; q < 8; ++q) t += sh[tid + 32 * q];
        colpart[(size_t)blockIdx.y * dp32 + col] = t;
    }
}

__global__ void __launch_bounds__(256) pca_colsum_finish_kernel(const double* __restrict__ colpart, int d, int dp32, int RB,
                                                                double* __restrict__ csum) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    double a = 0.0;
    for (int q = 0; q < RB; ++q) a += colpart[(size_t)q * dp32 + col];
    csum[col] = a;
}

// ------------------------------------------------------------------------------------------------ Gram partials
// grid (upper-triangle tiles, R).  Tile t is (ti, tj) with ti <= tj: rows ti * 128 ... of G against columns tj * 128 ...; part [R, d, d]
// float64, of which the tile's elements alone are written.  flags int [n]: a row that holds a non-finite c is counted once in info[0]
// (the diagonal tiles see every column exactly once).
__global__ void __launch_bounds__(PC_THREADS) pca_gram_kernel(const float* __restrict__ X, const float* __restrict__ shift, long long n, int d,
                                                              int dtiles, long long rows_per_range, double* __restrict__ part,
                                                              int* __restrict__ flags, int* __restrict__ info) {
    __shared__ float as[PC_GK * PC_GLD];
    __shared__ float bs[PC_GK * PC_GLD];
    // the tile of this block: row ti of the triangle holds dtiles - ti tiles
    int ti = 0, rem = blockIdx.x;
    while (rem >= dtiles - ti) {
        rem -= dtiles - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int a0 = ti * PC_GT, b0 = tj * PC_GT;
    const bool diag = ti == tj;
    const long long lo = (long long)blockIdx.y * rows_per_range;
    const long long hi = lo + rows_per_range < n ? lo + rows_per_range : n;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    bool on[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) on[i][j] = a0 + wm * 64 + i * 32 < d && b0 + wn * 64 + j * 32 < d;

    f32x16 acc[2][2];
    double acc64[2][2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                acc[i][j][q] = 0.f;
                acc64[i][j][q] = 0.0;
            }

    // a thread stages one column of each operand (col = tid & 127), rows 2 i + (tid >> 7): its two shifts are loaded once
    const int col = tid & 127, rsub = tid >> 7;
    const bool ina = a0 + col < d, inb = b0 + col < d;
    const int ca = ina ? a0 + col : d - 1, cb = inb ? b0 + col : d - 1;
    const float sa = shift[ca], sb = shift[cb];

    // no branch around a load: the next 32 rows are in registers while the MFMAs run (addresses clamped, values masked)
    float ar[PC_GK * PC_GT / PC_THREADS], br[PC_GK * PC_GT / PC_THREADS];
    auto load_rows = [&](long long base) {
#pragma unroll
        for (int i = 0; i < PC_GK * PC_GT / PC_THREADS; ++i) {
            const long long gr = base + 2 * i + rsub;
            const long long g = gr < hi ? gr : hi - 1;
            ar[i] = X[(size_t)g * d + ca];
            br[i] = X[(size_t)g * d + cb];
        }
    };
    load_rows(lo);
    for (long long base = lo; base < hi; base += PC_GK) {
        __syncthreads();
        int bad = 0;
#pragma unroll
        for (int i = 0; i < PC_GK * PC_GT / PC_THREADS; ++i) {
            const int row = 2 * i + rsub;
            const bool in = base + row < hi;
            const float cva = ar[i] - sa, cvb = br[i] - sb;
            as[row * PC_GLD + col] = (in && ina) ? cva : 0.f;
            bs[row * PC_GLD + col] = (in && inb) ? cvb : 0.f;
            if (in && inb && !(fabsf(cvb) < INFINITY)) bad |= 1 << i;
        }
        if (diag && bad) {
#pragma unroll
            for (int i = 0; i < PC_GK * PC_GT / PC_THREADS; ++i)
                if (bad & (1 << i)) {
                    if (atomicOr(&flags[base + 2 * i + rsub], 1) == 0) atomicAdd(&info[0], 1);
                }
        }
        __syncthreads();
        load_rows(base + PC_GK);
#pragma unroll 4
        for (int s = 0; s < PC_GK / 2; ++s) {
            const int kk = 2 * s + h;
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                av[i] = as[kk * PC_GLD + wm * 64 + i * 32 + li];
                bv[i] = bs[kk * PC_GLD + wn * 64 + i * 32 + li];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (on[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if ((base - lo + PC_GK) % PC_CHAIN == 0 || base + PC_GK >= hi) {        // the end of a chain: into float64
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        acc64[i][j][q] += (double)acc[i][j][q];
                        acc[i][j][q] = 0.f;
                    }
        }
    }
    double* out = part + (size_t)blockIdx.y * d * d;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = a0 + wm * 64 + i * 32 + pc_row(q, h), c = b0 + wn * 64 + j * 32 + li;
                if (r < d && c < d) out[(size_t)r * d + c] = acc64[i][j][q];
            }
}

// the ranges in ascending order; element (j, l) with j <= l lies in an upper-triangle tile, and both G[j][l] and G[l][j] get its sum
__global__ void __launch_bounds__(256) pca_gram_finish_kernel(const double* __restrict__ part, int d, int R, double* __restrict__ G) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)d * d) return;
    const int j = (int)(e / d), l = (int)(e % d);
    if (j > l) return;
    double a = 0.0;
    for (int q = 0; q < R; ++q) a += part[(size_t)q * d * d + e];
    G[(size_t)j * d + l] = a;
    G[(size_t)l * d + j] = a;
}

// ------------------------------------------------------------------------------------------------ pack W
__global__ void __launch_bounds__(256) pca_pack_kernel(const float* __restrict__ W, int m, int d, int mp, int dp, float* __restrict__ Wp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= mp * dp) return;
    const int comp = e / dp, q = e % dp;
    const int k = (q & ~7) + 2 * (q & 3) + ((q & 7) >> 2);
    Wp[e] = (comp < m && k < d) ? W[(size_t)comp * d + k] : 0.f;
}

// ------------------------------------------------------------------------------------------------ projection
template <int NT>
__global__ void __launch_bounds__(PC_THREADS) pca_fwd_kernel(const float* __restrict__ X, const float* __restrict__ shift, long long n, int d, int dp,
                                                             int m, int mp, const float* __restrict__ Wp, int unit, float* __restrict__ Y,
                                                             int* __restrict__ info) {
    __shared__ float xs[PC_RT * PC_XLD];
    __shared__ float red[4][PC_RT];             // per wave: the row's sum of squares over the wave's columns
    __shared__ int bad_s[PC_RT];
    const long long row0 = (long long)blockIdx.x * PC_RT;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;

    if (tid < PC_RT) bad_s[tid] = 0;

    f32x16 acc[NT];
    int woff[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
        const int comp = (t * 4 + wave) * 32 + li;
        woff[t] = (comp < mp ? comp : mp - 1) * dp + 4 * h;     // a tile past mp repeats the last row: computed, never used
    }

    // no branch around a load: the chunk after the current one is in registers while the MFMAs run (addresses clamped, values masked)
    float xr[PC_RT * PC_BK / PC_THREADS], sr;
    f32x4 bw[NT], bn[NT];
    auto load_x = [&](int k0) {
        const int k = k0 + (tid & 63), kc = k < d ? k : d - 1;
        sr = shift[kc];
#pragma unroll
        for (int i = 0; i < PC_RT * PC_BK / PC_THREADS; ++i) {
            const int row = (tid + PC_THREADS * i) >> 6;
            const long long g = row0 + row < n ? row0 + row : n - 1;
            xr[i] = X[(size_t)g * d + kc];
        }
    };
    load_x(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) bw[t] = *reinterpret_cast<const f32x4*>(Wp + woff[t]);
    for (int k0 = 0; k0 < dp; k0 += PC_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PC_RT * PC_BK / PC_THREADS; ++i) {
            const int idx = tid + PC_THREADS * i, row = idx >> 6, kk = idx & 63;
            xs[row * PC_XLD + kk] = (row0 + row < n && k0 + kk < d) ? xr[i] - sr : 0.f;
        }
        __syncthreads();
        load_x(k0 + PC_BK);
        const int kend = dp - k0 < PC_BK ? dp - k0 : PC_BK;     // a multiple of 8
        for (int k8 = 0; k8 < kend; k8 += 8) {
            const int kn = k0 + k8 + 8 < dp ? k0 + k8 + 8 : dp - 8;
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[t] = *reinterpret_cast<const f32x4*>(Wp + woff[t] + kn);
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = xs[li * PC_XLD + k8 + 2 * j + h];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bw[t][j], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) bw[t] = bn[t];
        }
    }

    // acc[t][q] = y of row pc_row(q, h), column (4 t + wave) * 32 + li
    float ss[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) ss[q] = 0.f;
    int bad = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const bool valid = (t * 4 + wave) * 32 + li < m;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float v = valid ? acc[t][q] : 0.f;            // the padded columns hold zeros by the packing, and are masked as well
            if (!(fabsf(v) < INFINITY)) bad |= 1 << q;
            ss[q] = fmaf(v, v, ss[q]);
        }
    }
    if (bad) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (bad & (1 << q)) atomicOr(&bad_s[pc_row(q, h)], 1);
    }
    float nrm[16];
    if (unit) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1)
#pragma unroll
            for (int q = 0; q < 16; ++q) ss[q] += __shfl_xor(ss[q], o, 64);
        if (li == 0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) red[wave][pc_row(q, h)] = ss[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = pc_row(q, h);
        nrm[q] = unit ? sqrtf(((red[0][row] + red[1][row]) + red[2][row]) + red[3][row]) : 1.f;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int comp = (t * 4 + wave) * 32 + li;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long g = row0 + pc_row(q, h);
            if (g < n && comp < m) {
                const float v = acc[t][q];
                Y[(size_t)g * m + comp] = unit ? (nrm[q] == 0.f ? 0.f : v / nrm[q]) : v;
            }
        }
    }
    if (tid < PC_RT && row0 + tid < n) {
        if (bad_s[tid]) atomicAdd(&info[0], 1);
        if (unit && sqrtf(((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) == 0.f) atomicAdd(&info[1], 1);
    }
}

struct pca_plan {
    int mp, dp, dp32, dtiles, tiles, R, RB;
    long long rows_per_range, cs_rows;
    size_t zeros, colpart, flags, part, wp, end;
};

static bool pca_shape_ok(int64_t n, int d, int m) { return n >= 1 && n < (1ll << 31) && d >= 1 && d <= PC_DMAX && m >= 1 && m <= PC_MMAX; }

static void pca_layout(int64_t n, int d, int m, pca_plan& p) {
    p.mp = (int)scd_cdiv(m, 32) * 32;
    p.dp = (int)scd_cdiv(d, 8) * 8;
    p.dp32 = (int)scd_cdiv(d, 32) * 32;
    p.dtiles = (int)scd_cdiv(d, PC_GT);
    p.tiles = p.dtiles * (p.dtiles + 1) / 2;
    // row ranges of the Gram matrix: at least four chains each, at most 32, about 1024 blocks; a whole number of chains per range
    const long long chains = scd_cdiv(n, PC_CHAIN);
    long long R = chains / 4, cap = scd_cdiv(1024, (long long)p.tiles);
    if (cap > 32) cap = 32;
    if (R > cap) R = cap;
    if (R < 1) R = 1;
    p.rows_per_range = scd_cdiv(chains, R) * PC_CHAIN;
    p.R = (int)scd_cdiv(n, p.rows_per_range);
    long long RB = scd_cdiv(n, PC_CS_ROWS);
    if (RB > PC_CS_RANGES) RB = PC_CS_RANGES;
    p.cs_rows = scd_cdiv(n, RB);
    p.RB = (int)scd_cdiv(n, p.cs_rows);
    p.zeros = 0;                                                                    // zeros   f32 [d]: the shift of a NULL shift
    p.colpart = p.zeros + scd_align((size_t)d * 4);                                 // colpart f64 [RB, dp32]
    p.flags = p.colpart + scd_align((size_t)p.RB * p.dp32 * 8);                     // flags   i32 [n]
    p.part = p.flags + scd_align((size_t)n * 4);                                    // part    f64 [R, d, d]
    p.wp = p.part + scd_align((size_t)p.R * d * d * 8);                             // Wp      f32 [mp, dp]
    p.end = p.wp + scd_align((size_t)p.mp * p.dp * 4);
}

extern "C" int scd_pca_row_tile(void) { return PC_RT; }
extern "C" int scd_pca_chain_rows(void) { return PC_CHAIN; }

extern "C" size_t scd_pca_ws_bytes(int64_t n, int d, int m) {
    if (!pca_shape_ok(n, d, m)) return 0;
    pca_plan p;
    pca_layout(n, d, m, p);
    return p.end;
}

#define PCA_SHAPE_REQUIRE(who)                                                                                    \
    SCD_REQUIRE(n >= 1 && n < (1ll << 31), who ": n = %lld outside [1, 2^31)", (long long)n);                     \
    SCD_REQUIRE(d >= 1 && d <= PC_DMAX, who ": d = %d outside [1, %d]", d, PC_DMAX);                              \
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, who ": workspace not 16-byte aligned")

// the shift the kernels read: the caller's, or the workspace's zeros (x - 0 is x, so no kernel branches on a NULL shift)
static int pca_shift(const float* shift, char* w, const pca_plan& p, int d, hipStream_t st, const float** out) {
    *out = shift;
    if (!shift) {
        SCD_HIP(hipMemsetAsync(w + p.zeros, 0, (size_t)d * 4, st));
        *out = (const float*)(w + p.zeros);
    }
    return SCD_OK;
}

extern "C" int scd_pca_colsum(scd_handle h, const float* X, const float* shift, int64_t n, int d, double* csum_out, void* ws, size_t ws_bytes,
                              void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_pca_colsum");
    SCD_REQUIRE(X && csum_out && ws, "scd_pca_colsum: null argument");
    PCA_SHAPE_REQUIRE("scd_pca_colsum");
    pca_plan p;
    pca_layout(n, d, 1, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_pca_colsum: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    const float* sh;
    const int rc = pca_shift(shift, w, p, d, st, &sh);
    if (rc != SCD_OK) return rc;
    double* colpart = (double*)(w + p.colpart);
    pca_colsum_kernel<<<dim3((unsigned)(p.dp32 / 32), (unsigned)p.RB), PC_THREADS, 0, st>>>(X, sh, n, d, p.dp32, p.cs_rows, colpart);
    pca_colsum_finish_kernel<<<(unsigned)scd_cdiv(d, 256), 256, 0, st>>>(colpart, d, p.dp32, p.RB, csum_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_pca_gram(scd_handle h, const float* X, const float* shift, int64_t n, int d, double* G_out, int32_t* info_out, void* ws,
                            size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_pca_gram");
    SCD_REQUIRE(X && G_out && info_out && ws, "scd_pca_gram: null argument");
    PCA_SHAPE_REQUIRE("scd_pca_gram");
    pca_plan p;
    pca_layout(n, d, 1, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_pca_gram: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    const float* sh;
    const int rc = pca_shift(shift, w, p, d, st, &sh);
    if (rc != SCD_OK) return rc;
    int* flags = (int*)(w + p.flags);
    double* part = (double*)(w + p.part);
    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    SCD_HIP(hipMemsetAsync(flags, 0, (size_t)n * 4, st));
    pca_gram_kernel<<<dim3((unsigned)p.tiles, (unsigned)p.R), PC_THREADS, 0, st>>>(X, sh, n, d, p.dtiles, p.rows_per_range, part, flags, info_out);
    pca_gram_finish_kernel<<<(unsigned)scd_cdiv((int64_t)d * d, 256), 256, 0, st>>>(part, d, p.R, G_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_pca_transform(scd_handle h, const float* X, const float* shift, const float* W, int64_t n, int d, int m, int unit,
                                 float* Y_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_pca_transform");
    SCD_REQUIRE(X && W && Y_out && info_out && ws, "scd_pca_transform: null argument");
    PCA_SHAPE_REQUIRE("scd_pca_transform");
    SCD_REQUIRE(m >= 1 && m <= PC_MMAX, "scd_pca_transform: m = %d outside [1, %d]", m, PC_MMAX);
    pca_plan p;
    pca_layout(1, d, m, p);                                     // only the zeros and the packed W are needed
    SCD_REQUIRE(ws_bytes >= p.end, "scd_pca_transform: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    const float* sh;
    const int rc = pca_shift(shift, w, p, d, st, &sh);
    if (rc != SCD_OK) return rc;
    float* Wp = (float*)(w + p.wp);
    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    pca_pack_kernel<<<(unsigned)scd_cdiv((int64_t)p.mp * p.dp, 256), 256, 0, st>>>(W, m, d, p.mp, p.dp, Wp);
    const int per = (int)scd_cdiv(p.mp / 32, 4);                // the column tiles of a wave, rounded up to 1, 2, 4 or 8
    const unsigned grid = (unsigned)scd_cdiv(n, PC_RT);
    const int un = unit ? 1 : 0;
    if (per <= 1) pca_fwd_kernel<1><<<grid, PC_THREADS, 0, st>>>(X, sh, n, d, p.dp, m, p.mp, Wp, un, Y_out, info_out);
    else if (per <= 2) pca_fwd_kernel<2><<<grid, PC_THREADS, 0, st>>>(X, sh, n, d, p.dp, m, p.mp, Wp, un, Y_out, info_out);
    else if (per <= 4) pca_fwd_kernel<4><<<grid, PC_THREADS, 0, st>>>(X, sh, n, d, p.dp, m, p.mp, Wp, un, Y_out, info_out);
    else pca_fwd_kernel<8><<<grid, PC_THREADS, 0, st>>>(X, sh, n, d, p.dp, m, p.mp, Wp, un, Y_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
