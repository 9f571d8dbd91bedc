// Principal component analysis on gfx950: the centred Gram matrix of a feature cache and the projection onto its components, without a
// centred or float64 copy of the rows (scikit-learn 1.7's PCA(svd_solver='covariance_eigh'); the eigensolver of the d x d matrix runs on
// the host).  docs/design/pca.md has the semantics, the error model and the resources.
// The tile shapes, the k-octet packing, the float64 range sums and the host's range plan are f32mm.h's, shared with probe.hip and gmm.hip.
//
// Every kernel sees the rows as c_ij = fl32(x_ij - shift_j): one IEEE float32 subtraction in a register, as the value is staged.
//
//   scd_pca_colsum      float64 column sums of c: pca_colsum_kernel over RB row ranges of fixed size -> colpart [RB, d];
//                       pca_colsum_finish_kernel adds the ranges in ascending order.
//   scd_pca_gram        G = c^T c in float64: pca_gram_kernel on 128 x 128 tiles of (dim, dim), upper-triangle tiles only, times R row
//                       ranges; both operands go through LDS 32 rows at a time, the float32 MFMA (v_mfma_f32_32x32x2_f32) runs over
//                       chains of at most F32MM_CHAIN = 256 rows, each chain's tile is added into float64 registers; a range's float64 tile
//                       -> part [R, d, d].  pca_gram_finish_kernel adds the ranges in ascending order and writes G[j][l] and G[l][j]
//                       (j <= l) from the same sum: G is bit-symmetric.
//   scd_pca_transform   y_ik = sum_j c_ij W_kj: pca_pack_kernel packs W [m, d] by k-octet (probe.hip's packing); pca_fwd_kernel: a block
//                       owns F32MM_RT = 32 rows and all m columns (up to 32), wave w the 32-column tiles w, w + 4, ... in up to 8 accumulator
//                       tiles; c goes through LDS in chunks of 64 j, the packed W streams from L2; the sum over j ascends from a zero
//                       accumulator.  unit: the float32 sum of squares over the real m columns (lanes by shuffles, waves through LDS in
//                       wave order), sqrtf and a division, both correctly rounded; a row of norm 0 is written as zeros.
//
// No floating-point atomics (the info counters and the row flags are integers).  R, RB and every tile depend on (n, d, m) alone: two
// calls return the same bits on any device.
#include "f32mm.h"

// ------------------------------------------------------------------------------------------------ column sums
// grid (d up to 32 / 32, RB): float64 column sums of c over a row range -> colpart [RB, dp32]
__global__ void __launch_bounds__(F32MM_THREADS) pca_colsum_kernel(const float* __restrict__ X, const float* __restrict__ shift, long long n, int d,
                                                                   int dp32, long long rows_per_range, double* __restrict__ colpart) {
    __shared__ double sh[F32MM_THREADS];
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
    const int tid = threadIdx.x, col = blockIdx.x * 32 + (tid & 31), cc = col < d ? col : d - 1;
    const float sv = shift[cc];
    const double t = f32mm_colsum(lo, hi, [&](long long g) { return X[(size_t)g * d + cc] - sv; }, sh);
    if (tid < 32) colpart[(size_t)blockIdx.y * dp32 + col] = t;
}

__global__ void __launch_bounds__(256) pca_colsum_finish_kernel(const double* __restrict__ colpart, int d, int dp32, int RB,
                                                                double* __restrict__ csum) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    csum[col] = f32mm_range_sum(colpart, dp32, col, RB);
}

// ------------------------------------------------------------------------------------------------ Gram partials
// grid (upper-triangle tiles, R).  Tile t is (ti, tj) with ti <= tj: rows ti * 128 ... of G against columns tj * 128 ...; part [R, d, d]
// float64, of which the tile's elements alone are written.  flags int [n]: a row that holds a non-finite c is counted once in info[0]
// (the diagonal tiles see every column exactly once).
__global__ void __launch_bounds__(F32MM_THREADS) pca_gram_kernel(const float* __restrict__ X, const float* __restrict__ shift, long long n, int d,
                                                              int dtiles, long long rows_per_range, double* __restrict__ part,
                                                              int* __restrict__ flags, int* __restrict__ info) {
    __shared__ float as[F32MM_GK * F32MM_GLD];
    __shared__ float bs[F32MM_GK * F32MM_GLD];
    // the tile of this block: row ti of the triangle holds dtiles - ti tiles
    int ti = 0, rem = blockIdx.x;
    while (rem >= dtiles - ti) {
        rem -= dtiles - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int a0 = ti * F32MM_GT, b0 = tj * F32MM_GT;
    const bool diag = ti == tj;
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
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
    float ar[F32MM_GK * F32MM_GT / F32MM_THREADS], br[F32MM_GK * F32MM_GT / F32MM_THREADS];
    auto load_rows = [&](long long base) {
#pragma unroll
        for (int i = 0; i < F32MM_GK * F32MM_GT / F32MM_THREADS; ++i) {
            const long long gr = base + 2 * i + rsub;
            const long long g = gr < hi ? gr : hi - 1;
            ar[i] = X[(size_t)g * d + ca];
            br[i] = X[(size_t)g * d + cb];
        }
    };
    load_rows(lo);
    for (long long base = lo; base < hi; base += F32MM_GK) {
        __syncthreads();
        int bad = 0;
#pragma unroll
        for (int i = 0; i < F32MM_GK * F32MM_GT / F32MM_THREADS; ++i) {
            const int row = 2 * i + rsub;
            const bool in = base + row < hi;
            const float cva = ar[i] - sa, cvb = br[i] - sb;
            as[row * F32MM_GLD + col] = (in && ina) ? cva : 0.f;
            bs[row * F32MM_GLD + col] = (in && inb) ? cvb : 0.f;
            if (in && inb && !(fabsf(cvb) < INFINITY)) bad |= 1 << i;
        }
        if (diag && bad) {
#pragma unroll
            for (int i = 0; i < F32MM_GK * F32MM_GT / F32MM_THREADS; ++i)
                if (bad & (1 << i)) {
                    if (atomicOr(&flags[base + 2 * i + rsub], 1) == 0) atomicAdd(&info[0], 1);
                }
        }
        __syncthreads();
        load_rows(base + F32MM_GK);
#pragma unroll 4
        for (int s = 0; s < F32MM_GK / 2; ++s) {
            const int kk = 2 * s + h;
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                av[i] = as[kk * F32MM_GLD + wm * 64 + i * 32 + li];
                bv[i] = bs[kk * F32MM_GLD + wn * 64 + i * 32 + li];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (on[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if ((base - lo + F32MM_GK) % F32MM_CHAIN == 0 || base + F32MM_GK >= hi) {  // the end of a chain: into float64
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
                const int r = a0 + wm * 64 + i * 32 + f32mm_row(q, h), c = b0 + wn * 64 + j * 32 + li;
                if (r < d && c < d) out[(size_t)r * d + c] = acc64[i][j][q];
            }
}

// the ranges in ascending order; element (j, l) with j <= l lies in an upper-triangle tile, and both G[j][l] and G[l][j] get its sum
__global__ void __launch_bounds__(256) pca_gram_finish_kernel(const double* __restrict__ part, int d, int R, double* __restrict__ G) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)d * d) return;
    const int j = (int)(e / d), l = (int)(e % d);
    if (j > l) return;
    const double a = f32mm_range_sum(part, (size_t)d * d, e, R);
    G[(size_t)j * d + l] = a;
    G[(size_t)l * d + j] = a;
}

// ------------------------------------------------------------------------------------------------ pack W
__global__ void __launch_bounds__(256) pca_pack_kernel(const float* __restrict__ W, int m, int d, int mp, int dp, float* __restrict__ Wp) {
    const float* const src[1] = {W};
    f32mm_pack<1>(src, m, d, mp, dp, Wp);
}

// ------------------------------------------------------------------------------------------------ projection
template <int NT>
__global__ void __launch_bounds__(F32MM_THREADS) pca_fwd_kernel(const float* __restrict__ X, const float* __restrict__ shift, long long n, int d, int dp,
                                                             int m, int mp, const float* __restrict__ Wp, int unit, float* __restrict__ Y,
                                                             int* __restrict__ info) {
    __shared__ float xs[F32MM_RT * F32MM_XLD];
    __shared__ float red[4][F32MM_RT];          // per wave: the row's sum of squares over the wave's columns
    __shared__ int bad_s[F32MM_RT];
    const long long row0 = (long long)blockIdx.x * F32MM_RT;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;

    if (tid < F32MM_RT) bad_s[tid] = 0;

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
    float xr[F32MM_RT * F32MM_BK / F32MM_THREADS], sr;
    f32x4 bw[NT], bn[NT];
    auto load_x = [&](int k0) {
        const int k = k0 + (tid & 63), kc = k < d ? k : d - 1;
        sr = shift[kc];
#pragma unroll
        for (int i = 0; i < F32MM_RT * F32MM_BK / F32MM_THREADS; ++i) {
            const int row = (tid + F32MM_THREADS * i) >> 6;
            const long long g = row0 + row < n ? row0 + row : n - 1;
            xr[i] = X[(size_t)g * d + kc];
        }
    };
    load_x(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) bw[t] = *reinterpret_cast<const f32x4*>(Wp + woff[t]);
    for (int k0 = 0; k0 < dp; k0 += F32MM_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < F32MM_RT * F32MM_BK / F32MM_THREADS; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx >> 6, kk = idx & 63;
            xs[row * F32MM_XLD + kk] = (row0 + row < n && k0 + kk < d) ? xr[i] - sr : 0.f;
        }
        __syncthreads();
        load_x(k0 + F32MM_BK);
        const int kend = dp - k0 < F32MM_BK ? dp - k0 : F32MM_BK;               // a multiple of 8
        for (int k8 = 0; k8 < kend; k8 += 8) {
            const int kn = k0 + k8 + 8 < dp ? k0 + k8 + 8 : dp - 8;
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[t] = *reinterpret_cast<const f32x4*>(Wp + woff[t] + kn);
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = xs[li * F32MM_XLD + k8 + 2 * j + h];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bw[t][j], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) bw[t] = bn[t];
        }
    }

    // acc[t][q] = y of row f32mm_row(q, h), column (4 t + wave) * 32 + li
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
            if (bad & (1 << q)) atomicOr(&bad_s[f32mm_row(q, h)], 1);
    }
    float nrm[16];
    if (unit) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1)
#pragma unroll
            for (int q = 0; q < 16; ++q) ss[q] += __shfl_xor(ss[q], o, 64);
        if (li == 0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) red[wave][f32mm_row(q, h)] = ss[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = f32mm_row(q, h);
        nrm[q] = unit ? sqrtf(((red[0][row] + red[1][row]) + red[2][row]) + red[3][row]) : 1.f;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int comp = (t * 4 + wave) * 32 + li;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const long long g = row0 + f32mm_row(q, h);
            if (g < n && comp < m) {
                const float v = acc[t][q];
                Y[(size_t)g * m + comp] = unit ? (nrm[q] == 0.f ? 0.f : v / nrm[q]) : v;
            }
        }
    }
    if (tid < F32MM_RT && row0 + tid < n) {
        if (bad_s[tid]) atomicAdd(&info[0], 1);
        if (unit && sqrtf(((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) == 0.f) atomicAdd(&info[1], 1);
    }
}

struct pca_plan {
    int mp, dp, dp32, dtiles, tiles, R, RB;
    long long rows_per_range, cs_rows;
    size_t zeros, colpart, flags, part, wp, end;
};

static void pca_layout(int64_t n, int d, int m, pca_plan& p) {
    p.mp = f32mm_pad(m, 32);
    p.dp = f32mm_pad(d, 8);
    p.dp32 = f32mm_pad(d, 32);
    p.dtiles = (int)scd_cdiv(d, F32MM_GT);
    p.tiles = p.dtiles * (p.dtiles + 1) / 2;
    f32mm_ranges(n, p.tiles, 1024, p.R, p.rows_per_range);
    f32mm_colsum_ranges(n, p.RB, p.cs_rows);
    p.zeros = 0;                                                                    // zeros   f32 [d]: the shift of a NULL shift
    p.colpart = p.zeros + scd_align((size_t)d * 4);                                 // colpart f64 [RB, dp32]
    p.flags = p.colpart + scd_align((size_t)p.RB * p.dp32 * 8);                     // flags   i32 [n]
    p.part = p.flags + scd_align((size_t)n * 4);                                    // part    f64 [R, d, d]
    p.wp = p.part + scd_align((size_t)p.R * d * d * 8);                             // Wp      f32 [mp, dp]
    p.end = p.wp + scd_align((size_t)p.mp * p.dp * 4);
}

extern "C" int scd_pca_row_tile(void) { return F32MM_RT; }
extern "C" int scd_pca_chain_rows(void) { return F32MM_CHAIN; }

extern "C" size_t scd_pca_ws_bytes(int64_t n, int d, int m) {
    if (!f32mm_shape_ok(n, d, m, 1)) return 0;
    pca_plan p;
    pca_layout(n, d, m, p);
    return p.end;
}

#define PCA_SHAPE_REQUIRE(who) \
    F32MM_ND_REQUIRE(who, n, d);  \
    F32MM_WS_REQUIRE(who, ws)

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
    pca_colsum_kernel<<<dim3((unsigned)(p.dp32 / 32), (unsigned)p.RB), F32MM_THREADS, 0, st>>>(X, sh, n, d, p.dp32, p.cs_rows, colpart);
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
    pca_gram_kernel<<<dim3((unsigned)p.tiles, (unsigned)p.R), F32MM_THREADS, 0, st>>>(X, sh, n, d, p.dtiles, p.rows_per_range, part, flags,
                                                                                      info_out);
    pca_gram_finish_kernel<<<(unsigned)scd_cdiv((int64_t)d * d, 256), 256, 0, st>>>(part, d, p.R, G_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_pca_transform(scd_handle h, const float* X, const float* shift, const float* W, int64_t n, int d, int m, int unit,
                                 float* Y_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_pca_transform");
    SCD_REQUIRE(X && W && Y_out && info_out && ws, "scd_pca_transform: null argument");
    PCA_SHAPE_REQUIRE("scd_pca_transform");
    F32MM_WIDTH_REQUIRE("scd_pca_transform", "m", m, 1);
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
    f32mm_fwd_dispatch(n, p.mp, [&](unsigned grid, auto nt) {
        pca_fwd_kernel<decltype(nt)::value><<<grid, F32MM_THREADS, 0, st>>>(X, sh, n, d, p.dp, m, p.mp, Wp, unit ? 1 : 0, Y_out, info_out);
    });
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
