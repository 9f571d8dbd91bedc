// Exact t-SNE on gfx950 (van der Maaten & Hinton, JMLR 2008; the optimiser of scikit-learn 1.7's sklearn/manifold/_t_sne.py, which the
// reference's save_tsne calls: local_utils/util.py:178-216).  docs/design/tsne.md has the definitions, the error bound and the numbers.
//
//   scd_tsne_calibrate   tsne_calibrate_kernel, a wave per row, a lane per neighbour (k <= 64), float64: the conditional row
//                        p_j = exp(-b (d_j - d_min)) / sum with b the root of H(b) = log(perplexity).  The search starts at b = 1, doubles or
//                        halves until the root is bracketed, then bisects; TSNE_SEARCH_STEPS steps, no exit on a tolerance.
//   scd_tsne_gradient    tsne_repulse_kernel   the all-pairs sums (sum q^2 dx, sum q^2 dy, sum q) per row and column range, fp32 pairs
//                                              folded into float64 every TSNE_RUN columns;
//                        tsne_attract_kernel   the CSR sums sum_j P_ij q_ij (y_i - y_j) in float64, a wave per row, and the row's shares of KL;
//                        tsne_finish_kernel    the ranges of a row in range order;
//                        tsne_reduce_kernel    Z and KL over the rows: a fixed partition and tree, one block;
//                        tsne_combine_kernel   grad = 4 (a attract - repulse / Z).
//   scd_tsne_update      tsne_update_kernel    scikit-learn's _gradient_descent step (gains, velocity, step) in float64, and the fp32 copy.
//
// No floating-point atomics anywhere: two calls return the same bits.  This file is compiled with -ffp-contract=off (build.py): every
// fused multiply-add below is written as one, and the update step is the IEEE operations numpy performs.
#include "common.h"

#define TSNE_KMAX 64
#define TSNE_SEARCH_STEPS 200
#define TSNE_THREADS 256
#define TSNE_RPL 4                                  // rows per lane
#define TSNE_ROWS (TSNE_THREADS * TSNE_RPL)         // R: the row tile of a block
#define TSNE_CHUNK 1024                             // C: columns staged in LDS at a time
#define TSNE_RUN 64                                 // the longest fp32 run: columns summed in fp32 before the fold into float64
#define TSNE_YMAX 32
#define TSNE_YLIMIT 1152921504606846976.0f          // 2^60

// ------------------------------------------------------------------------------------------------ calibration
__global__ void __launch_bounds__(256) tsne_calibrate_kernel(const double* __restrict__ dist2, long long n, int k, double log_perp,
                                                            double* __restrict__ p_out, double* __restrict__ beta_out, int* __restrict__ info) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const bool live = lane < k;
    const double raw = live ? dist2[(size_t)i * k + lane] : INFINITY;
    const bool bad_lane = live && !(raw >= 0.0 && raw < INFINITY);
    if (__ballot(bad_lane) != 0ull) {                           // a negative or non-finite distance: a uniform row, counted
        if (live) p_out[(size_t)i * k + lane] = 1.0 / (double)k;
        if (lane == 0) {
            beta_out[i] = NAN;
            atomicAdd(&info[1], 1);
        }
        return;
    }
    double dmin = raw;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmin = fmin(dmin, __shfl_xor(dmin, o, 64));
    const double d = live ? raw - dmin : 0.0;
    double beta = 1.0, lo = -INFINITY, hi = INFINITY;
    for (int step = 0; step < TSNE_SEARCH_STEPS; ++step) {
        const double e = live ? exp(-d * beta) : 0.0;
        const double s = wave_sum_f64(e);                       // >= 1: the nearest neighbour has d = 0
        const double sd = wave_sum_f64(d * e);
        const double H = log(s) + beta * sd / s;
        if (H - log_perp > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : (beta + hi) * 0.5;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5 : (beta + lo) * 0.5;
        }
    }
    const double e = live ? exp(-d * beta) : 0.0;
    const double s = wave_sum_f64(e);
    if (live) p_out[(size_t)i * k + lane] = e / s;
    if (lane == 0) {
        beta_out[i] = beta;
        if (hi == INFINITY || lo == -INFINITY) atomicAdd(&info[0], 1);      // never bracketed: the entropy cannot reach the target
    }
}

extern "C" int scd_tsne_calibrate(scd_handle h, const double* dist2, int64_t n, int k, double perplexity, double* p_out, double* beta_out,
                                  int32_t* info_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_tsne_calibrate");
    SCD_REQUIRE(dist2 && p_out && beta_out && info_out, "scd_tsne_calibrate: null argument");
    SCD_REQUIRE(n >= 1 && n < (1ll << 31), "scd_tsne_calibrate: n = %lld outside [1, 2^31)", (long long)n);
    SCD_REQUIRE(k >= 2 && k <= TSNE_KMAX, "scd_tsne_calibrate: k = %d outside [2, %d]", k, TSNE_KMAX);
    SCD_REQUIRE(perplexity > 1.0 && perplexity < (double)k, "scd_tsne_calibrate: the perplexity must lie in (1, k = %d)", k);
    hipStream_t st = (hipStream_t)stream_;
    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    tsne_calibrate_kernel<<<(unsigned)scd_cdiv(n, 4), 256, 0, st>>>(dist2, n, k, log(perplexity), p_out, beta_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ repulsion: all pairs
// One pair in fp32 (T = float): dx, dy (one rounding each), d2 = fma(dx, dx, fma(dy, dy, 1)) (two), q = v_rcp_f32(d2) (1 ulp), t = q q
// (one), the three running sums (one each).  T = double (SCD_TSNE_EXACT_PAIRS) is the same loop with float64 pairs and a division.
// CHECK: the chunk holds the tile's own columns or columns >= n, excluded by index.
__device__ __forceinline__ float tsne_rcp(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ double tsne_rcp(double v) { return 1.0 / v; }
__device__ __forceinline__ float tsne_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double tsne_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

template <typename T, bool CHECK>
__device__ __forceinline__ void tsne_run(const float2* __restrict__ sY, int c_lo, long long col0, long long n, const long long (&row)[TSNE_RPL],
                                         const T (&x)[TSNE_RPL], const T (&y)[TSNE_RPL], T (&fx)[TSNE_RPL], T (&fy)[TSNE_RPL], T (&fz)[TSNE_RPL]) {
#pragma unroll 8
    for (int c = c_lo; c < c_lo + TSNE_RUN; ++c) {
        const float2 yj = sY[c];                                // the same address in every lane: an LDS broadcast
        const long long col = col0 + c;
#pragma unroll
        for (int r = 0; r < TSNE_RPL; ++r) {
            const T dx = x[r] - (T)yj.x, dy = y[r] - (T)yj.y;
            const T d2 = tsne_fma(dx, dx, tsne_fma(dy, dy, (T)1));
            T q = tsne_rcp(d2);
            if (CHECK) q = (col != row[r] && col < n) ? q : (T)0;
            const T t = q * q;
            fx[r] = tsne_fma(t, dx, fx[r]);
            fy[r] = tsne_fma(t, dy, fy[r]);
            fz[r] += q;
        }
    }
}

// part [ny, n, 3] float64: per column range and row (sum q^2 dx, sum q^2 dy, sum q) over the range's columns j != i, j < n.
template <typename T>
__global__ void __launch_bounds__(TSNE_THREADS) tsne_repulse_kernel(const float2* __restrict__ Y, long long n, long long chunks,
                                                                    long long chunks_per_y, double* __restrict__ part) {
    __shared__ float2 sY[TSNE_CHUNK];
    const long long row0 = (long long)blockIdx.x * TSNE_ROWS;
    const int tid = threadIdx.x;
    long long ch_lo = (long long)blockIdx.y * chunks_per_y, ch_hi = ch_lo + chunks_per_y;
    if (ch_hi > chunks) ch_hi = chunks;
    long long row[TSNE_RPL];
    T x[TSNE_RPL], y[TSNE_RPL];
    double ax[TSNE_RPL], ay[TSNE_RPL], az[TSNE_RPL];
#pragma unroll
    for (int r = 0; r < TSNE_RPL; ++r) {
        row[r] = row0 + r * TSNE_THREADS + tid;                 // consecutive lanes, consecutive rows
        const float2 v = row[r] < n ? Y[row[r]] : float2{0.f, 0.f};
        x[r] = (T)v.x;
        y[r] = (T)v.y;
        ax[r] = ay[r] = az[r] = 0.0;
    }
    for (long long ch = ch_lo; ch < ch_hi; ++ch) {
        const long long col0 = ch * TSNE_CHUNK;
        __syncthreads();                                        // the previous chunk has been read
#pragma unroll
        for (int s = 0; s < TSNE_CHUNK / TSNE_THREADS; ++s) {
            const long long j = col0 + s * TSNE_THREADS + tid;
            sY[s * TSNE_THREADS + tid] = j < n ? Y[j] : float2{0.f, 0.f};
        }
        __syncthreads();
        // the same in every lane of the block: this chunk holds a padding column, or one of the tile's own columns
        const bool check = col0 + TSNE_CHUNK > n || (col0 < row0 + TSNE_ROWS && col0 + TSNE_CHUNK > row0);
        for (int c_lo = 0; c_lo < TSNE_CHUNK; c_lo += TSNE_RUN) {
            if (col0 + c_lo >= n) break;                        // nothing but padding from here on
            T fx[TSNE_RPL], fy[TSNE_RPL], fz[TSNE_RPL];
#pragma unroll
            for (int r = 0; r < TSNE_RPL; ++r) fx[r] = fy[r] = fz[r] = (T)0;
            if (check)
                tsne_run<T, true>(sY, c_lo, col0, n, row, x, y, fx, fy, fz);
            else
                tsne_run<T, false>(sY, c_lo, col0, n, row, x, y, fx, fy, fz);
#pragma unroll
            for (int r = 0; r < TSNE_RPL; ++r) {
                ax[r] += (double)fx[r];
                ay[r] += (double)fy[r];
                az[r] += (double)fz[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TSNE_RPL; ++r)
        if (row[r] < n) {
            double* o = part + ((size_t)blockIdx.y * n + row[r]) * 3;
            o[0] = ax[r];
            o[1] = ay[r];
            o[2] = az[r];
        }
}

// ------------------------------------------------------------------------------------------------ attraction: the CSR rows
// A wave per row; lane l takes the row's entries l, l + 64, ... in column order, then a fixed butterfly.  rowv [n, 4] = (sum P q dx,
// sum P q dy, sum P (log P - log q), sum P).  An indptr pair outside 0 <= lo <= hi <= nnz, a column outside [0, n) and a row of Y that is not
// finite below 2^60 are counted (info[0], info[0], info[1]) and skipped: nothing is read out of range.
__global__ void __launch_bounds__(256) tsne_attract_kernel(const float2* __restrict__ Y, const long long* __restrict__ indptr,
                                                          const int* __restrict__ indices, const double* __restrict__ values, long long n,
                                                          long long nnz, int want_kl, double* __restrict__ rowv, int* __restrict__ info) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const float2 yi = Y[i];
    const bool y_ok = fabsf(yi.x) < TSNE_YLIMIT && fabsf(yi.y) < TSNE_YLIMIT;          // false for NaN and inf too
    long long lo = indptr[i], hi = indptr[i + 1];
    bool bad = !(lo >= 0 && lo <= hi && hi <= nnz);
    if (bad) lo = hi = 0;
    double sx = 0.0, sy = 0.0, sk = 0.0, sp = 0.0;
    for (long long e = lo + lane; e < hi; e += 64) {
        const long long j = indices[e];
        if (j < 0 || j >= n) {
            bad = true;
            continue;
        }
        const double p = values[e];
        const float2 yj = Y[j];
        const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y;
        const double d2 = dx * dx + dy * dy;
        const double w = p / (1.0 + d2);
        sx += w * dx;
        sy += w * dy;
        sp += p;
        if (want_kl && p > 0.0) sk += p * (log(p) + log1p(d2));
    }
    sx = wave_sum_f64(sx);
    sy = wave_sum_f64(sy);
    sk = wave_sum_f64(sk);
    sp = wave_sum_f64(sp);
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
        double* o = rowv + (size_t)i * 4;
        o[0] = sx;
        o[1] = sy;
        o[2] = sk;
        o[3] = sp;
        if (any_bad) atomicAdd(&info[0], 1);
        if (!y_ok) atomicAdd(&info[1], 1);
    }
}

// rep [n, 3] = the ranges of part in range order
__global__ void __launch_bounds__(256) tsne_finish_kernel(const double* __restrict__ part, long long n, int ny, double* __restrict__ rep) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * 3) return;
    double s = 0.0;
    for (int yy = 0; yy < ny; ++yy) s += part[(size_t)yy * n * 3 + e];
    rep[e] = s;
}

// One block of 1024 threads: thread t sums rows t, t + 1024, ... in row order, then an LDS tree.  zk[0] = Z, zk[1] = KL.
__global__ void __launch_bounds__(1024) tsne_reduce_kernel(const double* __restrict__ rep, const double* __restrict__ rowv, long long n, int want_kl,
                                                          double* __restrict__ zk) {
    __shared__ double sz[1024], sk[1024], sp[1024];
    const int t = threadIdx.x;
    double z = 0.0, kk = 0.0, pp = 0.0;
    for (long long i = t; i < n; i += 1024) {
        z += rep[(size_t)i * 3 + 2];
        kk += rowv[(size_t)i * 4 + 2];
        pp += rowv[(size_t)i * 4 + 3];
    }
    sz[t] = z;
    sk[t] = kk;
    sp[t] = pp;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) {
            sz[t] += sz[t + o];
            sk[t] += sk[t + o];
            sp[t] += sp[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        zk[0] = sz[0];
        zk[1] = want_kl ? sk[0] + log(sz[0]) * sp[0] : NAN;
    }
}

__global__ void __launch_bounds__(256) tsne_combine_kernel(const double* __restrict__ rep, const double* __restrict__ rowv, const double* __restrict__ zk,
                                                           long long n, double exaggeration, double* __restrict__ grad, double* __restrict__ z_out,
                                                           double* __restrict__ kl_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const double Z = zk[0];
    if (i == 0) {
        z_out[0] = Z;
        if (kl_out) kl_out[0] = zk[1];
    }
    if (i >= n) return;
    grad[i * 2 + 0] = 4.0 * (exaggeration * rowv[(size_t)i * 4 + 0] - rep[(size_t)i * 3 + 0] / Z);
    grad[i * 2 + 1] = 4.0 * (exaggeration * rowv[(size_t)i * 4 + 1] - rep[(size_t)i * 3 + 1] / Z);
}

struct tsne_plan {
    long long chunks, tiles;
    int ny_max;
    size_t part, rep, rowv, zk, end;
};

static bool tsne_shape_ok(int64_t n, int64_t nnz) { return n >= 2 && n < (1ll << 31) && nnz >= 0 && nnz < (1ll << 40); }

static void tsne_layout(int64_t n, tsne_plan& p) {
    p.chunks = scd_cdiv(n, TSNE_CHUNK);
    p.tiles = scd_cdiv(n, TSNE_ROWS);
    p.ny_max = (int)(p.chunks < TSNE_YMAX ? p.chunks : TSNE_YMAX);
    p.part = 0;                                                                     // part f64 [ny_max, n, 3]
    p.rep = p.part + scd_align((size_t)p.ny_max * n * 24);                          // rep  f64 [n, 3]
    p.rowv = p.rep + scd_align((size_t)n * 24);                                     // rowv f64 [n, 4]
    p.zk = p.rowv + scd_align((size_t)n * 32);                                      // zk   f64 [2]
    p.end = p.zk + scd_align(16);
}

extern "C" int scd_tsne_row_tile(void) { return TSNE_ROWS; }
extern "C" int scd_tsne_col_chunk(void) { return TSNE_CHUNK; }

extern "C" size_t scd_tsne_gradient_ws_bytes(int64_t n, int64_t nnz) {
    if (!tsne_shape_ok(n, nnz)) return 0;
    tsne_plan p;
    tsne_layout(n, p);
    return p.end;
}

extern "C" int scd_tsne_gradient(scd_handle h, const float* Y, const int64_t* indptr, const int32_t* indices, const double* values, int64_t n,
                                 int64_t nnz, double exaggeration, int flags, double* grad_out, double* z_out, double* kl_out, int32_t* info_out,
                                 void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_tsne_gradient");
    SCD_REQUIRE(Y && indptr && grad_out && z_out && info_out && ws, "scd_tsne_gradient: null argument");
    SCD_REQUIRE(n >= 2 && n < (1ll << 31), "scd_tsne_gradient: n = %lld outside [2, 2^31)", (long long)n);
    SCD_REQUIRE(nnz >= 0 && nnz < (1ll << 40), "scd_tsne_gradient: nnz = %lld outside [0, 2^40)", (long long)nnz);
    SCD_REQUIRE(nnz == 0 || (indices && values), "scd_tsne_gradient: null indices or values with nnz > 0");
    SCD_REQUIRE(exaggeration > 0.0 && exaggeration < INFINITY, "scd_tsne_gradient: the exaggeration must be positive and finite");
    SCD_REQUIRE((flags & ~SCD_TSNE_EXACT_PAIRS) == 0, "scd_tsne_gradient: unknown flags %d", flags);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0 && (uintptr_t)Y % 8 == 0, "scd_tsne_gradient: workspace not 16-byte or Y not 8-byte aligned");
    tsne_plan p;
    tsne_layout(n, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_tsne_gradient: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    double* part = (double*)(w + p.part);
    double* rep = (double*)(w + p.rep);
    double* rowv = (double*)(w + p.rowv);
    double* zk = (double*)(w + p.zk);
    // column ranges (grid.y) when the row tiles alone do not give four blocks per compute unit; the sums of a range are combined in
    // range order, so the result depends on the device's compute-unit count alone
    long long ny = scd_cdiv(4ll * h->n_cu, p.tiles);
    if (ny > p.ny_max) ny = p.ny_max;
    if (ny < 1) ny = 1;
    const long long chunks_per_y = scd_cdiv(p.chunks, ny);
    ny = scd_cdiv(p.chunks, chunks_per_y);                      // no empty range
    const int want_kl = kl_out != nullptr;
    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    const dim3 grid((unsigned)p.tiles, (unsigned)ny);
    if (flags & SCD_TSNE_EXACT_PAIRS)
        tsne_repulse_kernel<double><<<grid, TSNE_THREADS, 0, st>>>((const float2*)Y, n, p.chunks, chunks_per_y, part);
    else
        tsne_repulse_kernel<float><<<grid, TSNE_THREADS, 0, st>>>((const float2*)Y, n, p.chunks, chunks_per_y, part);
    tsne_attract_kernel<<<(unsigned)scd_cdiv(n, 4), 256, 0, st>>>((const float2*)Y, (const long long*)indptr, indices, values, n, nnz, want_kl, rowv,
                                                                   info_out);
    tsne_finish_kernel<<<(unsigned)scd_cdiv(n * 3, 256), 256, 0, st>>>(part, n, (int)ny, rep);
    tsne_reduce_kernel<<<1, 1024, 0, st>>>(rep, rowv, n, want_kl, zk);
    tsne_combine_kernel<<<(unsigned)scd_cdiv(n, 256), 256, 0, st>>>(rep, rowv, zk, n, exaggeration, grad_out, z_out, kl_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ the update step
// _gradient_descent (sklearn/manifold/_t_sne.py) on 2 n elements: inc = vel * grad < 0; gains += 0.2 where inc, *= 0.8 elsewhere, floored;
// vel = momentum vel - learning_rate (gains grad); Y64 += vel; Y32 = Y64 rounded to nearest.  gg_out (may be NULL) = gains grad, whose
// norm is the optimiser's stopping value.
__global__ void __launch_bounds__(256) tsne_update_kernel(const double* __restrict__ grad, double* __restrict__ Y64, double* __restrict__ vel,
                                                          double* __restrict__ gains, float* __restrict__ Y32, long long m, double momentum,
                                                          double learning_rate, double min_gain, double* __restrict__ gg_out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const double g = grad[e], v = vel[e];
    double ga = gains[e];
    ga = (v * g < 0.0) ? ga + 0.2 : ga * 0.8;
    ga = ga < min_gain ? min_gain : ga;
    const double gg = g * ga;
    const double nv = momentum * v - learning_rate * gg;
    const double ny = Y64[e] + nv;
    gains[e] = ga;
    vel[e] = nv;
    Y64[e] = ny;
    Y32[e] = __double2float_rn(ny);
    if (gg_out) gg_out[e] = gg;
}

extern "C" int scd_tsne_update(scd_handle h, const double* grad, double* Y64, double* vel, double* gains, float* Y32_out, int64_t n, double momentum,
                               double learning_rate, double min_gain, double* gg_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_tsne_update");
    SCD_REQUIRE(grad && Y64 && vel && gains && Y32_out, "scd_tsne_update: null argument");
    SCD_REQUIRE(n >= 1 && n < (1ll << 31), "scd_tsne_update: n = %lld outside [1, 2^31)", (long long)n);
    SCD_REQUIRE(momentum >= 0.0 && momentum < 1.0 && learning_rate > 0.0 && learning_rate < INFINITY && min_gain >= 0.0 && min_gain < INFINITY,
                "scd_tsne_update: momentum in [0, 1), learning_rate > 0 and min_gain >= 0, all finite");
    tsne_update_kernel<<<(unsigned)scd_cdiv(2 * n, 256), 256, 0, (hipStream_t)stream_>>>(grad, Y64, vel, gains, Y32_out, 2 * n, momentum,
                                                                                         learning_rate, min_gain, gg_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
