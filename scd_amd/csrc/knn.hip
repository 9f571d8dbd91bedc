// Exact k nearest neighbours under the inner product on gfx950, and the k-NN vote on top of them (the weighted k-NN protocol of DINO /
// DINOv2: Caron et al., "Emerging Properties in Self-Supervised Vision Transformers", ICCV 2021, section 4.1; k = 20, T = 0.07).
// docs/design/knn.md has the semantics and the derivations.
//
//   scd_knn        for query i the k admissible columns j of X with the largest fn_dot64(Q_i, X_j), ordered by (value descending, column
//                  ascending); column self_base + i is not admissible when self_base >= 0.  A fast pass proposes, float64 decides:
//                    1. fn_prep_kernel (finch_shared.h) for X and, unless Q is X, for Q: fp16 copies HX, HQ (subnormal halfs flushed), per
//                       row e = |row - H row| and h = |H row|, their maxima over X, the flag for a value that does not fit fp16;
//                    2. knn_bound_kernel: the m x n x d pass with v_mfma_f32_16x16x32_f16, FINCH's loop (128-row panels, ranges of 128-column
//                       tiles in grid.y, a two-buffer LDS ring).  Per row and range a lane keeps the largest approximate dot of its residue
//                       class of columns mod 16 (self and the padding columns excluded by index): 16 * ranges kept values per row, each of
//                       another column.  knn_thresh_kernel: t_i = the k-th largest kept value of row i, a lower bound of the k-th largest
//                       approximate dot over all admissible columns; a row that keeps fewer than k columns has no bound;
//                    3. knn_emit_kernel: the same pass again; every admissible column with approximate dot >= t_i - 2 B_i is appended to
//                       row i's KNN_SLOTS slots (an integer atomic counter per row, plain vector stores);
//                    4. knn_refine_kernel, a wave per row: the float64 values of the slot columns, the k best by (value, column).  A row
//                       without a bound, a row whose slots overflowed and - when the flag is set - every row take the exact pass over all
//                       admissible columns instead (info[0]).  The result never depends on the filter.
//                  The bound.  s_ij is the approximate dot (fp32 MFMA accumulation of the fp16 rows), v_ij = Q_i . X_j.  With Q = HQ + RQ and
//                  X = HX + RX,  |v_ij - HQ_i . HX_j| <= e_i (h_j + e_j) + h_i e_j  (Cauchy-Schwarz on RQ_i . HX_j + HQ_i . RX_j + RQ_i . RX_j);
//                  products of two halfs are exact in fp32 and the fp32 accumulation of dp / 32 MFMA steps is charged
//                  2^-22 (dp / 32 + 1) h_i h_j (2^-23 per step relative to the step's sum of magnitudes, doubled).  So
//                    |s_ij - v_ij| <= B_i = e_i (h_max + e_max) + h_i e_max + 2^-22 (dp / 32 + 1) h_i h_max,
//                  e_i, h_i of the query row, the maxima over X, evaluated in float64 and inflated by 1e-3 (which also covers the rounding
//                  of the float64 dot itself).
//                  The certificate.  k admissible columns have s >= t_i, hence v >= t_i - B_i, so the k-th largest value of the row is
//                  >= t_i - B_i.  A column of the answer, or one that ties with its last place, has v >= that, hence s >= t_i - 2 B_i: it is
//                  in the slots.  The threshold is rounded down to fp32 for the comparison in the MFMA epilogue.  The decision is made on
//                  float64 values alone.
//   scd_knn_vote   one thread per query over its k_use neighbours, O(k^2) passes, no per-class table: uniform counts (scikit-learn's
//                  KNeighborsClassifier rule) or exp((dot_j - dot_0) / T) weights (DINO's), the largest score wins, ties to the lowest class
//
// No floating-point atomics: the slot order varies from call to call, the selection by (value, column) does not.
#include "common.h"
#include "finch_shared.h"                       // fn_dot64, fn_vec_ok, fn_prep_kernel
#include "knn_tile.h"                           // the KNN_* shape constants and knn_tile, shared with hdbscan.hip

// the place in this panel of the column a row must not return (row loc of the panel excludes column self_off + loc), or -1
__device__ __forceinline__ int knn_self_loc(long long col, long long self_off) {
    const long long dc = col - self_off;
    return (dc >= 0 && dc < KNN_BM) ? (int)dc : -1;
}

// ------------------------------------------------------------------------------------------------ pass A: per-class maxima
// cand_v [ny, m_alloc, 16]: per range y and row the largest approximate dot of each residue class of admissible columns, or -inf
__global__ void __launch_bounds__(KNN_THREADS) knn_bound_kernel(const half_t* __restrict__ HQ, const half_t* __restrict__ HX, long long n, int ld,
                                                                int dp, long long m_alloc, long long tiles, long long tiles_per_y,
                                                                long long self_base, float* __restrict__ cand_v) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    half_t* sA = reinterpret_cast<half_t*>(knn_lds);            // [2][KNN_BM][KNN_LDK]
    half_t* sB = sA + 2 * KNN_BM * KNN_LDK;                     // [2][KNN_BN][KNN_LDK]
    const long long row0 = (long long)blockIdx.x * KNN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;
    const long long self_off = self_base >= 0 ? self_base + row0 : -(1ll << 40);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float v1[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) v1[mt][r] = -INFINITY;
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const half_t* gA = HQ + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * KNN_LDK + lq * 8, b_frag = lr * KNN_LDK + lq * 8, st_off = lrow * KNN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * KNN_BN;
        f32x4 acc[2][8];
        knn_tile(gA, HX + (size_t)(j0 + lrow) * ld + lk, ld, dp, sA, sB, a_frag, b_frag, st_off, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            const bool valid = col < n;
            const int dcol = knn_self_loc(col, self_off);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int loc = wave * 32 + mt * 16 + lq * 4 + r;
                    const float vv = (valid && dcol != loc) ? acc[mt][nt][r] : -INFINITY;
                    v1[mt][r] = fmaxf(v1[mt][r], vv);
                }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;              // p < m_alloc: the buffers hold the padding rows
            cand_v[((size_t)y * m_alloc + p) * 16 + lr] = v1[mt][r];
        }
}

// ------------------------------------------------------------------------------------------------ the threshold of a row
// A wave per row of m_alloc.  theta[p] = t_p - 2 B_p rounded down to fp32, or +inf: a padding row, a row that kept fewer than k columns,
// every row when a value did not fit fp16.  Also clears the row's candidate counter.
__global__ void __launch_bounds__(256) knn_thresh_kernel(const float* __restrict__ cand_v, long long m, long long m_alloc, int ny, int k, int dp,
                                                         const float* __restrict__ e_q, const float* __restrict__ h_q,
                                                         const unsigned* __restrict__ gq, const unsigned* __restrict__ gx,
                                                         float* __restrict__ theta, int* __restrict__ cnt) {
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= m_alloc) return;
    if (lane == 0) cnt[p] = 0;
    if (p >= m || gq[2] != 0 || gx[2] != 0) {
        if (lane == 0) theta[p] = INFINITY;
        return;
    }
    const int ne = ny * 16;                                     // <= 16 KNN_YMAX = 512 = 8 per lane
    float v[8];
    int kept = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int q = lane + 64 * s;
        v[s] = q < ne ? cand_v[((size_t)(q >> 4) * m_alloc + p) * 16 + (q & 15)] : -INFINITY;
        kept += v[s] > -INFINITY;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
    if (kept < k) {
        if (lane == 0) theta[p] = INFINITY;
        return;
    }
    float t = -INFINITY;
    for (int it = 0; it < k; ++it) {                            // the k-th largest: take the largest away k - 1 times
        float lm = v[0];
#pragma unroll
        for (int s = 1; s < 8; ++s) lm = fmaxf(lm, v[s]);
        t = wave_max_f32(lm);
        if (it == k - 1) break;
        const unsigned long long who = __ballot(lm == t);
        if (lane == __ffsll((long long)who) - 1) {
            bool done = false;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const bool hit = !done && v[s] == t;
                v[s] = hit ? -INFINITY : v[s];
                done = done || hit;
            }
        }
    }
    if (lane == 0) {
        const double hmax = (double)__uint_as_float(gx[0]), emax = (double)__uint_as_float(gx[1]);
        const double ei = (double)e_q[p], hi = (double)h_q[p];
        const double acc_err = 2.384185791015625e-07 * (double)(dp / 32 + 1);             // 2^-22 (dp / 32 + 1)
        const double B = (ei * (hmax + emax) + hi * emax + acc_err * hi * hmax) * 1.001 + 1e-300;
        const double th = (double)t - 2.0 * B;
        theta[p] = (t > -INFINITY && t < INFINITY) ? __double2float_rd(th) : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ pass B: the candidates
__global__ void __launch_bounds__(KNN_THREADS) knn_emit_kernel(const half_t* __restrict__ HQ, const half_t* __restrict__ HX, long long n, int ld,
                                                               int dp, long long tiles, long long tiles_per_y, long long self_base,
                                                               const float* __restrict__ theta, int* __restrict__ cnt,
                                                               int* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
    half_t* sA = reinterpret_cast<half_t*>(knn_lds);
    half_t* sB = sA + 2 * KNN_BM * KNN_LDK;
    const long long row0 = (long long)blockIdx.x * KNN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;
    const long long self_off = self_base >= 0 ? self_base + row0 : -(1ll << 40);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float th[2][4];                                             // +inf for the padding rows: they emit nothing
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) th[mt][r] = theta[row0 + wave * 32 + mt * 16 + lq * 4 + r];
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const half_t* gA = HQ + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * KNN_LDK + lq * 8, b_frag = lr * KNN_LDK + lq * 8, st_off = lrow * KNN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * KNN_BN;
        f32x4 acc[2][8];
        knn_tile(gA, HX + (size_t)(j0 + lrow) * ld + lk, ld, dp, sA, sB, a_frag, b_frag, st_off, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            const bool valid = col < n;
            const int dcol = knn_self_loc(col, self_off);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int loc = wave * 32 + mt * 16 + lq * 4 + r;
                    if (valid && dcol != loc && acc[mt][nt][r] >= th[mt][r]) {
                        const long long p = row0 + loc;
                        const int at = atomicAdd(&cnt[p], 1);
                        if (at < KNN_SLOTS) slots[(size_t)p * KNN_SLOTS + at] = (int)col;
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ refine / exact pass
// The `want` best of the entries q < count with cols[q] >= 0 by (value descending, column ascending) -> tv, tj; returns how many there
// were (<= want).  One wave per block, so __syncthreads orders the wave's LDS traffic.  Taken entries get cols[q] = -1.
__device__ __forceinline__ int knn_select(double* vals, int* cols, int count, int want, double* tv, int* tj, int lane) {
    int got = 0;
    __syncthreads();
    for (int r = 0; r < want; ++r) {
        double bv = -INFINITY;
        int bj = 0x7fffffff, bq = -1;
        for (int q = lane; q < count; q += 64) {
            const int j = cols[q];
            if (j < 0) continue;
            const double v = vals[q];
            if (bq < 0 || v > bv || (v == bv && j < bj)) {
                bv = v;
                bj = j;
                bq = q;
            }
        }
        const int mine = bj;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (oj != 0x7fffffff && (bj == 0x7fffffff || ov > bv || (ov == bv && oj < bj))) {
                bv = ov;
                bj = oj;
            }
        }
        if (bj == 0x7fffffff) break;                            // nothing left (the same in every lane)
        if (bq >= 0 && mine == bj) cols[bq] = -1;               // columns are distinct: one owner
        if (lane == 0) {
            tv[r] = bv;
            tj[r] = bj;
        }
        ++got;
        __syncthreads();
    }
    __syncthreads();
    return got;
}

__global__ void __launch_bounds__(64) knn_refine_kernel(const float* __restrict__ Q, long long m, const float* __restrict__ X, long long n, int d,
                                                        int k, long long self_base, const float* __restrict__ theta,
                                                        const int* __restrict__ cnt, const int* __restrict__ slots,
                                                        const unsigned* __restrict__ gq, const unsigned* __restrict__ gx,
                                                        int* __restrict__ idx_out, double* __restrict__ dot_out, int* __restrict__ info) {
    __shared__ double vals[KNN_SLOTS];
    __shared__ int cols[KNN_SLOTS];
    __shared__ double tv[KNN_KMAX];
    __shared__ int tj[KNN_KMAX];
    const long long i = blockIdx.x;
    const int lane = threadIdx.x;
    const float th = theta[i];
    const int c = cnt[i];
    const bool bounded = th < INFINITY;
    const bool filtered = bounded && c >= k && c <= KNN_SLOTS;
    if (lane == 0) {
        if (!filtered) atomicAdd(&info[0], 1);
        if (bounded && c > KNN_SLOTS) atomicAdd(&info[2], 1);
        atomicMax(&info[3], c);
        if (i == 0 && (gq[2] != 0 || gx[2] != 0)) info[1] = 1;
    }
    const float* qi = Q + (size_t)i * d;
    const bool vec = fn_vec_ok(Q, d) && fn_vec_ok(X, d);
    const long long self = self_base >= 0 ? self_base + i : -1;
    int got;
    if (filtered) {
        for (int q = lane; q < c; q += 64) {
            const int j = slots[(size_t)i * KNN_SLOTS + q];
            cols[q] = j;
            vals[q] = fn_dot64(qi, X + (size_t)j * d, d, vec);
        }
        got = knn_select(vals, cols, c, k, tv, tj, lane);
    } else {                                                    // all admissible columns, KNN_CHUNK at a time behind the best so far
        got = 0;
        for (long long base = 0; base < n; base += KNN_CHUNK) {
            const int span = (int)((n - base < KNN_CHUNK) ? n - base : KNN_CHUNK);
            for (int q = lane; q < span; q += 64) {
                const long long j = base + q;
                const bool ok = j != self;
                cols[got + q] = ok ? (int)j : -1;
                vals[got + q] = ok ? fn_dot64(qi, X + (size_t)j * d, d, vec) : 0.0;
            }
            const int g2 = knn_select(vals, cols, got + span, k, tv, tj, lane);
            for (int q = lane; q < g2; q += 64) {
                vals[q] = tv[q];
                cols[q] = tj[q];
            }
            got = g2;
            __syncthreads();
        }
    }
    for (int q = lane; q < k; q += 64) {
        idx_out[(size_t)i * k + q] = q < got ? tj[q] : -1;
        dot_out[(size_t)i * k + q] = q < got ? tv[q] : NAN;
    }
}

struct knn_plan {
    int ld, dp, ny_max;
    long long n_alloc, m_alloc, xtiles, panels;
    size_t hx, ex, hnx, gx, hq, eq, hnq, gq, cand_v, theta, cnt, slots, end;
};

static void knn_layout(int64_t m, int64_t n, int d, int k, knn_plan& p) {
    p.dp = (int)scd_cdiv(d, 32) * 32;
    p.ld = (int)scd_cdiv(d, KNN_BK) * KNN_BK;
    p.xtiles = scd_cdiv(n, KNN_BN);
    p.n_alloc = p.xtiles * KNN_BN;
    p.panels = scd_cdiv(m, KNN_BM);
    p.m_alloc = p.panels * KNN_BM;
    // ranges: FINCH's fill rule, and at least k / 4 of them so that a row keeps 4 k columns where the data has that many - the k-th
    // largest of 4 k class maxima lies close to the k-th largest dot, and the slots hold what passes it
    long long ny = scd_cdiv(KNN_TARGET_BLOCKS, p.panels);
    if (ny < scd_cdiv(k, 4)) ny = scd_cdiv(k, 4);
    if (ny > KNN_YMAX) ny = KNN_YMAX;
    if (ny > p.xtiles) ny = p.xtiles;
    p.ny_max = (int)ny;
    p.hx = 0;                                                                       // HX     f16   [n_alloc, ld]
    p.ex = p.hx + scd_align((size_t)p.n_alloc * p.ld * 2);                          // e(X)   f32   [n]
    p.hnx = p.ex + scd_align((size_t)n * 4);                                        // h(X)   f32   [n]
    p.gx = p.hnx + scd_align((size_t)n * 4);                                        // gstat  u32   [4] of X
    p.hq = p.gx + scd_align(16);                                                    // HQ     f16   [m_alloc, ld]
    p.eq = p.hq + scd_align((size_t)p.m_alloc * p.ld * 2);                          // e(Q)   f32   [m]
    p.hnq = p.eq + scd_align((size_t)m * 4);                                        // h(Q)   f32   [m]
    p.gq = p.hnq + scd_align((size_t)m * 4);                                        // gstat  u32   [4] of Q
    p.cand_v = p.gq + scd_align(16);                                                // cand_v f32   [ny_max, m_alloc, 16]
    p.theta = p.cand_v + scd_align((size_t)p.ny_max * p.m_alloc * 64);              // theta  f32   [m_alloc]
    p.cnt = p.theta + scd_align((size_t)p.m_alloc * 4);                             // cnt    int32 [m_alloc]
    p.slots = p.cnt + scd_align((size_t)p.m_alloc * 4);                             // slots  int32 [m_alloc, KNN_SLOTS]
    p.end = p.slots + scd_align((size_t)p.m_alloc * KNN_SLOTS * 4);
}

static bool knn_shape_ok(int64_t m, int64_t n, int d, int k) {
    return m >= 1 && m < (1ll << 31) && n >= 2 && n < (1ll << 31) && d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX && k >= 1 && k <= KNN_KMAX;
}

extern "C" int scd_knn_slots(void) { return KNN_SLOTS; }

extern "C" size_t scd_knn_ws_bytes(int64_t m, int64_t n, int d, int k) {
    if (!knn_shape_ok(m, n, d, k)) return 0;
    knn_plan p;
    knn_layout(m, n, d, k, p);
    return p.end;
}

extern "C" int scd_knn(scd_handle h, const float* Q, int64_t m, const float* X, int64_t n, int d, int k, int64_t self_base, int32_t* idx_out,
                       double* dot_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_knn");
    SCD_REQUIRE(Q && X && idx_out && dot_out && info_out && ws, "scd_knn: null argument");
    SCD_REQUIRE(m >= 1 && m < (1ll << 31), "scd_knn: m = %lld outside [1, 2^31)", (long long)m);
    SCD_REQUIRE(n >= 2 && n < (1ll << 31), "scd_knn: n = %lld outside [2, 2^31)", (long long)n);
    SCD_REQUIRE(d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX, "scd_knn: d = %d outside [1, %d]", d, KNN_DP_MAX);
    SCD_REQUIRE(k >= 1 && k <= KNN_KMAX, "scd_knn: k = %d outside [1, %d]", k, KNN_KMAX);
    SCD_REQUIRE(self_base == -1 || (self_base >= 0 && self_base + m <= n), "scd_knn: self_base = %lld: -1, or rows self_base .. self_base + m of X",
                (long long)self_base);
    SCD_REQUIRE(k <= n - (self_base >= 0 ? 1 : 0), "scd_knn: k = %d exceeds the %lld admissible columns", k, (long long)(n - (self_base >= 0 ? 1 : 0)));
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_knn: workspace not 16-byte aligned");
    knn_plan p;
    knn_layout(m, n, d, k, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_knn: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    SCD_REQUIRE(scd_cdiv(p.n_alloc, 4) < (1ll << 31) && scd_cdiv(p.m_alloc, 4) < (1ll << 31), "scd_knn: grid too large");
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    const bool same = Q == X && m == n;                         // the k-NN graph: one preparation serves both sides
    half_t* HX = (half_t*)(w + p.hx);
    unsigned* gx = (unsigned*)(w + p.gx);
    half_t* HQ = same ? HX : (half_t*)(w + p.hq);
    float* eq = (float*)(w + (same ? p.ex : p.eq));
    float* hnq = (float*)(w + (same ? p.hnx : p.hnq));
    unsigned* gq = same ? gx : (unsigned*)(w + p.gq);
    float* cand_v = (float*)(w + p.cand_v);
    float* theta = (float*)(w + p.theta);
    int* cnt = (int*)(w + p.cnt);
    int* slots = (int*)(w + p.slots);

    SCD_HIP(hipMemsetAsync(gx, 0, 16, st));
    SCD_HIP(hipMemsetAsync(info_out, 0, 16, st));
    fn_prep_kernel<<<(unsigned)scd_cdiv(p.n_alloc, 4), 256, 0, st>>>(X, n, d, p.ld, p.n_alloc, HX, (float*)(w + p.ex), (float*)(w + p.hnx), gx);
    if (!same) {
        SCD_HIP(hipMemsetAsync(gq, 0, 16, st));
        fn_prep_kernel<<<(unsigned)scd_cdiv(p.m_alloc, 4), 256, 0, st>>>(Q, m, d, p.ld, p.m_alloc, HQ, eq, hnq, gq);
    }
    SCD_LAUNCH_CHECK();
    // ranges of column tiles (grid.y).  The result does not depend on the choice: it moves rows between the two paths of the refine stage.
    long long ny = scd_cdiv(4ll * h->n_cu, p.panels);
    if (ny < scd_cdiv(k, 4)) ny = scd_cdiv(k, 4);
    if (ny > p.ny_max) ny = p.ny_max;
    if (ny < 1) ny = 1;
    const long long tiles_per_y = scd_cdiv(p.xtiles, ny);
    ny = scd_cdiv(p.xtiles, tiles_per_y);                       // no empty range
    { const int rc_ = scd_set_max_lds((const void*)knn_bound_kernel, KNN_LDS_BYTES); if (rc_) return rc_; }
    { const int rc_ = scd_set_max_lds((const void*)knn_emit_kernel, KNN_LDS_BYTES); if (rc_) return rc_; }
    const dim3 grid((unsigned)p.panels, (unsigned)ny);
    knn_bound_kernel<<<grid, KNN_THREADS, KNN_LDS_BYTES, st>>>(HQ, HX, n, p.ld, p.dp, p.m_alloc, p.xtiles, tiles_per_y, self_base, cand_v);
    knn_thresh_kernel<<<(unsigned)scd_cdiv(p.m_alloc, 4), 256, 0, st>>>(cand_v, m, p.m_alloc, (int)ny, k, p.dp, eq, hnq, gq, gx, theta, cnt);
    knn_emit_kernel<<<grid, KNN_THREADS, KNN_LDS_BYTES, st>>>(HQ, HX, n, p.ld, p.dp, p.xtiles, tiles_per_y, self_base, theta, cnt, slots);
    knn_refine_kernel<<<(unsigned)m, 64, 0, st>>>(Q, m, X, n, d, k, self_base, theta, cnt, slots, gq, gx, idx_out, dot_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ the vote
// idx int32 [m, k_stride], dot float64 [m, k_stride]: the first k_use neighbours of each query vote with their base label.
__global__ void __launch_bounds__(256) knn_vote_kernel(const int* __restrict__ idx, const double* __restrict__ dot, long long m, int k_stride,
                                                       int k_use, const int* __restrict__ labels, long long n, int mode, double temperature,
                                                       int* __restrict__ pred_out, double* __restrict__ score_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int* ri = idx + (size_t)i * k_stride;
    const double* rd = dot + (size_t)i * k_stride;
    const double d0 = rd[0];
    int best_c = -1;
    double best_s = 0.0;
    for (int a = 0; a < k_use; ++a) {
        const long long ja = ri[a];
        const int la = (ja >= 0 && ja < n) ? labels[ja] : -1;
        if (la < 0) continue;
        bool first = true;
        for (int b = 0; b < a; ++b) {
            const long long jb = ri[b];
            if (jb >= 0 && jb < n && labels[jb] == la) first = false;
        }
        if (!first) continue;
        double s = 0.0;
        for (int b = a; b < k_use; ++b) {                       // the class's neighbours in neighbour order
            const long long jb = ri[b];
            if (jb >= 0 && jb < n && labels[jb] == la) s += mode ? exp((rd[b] - d0) / temperature) : 1.0;
        }
        if (best_c < 0 || s > best_s || (s == best_s && la < best_c)) {
            best_s = s;
            best_c = la;
        }
    }
    pred_out[i] = best_c;
    score_out[i] = best_s;
}

extern "C" int scd_knn_vote(scd_handle h, const int32_t* idx, const double* dot, int64_t m, int k_stride, int k_use, const int32_t* base_labels,
                            int64_t n, int mode, double temperature, int32_t* pred_out, double* score_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_knn_vote");
    SCD_REQUIRE(idx && dot && base_labels && pred_out && score_out, "scd_knn_vote: null argument");
    SCD_REQUIRE(m >= 1 && scd_cdiv(m, 256) < (1ll << 31) && n >= 1 && n < (1ll << 31), "scd_knn_vote: bad shape (m = %lld, n = %lld)", (long long)m,
                (long long)n);
    SCD_REQUIRE(k_use >= 1 && k_use <= k_stride, "scd_knn_vote: k_use = %d outside [1, k_stride = %d]", k_use, k_stride);
    SCD_REQUIRE(mode == 0 || mode == 1, "scd_knn_vote: mode %d (0 uniform, 1 softmax)", mode);
    SCD_REQUIRE(mode == 0 || (temperature > 0.0 && temperature < INFINITY), "scd_knn_vote: the temperature must be positive and finite");
    knn_vote_kernel<<<(unsigned)scd_cdiv(m, 256), 256, 0, (hipStream_t)stream_>>>(idx, dot, m, k_stride, k_use, base_labels, n, mode, temperature,
                                                                                  pred_out, score_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
