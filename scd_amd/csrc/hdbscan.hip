// One Boruvka round of the minimum spanning tree of HDBSCAN's mutual-reachability graph on gfx950, without the n x n matrix
// (Campello, Moulavi & Sander, "Density-Based Clustering Based on Hierarchical Density Estimates", PAKDD 2013; scikit-learn 1.7's
// sklearn.cluster.HDBSCAN(metric='euclidean', algorithm='brute') on unit rows).  docs/design/hdbscan.md has the semantics and the derivation.
//
//   scd_mr_nearest  for row i the column j of another component (comp[j] != comp[i]) with the largest mutual-reachability similarity
//                   r_ij = min(c_i, c_j, v_ij), v_ij = fn_dot64(U_i, U_j), c the core dots; ties to the lowest j.  scd_knn's pipeline at
//                   k = 1, square, with the component mask and the clamp by c_j in the MFMA epilogue:
//                     1. fn_prep_kernel (finch_shared.h), unless the caller says the workspace still holds this U's copy; mr_core_kernel:
//                        the core dots rounded down (pass A) and up (pass B) to fp32;
//                     2. mr_bound_kernel: a_ij = min(c_j rounded down, s_ij) on foreign columns, s the approximate dot; per row, range and
//                        lane class the largest; mr_thresh_kernel: g_i = the largest over ranges and classes,
//                        theta_i = min(c_i, g_i - B_i) - B_i rounded down to fp32;
//                     3. mr_emit_kernel: every foreign column with min(c_j rounded up, s_ij) >= theta_i goes to the row's KNN_SLOTS slots;
//                     4. mr_refine_kernel, a wave per row: the float64 r_ij of the slot columns, the best by (r descending, j ascending).
//                        A row without a bound, a row whose slots overflowed and - when a value does not fit fp16 - every row walk all
//                        foreign columns with the same selection instead (info[0]).  The result never depends on the filter.
//                   The certificate.  |s_ij - v_ij| <= B_i (knn.hip).  min is 1-Lipschitz in each argument, and the rounded-down core dot
//                   is <= c_j, so a^A_ij <= min(c_j, v_ij) + B_i: some foreign column has min(c_j, v_ij) >= g_i - B_i, and the row's best
//                   value is r*_i = min(c_i, max_j min(c_j, v_ij)) >= min(c_i, g_i - B_i).  A column that attains r*_i has
//                   min(c_j, v_ij) >= r*_i, hence min(c_j rounded up, s_ij) >= r*_i - B_i >= theta_i: it is in the slots, ties included.
//
// No floating-point atomics: the slot order varies from call to call, the selection by (r, j) does not.
#include "common.h"
#include "finch_shared.h"                       // fn_dot64, fn_vec_ok, fn_prep_kernel
#include "knn_tile.h"                           // the KNN_* shape constants, knn_tile

// ------------------------------------------------------------------------------------------------ the core dots in fp32, both ways
__global__ void __launch_bounds__(256) mr_core_kernel(const double* __restrict__ core, long long n, float* __restrict__ c_dn, float* __restrict__ c_up) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double c = core[j];
    c_dn[j] = __double2float_rd(c);
    c_up[j] = __double2float_ru(c);
}

// ------------------------------------------------------------------------------------------------ pass A: per-class maxima
// cand_v [ny, n_alloc, 16]: per range y and row the largest a_ij of each residue class of foreign columns, or -inf
__global__ void __launch_bounds__(KNN_THREADS) mr_bound_kernel(const half_t* __restrict__ H, long long n, int ld, int dp, long long n_alloc,
                                                               long long tiles, long long tiles_per_y, const int* __restrict__ comp,
                                                               const float* __restrict__ c_dn, float* __restrict__ cand_v) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mr_lds[];
    half_t* sA = reinterpret_cast<half_t*>(mr_lds);             // [2][KNN_BM][KNN_LDK]
    half_t* sB = sA + 2 * KNN_BM * KNN_LDK;                     // [2][KNN_BN][KNN_LDK]
    const long long row0 = (long long)blockIdx.x * KNN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float v1[2][4];
    int rc[2][4];                                               // the rows' components; a padding row's answer is never read
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v1[mt][r] = -INFINITY;
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
            rc[mt][r] = p < n ? comp[p] : 0;
        }
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const half_t* gA = H + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * KNN_LDK + lq * 8, b_frag = lr * KNN_LDK + lq * 8, st_off = lrow * KNN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * KNN_BN;
        int cc[8];
        float cj[8];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            cc[nt] = col < n ? comp[col] : 0;
            cj[nt] = col < n ? c_dn[col] : -INFINITY;           // a padding column never wins
        }
        f32x4 acc[2][8];
        knn_tile(gA, H + (size_t)(j0 + lrow) * ld + lk, ld, dp, sA, sB, a_frag, b_frag, st_off, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const bool valid = j0 + nt * 16 + lr < n;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float vv = (valid && cc[nt] != rc[mt][r]) ? fminf(cj[nt], acc[mt][nt][r]) : -INFINITY;
                    v1[mt][r] = fmaxf(v1[mt][r], vv);
                }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;              // p < n_alloc: the buffers hold the padding rows
            cand_v[((size_t)y * n_alloc + p) * 16 + lr] = v1[mt][r];
        }
}

// ------------------------------------------------------------------------------------------------ the threshold of a row
// A wave per row of n_alloc.  theta[p] = min(c_p, g_p - B_p) - B_p rounded down to fp32, or +inf: a padding row, a row without a foreign
// column, every row when a value did not fit fp16.  Also clears the row's candidate counter.
__global__ void __launch_bounds__(256) mr_thresh_kernel(const float* __restrict__ cand_v, long long n, long long n_alloc, int ny, int dp,
                                                        const float* __restrict__ e_r, const float* __restrict__ h_r,
                                                        const unsigned* __restrict__ gx, const double* __restrict__ core,
                                                        float* __restrict__ theta, int* __restrict__ cnt) {
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= n_alloc) return;
    if (lane == 0) cnt[p] = 0;
    if (p >= n || gx[2] != 0) {
        if (lane == 0) theta[p] = INFINITY;
        return;
    }
    const int ne = ny * 16;                                     // <= 16 KNN_YMAX = 512 = 8 per lane
    float g = -INFINITY;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int q = lane + 64 * s;
        if (q < ne) g = fmaxf(g, cand_v[((size_t)(q >> 4) * n_alloc + p) * 16 + (q & 15)]);
    }
    g = wave_max_f32(g);
    if (lane == 0) {
        const double hmax = (double)__uint_as_float(gx[0]), emax = (double)__uint_as_float(gx[1]);
        const double ei = (double)e_r[p], hi = (double)h_r[p];
        const double acc_err = 2.384185791015625e-07 * (double)(dp / 32 + 1);             // 2^-22 (dp / 32 + 1)
        const double B = (ei * (hmax + emax) + hi * emax + acc_err * hi * hmax) * 1.001 + 1e-300;
        const double th = fmin(core[p], (double)g - B) - B;
        theta[p] = (g > -INFINITY && g < INFINITY) ? __double2float_rd(th) : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ pass B: the candidates
__global__ void __launch_bounds__(KNN_THREADS) mr_emit_kernel(const half_t* __restrict__ H, long long n, int ld, int dp, long long tiles,
                                                              long long tiles_per_y, const int* __restrict__ comp,
                                                              const float* __restrict__ c_up, const float* __restrict__ theta,
                                                              int* __restrict__ cnt, int* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mr_lds[];
    half_t* sA = reinterpret_cast<half_t*>(mr_lds);
    half_t* sB = sA + 2 * KNN_BM * KNN_LDK;
    const long long row0 = (long long)blockIdx.x * KNN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float th[2][4];                                             // +inf for the padding rows: they emit nothing
    int rc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
            th[mt][r] = theta[p];
            rc[mt][r] = p < n ? comp[p] : 0;
        }
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const half_t* gA = H + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * KNN_LDK + lq * 8, b_frag = lr * KNN_LDK + lq * 8, st_off = lrow * KNN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * KNN_BN;
        int cc[8];
        float cj[8];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            cc[nt] = col < n ? comp[col] : 0;
            cj[nt] = col < n ? c_up[col] : -INFINITY;
        }
        f32x4 acc[2][8];
        knn_tile(gA, H + (size_t)(j0 + lrow) * ld + lk, ld, dp, sA, sB, a_frag, b_frag, st_off, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            const bool valid = col < n;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
                    if (valid && p < n && cc[nt] != rc[mt][r] && fminf(cj[nt], acc[mt][nt][r]) >= th[mt][r]) {
                        const int at = atomicAdd(&cnt[p], 1);
                        if (at < KNN_SLOTS) slots[(size_t)p * KNN_SLOTS + at] = (int)col;
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ refine / exact walk
// (r, j) of this lane against another: larger r wins, then the lower column; j < 0 is "none"
__device__ __forceinline__ void mr_better(double& bv, int& bj, double v, int j) {
    if (j >= 0 && (bj < 0 || v > bv || (v == bv && j < bj))) {
        bv = v;
        bj = j;
    }
}

__global__ void __launch_bounds__(64) mr_refine_kernel(const float* __restrict__ U, long long n, int d, const double* __restrict__ core,
                                                       const int* __restrict__ comp, const float* __restrict__ theta,
                                                       const int* __restrict__ cnt, const int* __restrict__ slots,
                                                       const unsigned* __restrict__ gx, int* __restrict__ nn_out, double* __restrict__ r_out,
                                                       int* __restrict__ info) {
    const long long i = blockIdx.x;
    const int lane = threadIdx.x;
    const float th = theta[i];
    const int c = cnt[i];
    const bool bounded = th < INFINITY;
    const bool filtered = bounded && c >= 1 && c <= KNN_SLOTS;
    if (lane == 0) {
        if (!filtered) atomicAdd(&info[0], 1);
        if (bounded && c > KNN_SLOTS) atomicAdd(&info[2], 1);
        atomicMax(&info[3], c);
        if (i == 0 && gx[2] != 0) info[1] = 1;
    }
    const float* ui = U + (size_t)i * d;
    const bool vec = fn_vec_ok(U, d);
    const double ci = core[i];
    const int mine = comp[i];
    double bv = -INFINITY;
    int bj = -1;
    if (filtered) {
        for (int q = lane; q < c; q += 64) {
            const int j = slots[(size_t)i * KNN_SLOTS + q];
            const double v = fn_dot64(ui, U + (size_t)j * d, d, vec);
            mr_better(bv, bj, fmin(fmin(ci, core[j]), v), j);
        }
    } else {                                                    // all foreign columns
        for (long long j = lane; j < n; j += 64) {
            if (comp[j] == mine) continue;
            const double v = fn_dot64(ui, U + (size_t)j * d, d, vec);
            mr_better(bv, bj, fmin(fmin(ci, core[j]), v), (int)j);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        mr_better(bv, bj, ov, oj);
    }
    if (lane == 0) {
        nn_out[i] = bj;
        r_out[i] = bj >= 0 ? bv : -INFINITY;
    }
}

struct mr_plan {
    int ld, dp, ny_max;
    long long n_alloc, tiles;
    size_t hx, ex, hnx, gx, c_dn, c_up, cand_v, theta, cnt, slots, end;
};

static void mr_layout(int64_t n, int d, mr_plan& p) {
    p.dp = (int)scd_cdiv(d, 32) * 32;
    p.ld = (int)scd_cdiv(d, KNN_BK) * KNN_BK;
    p.tiles = scd_cdiv(n, KNN_BN);
    p.n_alloc = p.tiles * KNN_BN;
    long long ny = scd_cdiv(KNN_TARGET_BLOCKS, p.tiles);        // FINCH's fill rule; the panels are the tiles (square)
    if (ny > KNN_YMAX) ny = KNN_YMAX;
    if (ny > p.tiles) ny = p.tiles;
    p.ny_max = (int)ny;
    p.hx = 0;                                                                       // H      f16   [n_alloc, ld]     kept between calls
    p.ex = p.hx + scd_align((size_t)p.n_alloc * p.ld * 2);                          // e      f32   [n]               kept
    p.hnx = p.ex + scd_align((size_t)n * 4);                                        // h      f32   [n]               kept
    p.gx = p.hnx + scd_align((size_t)n * 4);                                        // gstat  u32   [4]               kept
    p.c_dn = p.gx + scd_align(16);                                                  // c_dn   f32   [n]
    p.c_up = p.c_dn + scd_align((size_t)n * 4);                                     // c_up   f32   [n]
    p.cand_v = p.c_up + scd_align((size_t)n * 4);                                   // cand_v f32   [ny_max, n_alloc, 16]
    p.theta = p.cand_v + scd_align((size_t)p.ny_max * p.n_alloc * 64);              // theta  f32   [n_alloc]
    p.cnt = p.theta + scd_align((size_t)p.n_alloc * 4);                             // cnt    int32 [n_alloc]
    p.slots = p.cnt + scd_align((size_t)p.n_alloc * 4);                             // slots  int32 [n_alloc, KNN_SLOTS]
    p.end = p.slots + scd_align((size_t)p.n_alloc * KNN_SLOTS * 4);
}

static bool mr_shape_ok(int64_t n, int d) { return n >= 2 && n < (1ll << 31) && d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX; }

extern "C" size_t scd_mr_nearest_ws_bytes(int64_t n, int d) {
    if (!mr_shape_ok(n, d)) return 0;
    mr_plan p;
    mr_layout(n, d, p);
    return p.end;
}

extern "C" int scd_mr_nearest(scd_handle h, const float* U, int64_t n, int d, const double* core, const int32_t* comp, int prepared,
                              int32_t* nn_out, double* r_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_mr_nearest");
    SCD_REQUIRE(U && core && comp && nn_out && r_out && info_out && ws, "scd_mr_nearest: null argument");
    SCD_REQUIRE(n >= 2 && n < (1ll << 31), "scd_mr_nearest: n = %lld outside [2, 2^31)", (long long)n);
    SCD_REQUIRE(d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX, "scd_mr_nearest: d = %d outside [1, %d]", d, KNN_DP_MAX);
    SCD_REQUIRE(prepared == 0 || prepared == 1, "scd_mr_nearest: prepared = %d (0: prepare the workspace, 1: it holds this U's copy)", prepared);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_mr_nearest: workspace not 16-byte aligned");
    mr_plan p;
    mr_layout(n, d, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_mr_nearest: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    SCD_REQUIRE(scd_cdiv(p.n_alloc, 4) < (1ll << 31), "scd_mr_nearest: grid too large");
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    half_t* H = (half_t*)(w + p.hx);
    float* er = (float*)(w + p.ex);
    float* hr = (float*)(w + p.hnx);
    unsigned* gx = (unsigned*)(w + p.gx);
    float* c_dn = (float*)(w + p.c_dn);
    float* c_up = (float*)(w + p.c_up);
    float* cand_v = (float*)(w + p.cand_v);
    float* theta = (float*)(w + p.theta);
    int* cnt = (int*)(w + p.cnt);
    int* slots = (int*)(w + p.slots);

    SCD_HIP(hipMemsetAsync(info_out, 0, 16, st));
    if (!prepared) {
        SCD_HIP(hipMemsetAsync(gx, 0, 16, st));
        fn_prep_kernel<<<(unsigned)scd_cdiv(p.n_alloc, 4), 256, 0, st>>>(U, n, d, p.ld, p.n_alloc, H, er, hr, gx);
    }
    mr_core_kernel<<<(unsigned)scd_cdiv(n, 256), 256, 0, st>>>(core, n, c_dn, c_up);
    SCD_LAUNCH_CHECK();
    // ranges of column tiles (grid.y).  The result does not depend on the choice, and at k = 1 neither does the candidate count.
    long long ny = scd_cdiv(4ll * h->n_cu, p.tiles);
    if (ny > p.ny_max) ny = p.ny_max;
    if (ny < 1) ny = 1;
    const long long tiles_per_y = scd_cdiv(p.tiles, ny);
    ny = scd_cdiv(p.tiles, tiles_per_y);                        // no empty range
    { const int rc_ = scd_set_max_lds((const void*)mr_bound_kernel, KNN_LDS_BYTES); if (rc_) return rc_; }
    { const int rc_ = scd_set_max_lds((const void*)mr_emit_kernel, KNN_LDS_BYTES); if (rc_) return rc_; }
    const dim3 grid((unsigned)p.tiles, (unsigned)ny);
    mr_bound_kernel<<<grid, KNN_THREADS, KNN_LDS_BYTES, st>>>(H, n, p.ld, p.dp, p.n_alloc, p.tiles, tiles_per_y, comp, c_dn, cand_v);
    mr_thresh_kernel<<<(unsigned)scd_cdiv(p.n_alloc, 4), 256, 0, st>>>(cand_v, n, p.n_alloc, (int)ny, p.dp, er, hr, gx, core, theta, cnt);
    mr_emit_kernel<<<grid, KNN_THREADS, KNN_LDS_BYTES, st>>>(H, n, p.ld, p.dp, p.tiles, tiles_per_y, comp, c_up, theta, cnt, slots);
    mr_refine_kernel<<<(unsigned)n, 64, 0, st>>>(U, n, d, core, comp, theta, cnt, slots, gx, nn_out, r_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
