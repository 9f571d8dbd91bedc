// Ward agglomerative clustering on gfx950 without the n x n matrix: the nearest-neighbour search of one round of the reciprocal-pair
// procedure and the merge of a round's pairs (Ward, "Hierarchical Grouping to Optimize an Objective Function", JASA 1963; Murtagh,
// "A Survey of Recent Advances in Hierarchical Clustering Algorithms", 1983, for reducibility and reciprocal nearest neighbours; the
// result is scipy's linkage(x, 'ward')).  docs/design/ward.md has the procedure, the derivation of the bound and the measurements.
//
//   scd_ward_nearest  the table is X float32 [m, d] with sizes xcnt int32 [m]; a position of size 0 is dead.  For query p (row Q_p, size
//                     qcnt[p], its own column qself[p] or -1) the live column j != qself[p] of the least
//                       cost_pj = w * D,  D = max(0, (q_p + q_j) - 2 v_pj),  w = ((double)a * (double)b) / (double)(a + b),
//                     q = fn_dot64 of a row with itself, v = fn_dot64(Q_p, X_j), a = qcnt[p], b = xcnt[j], every operation in float64 and
//                     rounded once ((q_p + q_j) - 2 v may contract to an fma: 2 v is exact, the bits are the same); ties to the lowest j.
//                     scd_knn's rectangular shape with scd_mr_nearest's k = 1 pipeline:
//                       1. ward_prep_kernel: the fp16 copy, e, h (finch_shared.h's terms), the fp16 flag and q of the positions of X from
//                          `prepared` on, and of Q; ward_cols_kernel: the maxima of e and h over the LIVE positions, per column q_j and
//                          1 / b rounded to fp32 (-1 on a dead or padding column); ward_rows_kernel: per query q_p, 1 / a and c_p = 2 B_p
//                          rounded up, B_p scd_knn's bound on |s_pj - v_pj|;
//                       2. ward_bound_kernel: U_pj, an fp32 upper bound of cost_pj, from the approximate dot s_pj; per query, range and lane
//                          class the least; ward_thresh_kernel: theta_p = the least over ranges and classes;
//                       3. ward_emit_kernel: every live foreign column whose lower bound L_pj <= theta_p goes to the query's KNN_SLOTS slots
//                          (an integer atomic counter, plain stores);
//                       4. ward_refine_kernel, a wave per query: the float64 cost of the slot columns, the best by (cost, j).  A query
//                          without a bound, one whose slots overflowed and - with the fp16 flag - every query walk all live columns with
//                          the same selection (info[0]).  The result never depends on the filter.
//                     The bound.  T = fl(q_p + q_j) on the fp32 norms, Dh = fma(-2, s, T), sl = fma(T, 2^-19, c_p).  E = q_p + q_j - 2 v
//                     differs from Dh by at most 2 B_p <= c_p / 1.001 (the dot), 2^-24 (q_p + q_j) (the fp32 norms), 2^-24 T (the sum),
//                     2^-24 |Dh| <= 2.01 2^-24 T (the fma; 2 |s| <= 1.01 T by Cauchy-Schwarz) and the roundings of sl and of Dh +- sl,
//                     2^-24 (|Dh| + 2 sl): under 0.2 * 2^-19 T + 2^-22 c_p beyond 2 B_p.  So max(0, Dh - sl) <= D <= max(0, Dh + sl), the
//                     float64 roundings of D (2^-52) included.  wh = 1 / (fl(1 / a) + fl(1 / b)) in fp32 is w (1 + t), |t| <= 3.1 2^-24, and
//                     two fp32 products add 2^-23: U = wh max(0, Dh + sl) (1 + 2^-18) >= cost, and a column with cost <= theta has
//                     max(0, Dh - sl) (1 - 2^-18) <= (theta + 1e-25) (fl(1 / a) + fl(1 / b)), the test of pass B (division-free; 1e-25
//                     keeps the right side a normal number and covers a product that went subnormal).
//                     The certificate.  theta_p = U_pj' >= cost_pj' >= the least cost c*.  A column that attains c* has cost <= theta_p and
//                     passes the test of pass B: it is in the slots, ties included.
//   scd_ward_merge    for every pair (lo, hi), lo < hi, of a round: X_lo <- fl32(((double)a X_lo + (double)b X_hi) / (double)(a + b)) per
//                     coordinate (the products are exact below 2^29 rows, 29 + 24 bits, so contracting them into an fma changes no bit),
//                     xcnt[lo] = a + b, xcnt[hi] = 0, and the prepared data of position lo made again by the code of ward_prep_kernel.
//
// No floating-point atomics: the slot order varies from call to call, the selection by (cost, j) does not.
#include "common.h"
#include "finch_shared.h"                       // fn_dot64, fn_vec_ok
#include "knn_tile.h"                           // the KNN_* shape constants, knn_tile

#define WARD_T_SLACK 1.9073486328125e-06f       // 2^-19
#define WARD_K_UP 1.000003814697265625f         // 1 + 2^-18
#define WARD_K_DN 0.999996185302734375f         // 1 - 2^-18
#define WARD_TH_ABS 1e-25f
#define WARD_NMAX (1ll << 29)

// ------------------------------------------------------------------------------------------------ prep of one row, a wave
// fn_prep_kernel's row (finch_shared.h) with the flag kept per row, and q = fn_dot64(row, row) by lane 0
__device__ __forceinline__ void ward_prep_row(const float* __restrict__ src, int d, int ld, bool vec, half_t* __restrict__ dst,
                                              float* __restrict__ e_out, float* __restrict__ h_out, int* __restrict__ bad_out,
                                              double* __restrict__ qn_out, int lane) {
    double e2 = 0.0, h2 = 0.0;
    int bad = 0;
    for (int c = lane; c < ld; c += 64) {
        half_t hv = (half_t)0.f;
        if (c < d) {
            const float x = src[c];
            hv = (half_t)x;
            float hf = (float)hv;
            if (!(fabsf(hf) <= 65504.f)) {                      // infinity or NaN
                bad = 1;
                hv = (half_t)0.f;
                hf = 0.f;
            } else if (fabsf(hf) < 6.103515625e-05f) {          // a subnormal half: flushed, the bound carries it in e
                hv = (half_t)0.f;
                hf = 0.f;
            }
            const double r = (double)x - (double)hf;
            e2 = fma(r, r, e2);
            h2 = fma((double)hf, (double)hf, h2);
        }
        dst[c] = hv;
    }
    e2 = wave_sum_f64(e2);
    h2 = wave_sum_f64(h2);
    bad = __any(bad);
    if (lane == 0) {
        const float ef = (float)(sqrt(e2) * 1.000001), hf = (float)(sqrt(h2) * 1.000001);
        *e_out = ef;
        *h_out = hf;
        *bad_out = (bad || !(ef == ef) || !(hf == hf)) ? 1 : 0;
        *qn_out = fn_dot64(src, src, d, vec);
    }
}

// rows first .. n_alloc - 1 of the buffers; a row >= n is padding: zeros, never live
__global__ void __launch_bounds__(256) ward_prep_kernel(const float* __restrict__ X, long long first, long long n, int d, int ld, long long n_alloc,
                                                        half_t* __restrict__ H, float* __restrict__ e_out, float* __restrict__ h_out,
                                                        int* __restrict__ bad_out, double* __restrict__ qn_out) {
    const long long row = first + (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_alloc) return;
    if (row >= n) {
        half_t* dst = H + (size_t)row * ld;
        for (int c = lane; c < ld; c += 64) dst[c] = (half_t)0.f;
        if (lane == 0) {
            e_out[row] = 0.f;
            h_out[row] = 0.f;
            bad_out[row] = 0;
            qn_out[row] = 0.0;
        }
        return;
    }
    ward_prep_row(X + (size_t)row * d, d, ld, fn_vec_ok(X, d), H + (size_t)row * ld, e_out + row, h_out + row, bad_out + row, qn_out + row, lane);
}

// ------------------------------------------------------------------------------------------------ per column, per query
// gstat: [0] bits of max h, [1] bits of max e over the live positions, [2] a live position with the flag
__global__ void __launch_bounds__(256) ward_cols_kernel(const int* __restrict__ xcnt, long long m, long long m_alloc, const float* __restrict__ e_x,
                                                        const float* __restrict__ h_x, const int* __restrict__ bad_x,
                                                        const double* __restrict__ qn_x, float* __restrict__ qf_x, float* __restrict__ rb_x,
                                                        unsigned* __restrict__ gstat) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    float e = 0.f, h = 0.f;
    int bad = 0;
    if (j < m_alloc) {
        const int b = j < m ? xcnt[j] : 0;
        qf_x[j] = (float)qn_x[j];
        rb_x[j] = b > 0 ? (float)(1.0 / (double)b) : -1.f;
        if (b > 0) {
            e = e_x[j];
            h = h_x[j];
            bad = bad_x[j];
        }
    }
    e = wave_max_f32(e);
    h = wave_max_f32(h);
    bad = __any(bad);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&gstat[1], __float_as_uint(e));
        atomicMax(&gstat[0], __float_as_uint(h));
        if (bad) atomicOr(&gstat[2], 1u);
    }
}

// per query of q_alloc: the fp32 norm, 1 / size, c = 2 B rounded up (0 on a padding row), the flag of Q into gstat[3]; clears the counter
__global__ void __launch_bounds__(256) ward_rows_kernel(const int* __restrict__ qcnt, long long q, long long q_alloc, int dp,
                                                        const float* __restrict__ e_q, const float* __restrict__ h_q, const int* __restrict__ bad_q,
                                                        const double* __restrict__ qn_q, unsigned* __restrict__ gstat, float* __restrict__ qf_q,
                                                        float* __restrict__ ra_q, float* __restrict__ c_q, int* __restrict__ cnt) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= q_alloc) return;
    cnt[p] = 0;
    if (p >= q) {
        qf_q[p] = 0.f;
        ra_q[p] = 1.f;
        c_q[p] = 0.f;
        return;
    }
    const double hmax = (double)__uint_as_float(gstat[0]), emax = (double)__uint_as_float(gstat[1]);
    const double ei = (double)e_q[p], hi = (double)h_q[p];
    const double acc_err = 2.384185791015625e-07 * (double)(dp / 32 + 1);                 // 2^-22 (dp / 32 + 1)
    const double B = (ei * (hmax + emax) + hi * emax + acc_err * hi * hmax) * 1.001 + 1e-300;
    qf_q[p] = (float)qn_q[p];
    const int a = qcnt[p];
    ra_q[p] = (float)(1.0 / (double)(a > 0 ? a : 1));
    c_q[p] = __double2float_ru(2.0 * B);
    if (bad_q[p]) atomicOr(&gstat[3], 1u);
}

// ------------------------------------------------------------------------------------------------ pass A: per-class minima of U
// cand_v [ny, q_alloc, 16]: per range y and query the least U_pj of each residue class of live foreign columns, or +inf
__global__ void __launch_bounds__(KNN_THREADS) ward_bound_kernel(const half_t* __restrict__ HQ, const half_t* __restrict__ HX, int ld, int dp,
                                                                 long long q_alloc, long long tiles, long long tiles_per_y,
                                                                 const float* __restrict__ qf_q, const float* __restrict__ ra_q,
                                                                 const float* __restrict__ c_q, const int* __restrict__ qself, long long q,
                                                                 const float* __restrict__ qf_x, const float* __restrict__ rb_x,
                                                                 float* __restrict__ cand_v) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ward_lds[];
    half_t* sA = reinterpret_cast<half_t*>(ward_lds);           // [2][KNN_BM][KNN_LDK]
    half_t* sB = sA + 2 * KNN_BM * KNN_LDK;                     // [2][KNN_BN][KNN_LDK]
    const long long row0 = (long long)blockIdx.x * KNN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float v1[2][4], qi[2][4], ra[2][4], ci[2][4];
    int self[2][4];                                             // a padding row's answer is never read
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
            v1[mt][r] = INFINITY;
            qi[mt][r] = qf_q[p];
            ra[mt][r] = ra_q[p];
            ci[mt][r] = c_q[p];
            self[mt][r] = p < q ? qself[p] : -1;
        }
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const half_t* gA = HQ + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * KNN_LDK + lq * 8, b_frag = lr * KNN_LDK + lq * 8, st_off = lrow * KNN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * KNN_BN;
        float qj[8], rb[8];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;            // < m_alloc: the column arrays hold the padding
            qj[nt] = qf_x[col];
            rb[nt] = rb_x[col];
        }
        f32x4 acc[2][8];
        knn_tile(gA, HX + (size_t)(j0 + lrow) * ld + lk, ld, dp, sA, sB, a_frag, b_frag, st_off, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int col = (int)(j0 + nt * 16 + lr);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float T = qi[mt][r] + qj[nt];
                    const float Dh = fmaf(-2.f, acc[mt][nt][r], T);
                    const float sl = fmaf(T, WARD_T_SLACK, ci[mt][r]);
                    const float Du = fmaxf(Dh + sl, 0.f);
                    const float wh = 1.f / (ra[mt][r] + rb[nt]);
                    const float U = (wh * Du) * WARD_K_UP;
                    const float vv = (rb[nt] > 0.f && col != self[mt][r]) ? U : INFINITY;
                    v1[mt][r] = fminf(v1[mt][r], vv);
                }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;              // p < q_alloc: the buffers hold the padding rows
            cand_v[((size_t)y * q_alloc + p) * 16 + lr] = v1[mt][r];
        }
}

// ------------------------------------------------------------------------------------------------ the threshold of a query
// A wave per row of q_alloc.  theta[p] = the least kept U, or +inf: a padding row, a query without a live foreign column, every query
// when a value did not fit fp16.
__global__ void __launch_bounds__(256) ward_thresh_kernel(const float* __restrict__ cand_v, long long q, long long q_alloc, int ny,
                                                          const unsigned* __restrict__ gstat, float* __restrict__ theta) {
    const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= q_alloc) return;
    if (p >= q || gstat[2] != 0 || gstat[3] != 0) {
        if (lane == 0) theta[p] = INFINITY;
        return;
    }
    const int ne = ny * 16;                                     // <= 16 KNN_YMAX = 512 = 8 per lane
    float g = INFINITY;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = lane + 64 * s;
        if (k < ne) g = fminf(g, cand_v[((size_t)(k >> 4) * q_alloc + p) * 16 + (k & 15)]);
    }
    g = -wave_max_f32(-g);
    if (lane == 0) theta[p] = (g >= 0.f && g < INFINITY) ? g : INFINITY;
}

// ------------------------------------------------------------------------------------------------ pass B: the candidates
__global__ void __launch_bounds__(KNN_THREADS) ward_emit_kernel(const half_t* __restrict__ HQ, const half_t* __restrict__ HX, int ld, int dp,
                                                                long long tiles, long long tiles_per_y, const float* __restrict__ qf_q,
                                                                const float* __restrict__ ra_q, const float* __restrict__ c_q,
                                                                const int* __restrict__ qself, long long q, const float* __restrict__ qf_x,
                                                                const float* __restrict__ rb_x, const float* __restrict__ theta,
                                                                int* __restrict__ cnt, int* __restrict__ slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ward_lds[];
    half_t* sA = reinterpret_cast<half_t*>(ward_lds);
    half_t* sB = sA + 2 * KNN_BM * KNN_LDK;
    const long long row0 = (long long)blockIdx.x * KNN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float th[2][4], qi[2][4], ra[2][4], ci[2][4];               // th < 0 for a query without a bound and the padding rows: they emit nothing
    int self[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
            const float t = theta[p];
            th[mt][r] = (p < q && t < INFINITY) ? t + WARD_TH_ABS : -1.f;
            qi[mt][r] = qf_q[p];
            ra[mt][r] = ra_q[p];
            ci[mt][r] = c_q[p];
            self[mt][r] = p < q ? qself[p] : -1;
        }
    const int lrow = tid >> 3, lk = (tid & 7) * 8;
    const half_t* gA = HQ + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * KNN_LDK + lq * 8, b_frag = lr * KNN_LDK + lq * 8, st_off = lrow * KNN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * KNN_BN;
        float qj[8], rb[8];
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            qj[nt] = qf_x[col];
            rb[nt] = rb_x[col];
        }
        f32x4 acc[2][8];
        knn_tile(gA, HX + (size_t)(j0 + lrow) * ld + lk, ld, dp, sA, sB, a_frag, b_frag, st_off, acc);
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int col = (int)(j0 + nt * 16 + lr);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float T = qi[mt][r] + qj[nt];
                    const float Dh = fmaf(-2.f, acc[mt][nt][r], T);
                    const float sl = fmaf(T, WARD_T_SLACK, ci[mt][r]);
                    const float Dl = fmaxf(Dh - sl, 0.f);
                    const float rs = ra[mt][r] + rb[nt];
                    if (rb[nt] > 0.f && col != self[mt][r] && Dl * WARD_K_DN <= th[mt][r] * rs) {
                        const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
                        const int at = atomicAdd(&cnt[p], 1);
                        if (at < KNN_SLOTS) slots[(size_t)p * KNN_SLOTS + at] = col;
                    }
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ refine / exact walk
// (cost, j) of this lane against another: the smaller cost wins, then the lower column; j < 0 is "none"
__device__ __forceinline__ void ward_better(double& bv, int& bj, double v, int j) {
    if (j >= 0 && (bj < 0 || v < bv || (v == bv && j < bj))) {
        bv = v;
        bj = j;
    }
}

// the pair value of the contract: every operation rounded once; 2 v is exact, so (qi + qj) - 2 v is the same bits as an fma
__device__ __forceinline__ double ward_cost64(double qi, double qj, double v, int a, int b) {
    const double D = fmax(0.0, (qi + qj) - 2.0 * v);
    const double w = ((double)a * (double)b) / (double)(a + b);
    return w * D;
}

__global__ void __launch_bounds__(64) ward_refine_kernel(const float* __restrict__ Q, const int* __restrict__ qcnt, const int* __restrict__ qself,
                                                         const double* __restrict__ qn_q, const float* __restrict__ X,
                                                         const int* __restrict__ xcnt, const double* __restrict__ qn_x, long long m, int d,
                                                         const float* __restrict__ theta, const int* __restrict__ cnt,
                                                         const int* __restrict__ slots, const unsigned* __restrict__ gstat,
                                                         int* __restrict__ nn_out, double* __restrict__ cost_out, int* __restrict__ info) {
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
        if (i == 0 && (gstat[2] != 0 || gstat[3] != 0)) info[1] = 1;
    }
    const float* qi = Q + (size_t)i * d;
    const bool vec = fn_vec_ok(Q, d) && fn_vec_ok(X, d);
    const double qq = qn_q[i];
    const int a = qcnt[i], self = qself[i];
    double bv = INFINITY;
    int bj = -1;
    if (filtered) {
        for (int s = lane; s < c; s += 64) {
            const int j = slots[(size_t)i * KNN_SLOTS + s];
            const double v = fn_dot64(qi, X + (size_t)j * d, d, vec);
            ward_better(bv, bj, ward_cost64(qq, qn_x[j], v, a, xcnt[j]), j);
        }
    } else {                                                    // all live foreign columns
        for (long long j = lane; j < m; j += 64) {
            const int b = xcnt[j];
            if (b <= 0 || j == self) continue;
            const double v = fn_dot64(qi, X + (size_t)j * d, d, vec);
            ward_better(bv, bj, ward_cost64(qq, qn_x[j], v, a, b), (int)j);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        ward_better(bv, bj, ov, oj);
    }
    if (lane == 0) {
        nn_out[i] = bj;
        cost_out[i] = bj >= 0 ? bv : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ the merge of a round's pairs
// A wave per pair.  A pair that is not 0 <= lo < hi < m with both positions live is left alone.
__global__ void __launch_bounds__(64) ward_merge_kernel(float* __restrict__ X, int* __restrict__ xcnt, const int* __restrict__ lo_,
                                                        const int* __restrict__ hi_, long long m, int d, int ld, half_t* __restrict__ H,
                                                        float* __restrict__ e_x, float* __restrict__ h_x, int* __restrict__ bad_x,
                                                        double* __restrict__ qn_x) {
    const int lane = threadIdx.x;
    const long long lo = lo_[blockIdx.x], hi = hi_[blockIdx.x];
    if (!(lo >= 0 && lo < hi && hi < m)) return;
    const int a = xcnt[lo], b = xcnt[hi];
    if (a <= 0 || b <= 0) return;
    float* xa = X + (size_t)lo * d;
    const float* xb = X + (size_t)hi * d;
    const double fa = (double)a, fb = (double)b, fs = (double)(a + b);
    // fa * xa and fb * xb are exact (29 + 24 bits): contracting them into an fma changes no bit
    for (int c = lane; c < d; c += 64) xa[c] = (float)((fa * (double)xa[c] + fb * (double)xb[c]) / fs);
    __threadfence_block();
    __syncthreads();                                            // lane 0 reads the whole new row below
    ward_prep_row(xa, d, ld, fn_vec_ok(X, d), H + (size_t)lo * ld, e_x + lo, h_x + lo, bad_x + lo, qn_x + lo, lane);
    if (lane == 0) {
        xcnt[lo] = a + b;
        xcnt[hi] = 0;
    }
}

struct ward_plan {
    int ld, dp, ny_max;
    long long m_alloc, q_alloc, xtiles, panels;
    size_t hx, ex, hnx, badx, qnx, xend;                        // the table's part: kept between calls, a function of m and d alone
    size_t gs, qfx, rbx, hq, eq, hnq, badq, qnq, qfq, raq, cq, cand_v, theta, cnt, slots, end;
};

static void ward_layout(int64_t q, int64_t m, int d, ward_plan& p) {
    p.dp = (int)scd_cdiv(d, 32) * 32;
    p.ld = (int)scd_cdiv(d, KNN_BK) * KNN_BK;
    p.xtiles = scd_cdiv(m, KNN_BN);
    p.m_alloc = p.xtiles * KNN_BN;
    p.panels = scd_cdiv(q, KNN_BM);
    p.q_alloc = p.panels * KNN_BM;
    long long ny = scd_cdiv(KNN_TARGET_BLOCKS, p.panels);       // FINCH's fill rule
    if (ny > KNN_YMAX) ny = KNN_YMAX;
    if (ny > p.xtiles) ny = p.xtiles;
    p.ny_max = (int)ny;
    p.hx = 0;                                                                       // HX     f16   [m_alloc, ld]     kept
    p.ex = p.hx + scd_align((size_t)p.m_alloc * p.ld * 2);                          // e(X)   f32   [m_alloc]         kept
    p.hnx = p.ex + scd_align((size_t)p.m_alloc * 4);                                // h(X)   f32   [m_alloc]         kept
    p.badx = p.hnx + scd_align((size_t)p.m_alloc * 4);                              // flag   int32 [m_alloc]         kept
    p.qnx = p.badx + scd_align((size_t)p.m_alloc * 4);                              // q(X)   f64   [m_alloc]         kept
    p.xend = p.qnx + scd_align((size_t)p.m_alloc * 8);
    p.gs = p.xend;                                                                  // gstat  u32   [4]
    p.qfx = p.gs + scd_align(16);                                                   // q(X)   f32   [m_alloc]
    p.rbx = p.qfx + scd_align((size_t)p.m_alloc * 4);                               // 1 / b  f32   [m_alloc]
    p.hq = p.rbx + scd_align((size_t)p.m_alloc * 4);                                // HQ     f16   [q_alloc, ld]
    p.eq = p.hq + scd_align((size_t)p.q_alloc * p.ld * 2);                          // e(Q)   f32   [q_alloc]
    p.hnq = p.eq + scd_align((size_t)p.q_alloc * 4);                                // h(Q)   f32   [q_alloc]
    p.badq = p.hnq + scd_align((size_t)p.q_alloc * 4);                              // flag   int32 [q_alloc]
    p.qnq = p.badq + scd_align((size_t)p.q_alloc * 4);                              // q(Q)   f64   [q_alloc]
    p.qfq = p.qnq + scd_align((size_t)p.q_alloc * 8);                               // q(Q)   f32   [q_alloc]
    p.raq = p.qfq + scd_align((size_t)p.q_alloc * 4);                               // 1 / a  f32   [q_alloc]
    p.cq = p.raq + scd_align((size_t)p.q_alloc * 4);                                // c      f32   [q_alloc]
    p.cand_v = p.cq + scd_align((size_t)p.q_alloc * 4);                             // cand_v f32   [ny_max, q_alloc, 16]
    p.theta = p.cand_v + scd_align((size_t)p.ny_max * p.q_alloc * 64);              // theta  f32   [q_alloc]
    p.cnt = p.theta + scd_align((size_t)p.q_alloc * 4);                             // cnt    int32 [q_alloc]
    p.slots = p.cnt + scd_align((size_t)p.q_alloc * 4);                             // slots  int32 [q_alloc, KNN_SLOTS]
    p.end = p.slots + scd_align((size_t)p.q_alloc * KNN_SLOTS * 4);
}

static bool ward_shape_ok(int64_t q, int64_t m, int d) {
    return q >= 1 && q < WARD_NMAX && m >= 2 && m < WARD_NMAX && d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX;
}

extern "C" size_t scd_ward_nearest_ws_bytes(int64_t q, int64_t m, int d) {
    if (!ward_shape_ok(q, m, d)) return 0;
    ward_plan p;
    ward_layout(q, m, d, p);
    return p.end;
}

extern "C" int scd_ward_nearest(scd_handle h, const float* Q, const int32_t* qcnt, const int32_t* qself, const float* X, const int32_t* xcnt,
                                int64_t q, int64_t m, int d, int64_t prepared, int32_t* nn_out, double* cost_out, int32_t* info_out, void* ws,
                                size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_ward_nearest");
    SCD_REQUIRE(Q && qcnt && qself && X && xcnt && nn_out && cost_out && info_out && ws, "scd_ward_nearest: null argument");
    SCD_REQUIRE(q >= 1 && q < WARD_NMAX, "scd_ward_nearest: q = %lld outside [1, 2^29)", (long long)q);
    SCD_REQUIRE(m >= 2 && m < WARD_NMAX, "scd_ward_nearest: m = %lld outside [2, 2^29)", (long long)m);
    SCD_REQUIRE(d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX, "scd_ward_nearest: d = %d outside [1, %d]", d, KNN_DP_MAX);
    SCD_REQUIRE(prepared >= 0 && prepared <= m, "scd_ward_nearest: prepared = %lld outside [0, m] (the leading positions whose data the workspace holds)",
                (long long)prepared);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_ward_nearest: workspace not 16-byte aligned");
    ward_plan p;
    ward_layout(q, m, d, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_ward_nearest: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    half_t* HX = (half_t*)(w + p.hx);
    float* ex = (float*)(w + p.ex);
    float* hnx = (float*)(w + p.hnx);
    int* badx = (int*)(w + p.badx);
    double* qnx = (double*)(w + p.qnx);
    unsigned* gs = (unsigned*)(w + p.gs);
    float* qfx = (float*)(w + p.qfx);
    float* rbx = (float*)(w + p.rbx);
    half_t* HQ = (half_t*)(w + p.hq);
    float* eq = (float*)(w + p.eq);
    float* hnq = (float*)(w + p.hnq);
    int* badq = (int*)(w + p.badq);
    double* qnq = (double*)(w + p.qnq);
    float* qfq = (float*)(w + p.qfq);
    float* raq = (float*)(w + p.raq);
    float* cq = (float*)(w + p.cq);
    float* cand_v = (float*)(w + p.cand_v);
    float* theta = (float*)(w + p.theta);
    int* cnt = (int*)(w + p.cnt);
    int* slots = (int*)(w + p.slots);

    SCD_HIP(hipMemsetAsync(info_out, 0, 16, st));
    SCD_HIP(hipMemsetAsync(gs, 0, 16, st));
    if (prepared < p.m_alloc)
        ward_prep_kernel<<<(unsigned)scd_cdiv(p.m_alloc - prepared, 4), 256, 0, st>>>(X, prepared, m, d, p.ld, p.m_alloc, HX, ex, hnx, badx, qnx);
    ward_prep_kernel<<<(unsigned)scd_cdiv(p.q_alloc, 4), 256, 0, st>>>(Q, 0, q, d, p.ld, p.q_alloc, HQ, eq, hnq, badq, qnq);
    ward_cols_kernel<<<(unsigned)scd_cdiv(p.m_alloc, 256), 256, 0, st>>>(xcnt, m, p.m_alloc, ex, hnx, badx, qnx, qfx, rbx, gs);
    ward_rows_kernel<<<(unsigned)scd_cdiv(p.q_alloc, 256), 256, 0, st>>>(qcnt, q, p.q_alloc, p.dp, eq, hnq, badq, qnq, gs, qfq, raq, cq, cnt);
    SCD_LAUNCH_CHECK();
    // ranges of column tiles (grid.y).  The result does not depend on the choice, and at k = 1 neither does the candidate count.
    long long ny = scd_cdiv(4ll * h->n_cu, p.panels);
    if (ny > p.ny_max) ny = p.ny_max;
    if (ny < 1) ny = 1;
    const long long tiles_per_y = scd_cdiv(p.xtiles, ny);
    ny = scd_cdiv(p.xtiles, tiles_per_y);                       // no empty range
    { const int rc_ = scd_set_max_lds((const void*)ward_bound_kernel, KNN_LDS_BYTES); if (rc_) return rc_; }
    { const int rc_ = scd_set_max_lds((const void*)ward_emit_kernel, KNN_LDS_BYTES); if (rc_) return rc_; }
    const dim3 grid((unsigned)p.panels, (unsigned)ny);
    ward_bound_kernel<<<grid, KNN_THREADS, KNN_LDS_BYTES, st>>>(HQ, HX, p.ld, p.dp, p.q_alloc, p.xtiles, tiles_per_y, qfq, raq, cq, qself, q, qfx, rbx,
                                                                cand_v);
    ward_thresh_kernel<<<(unsigned)scd_cdiv(p.q_alloc, 4), 256, 0, st>>>(cand_v, q, p.q_alloc, (int)ny, gs, theta);
    ward_emit_kernel<<<grid, KNN_THREADS, KNN_LDS_BYTES, st>>>(HQ, HX, p.ld, p.dp, p.xtiles, tiles_per_y, qfq, raq, cq, qself, q, qfx, rbx, theta, cnt,
                                                               slots);
    ward_refine_kernel<<<(unsigned)q, 64, 0, st>>>(Q, qcnt, qself, qnq, X, xcnt, qnx, m, d, theta, cnt, slots, gs, nn_out, cost_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_ward_merge(scd_handle h, float* X, int32_t* xcnt, const int32_t* lo, const int32_t* hi, int64_t pairs, int64_t m, int d,
                              void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_ward_merge");
    SCD_REQUIRE(X && xcnt && lo && hi && ws, "scd_ward_merge: null argument");
    SCD_REQUIRE(m >= 2 && m < WARD_NMAX, "scd_ward_merge: m = %lld outside [2, 2^29)", (long long)m);
    SCD_REQUIRE(d >= 1 && scd_cdiv(d, 32) * 32 <= KNN_DP_MAX, "scd_ward_merge: d = %d outside [1, %d]", d, KNN_DP_MAX);
    SCD_REQUIRE(pairs >= 0 && pairs <= m / 2, "scd_ward_merge: %lld pairs for %lld positions", (long long)pairs, (long long)m);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_ward_merge: workspace not 16-byte aligned");
    ward_plan p;
    ward_layout(1, m, d, p);
    SCD_REQUIRE(ws_bytes >= p.xend, "scd_ward_merge: workspace too small (%zu < %zu bytes)", ws_bytes, p.xend);
    if (pairs == 0) return SCD_OK;
    char* w = (char*)ws;
    ward_merge_kernel<<<(unsigned)pairs, 64, 0, (hipStream_t)stream_>>>(X, xcnt, lo, hi, m, d, p.ld, (half_t*)(w + p.hx), (float*)(w + p.ex),
                                                                        (float*)(w + p.hnx), (int*)(w + p.badx), (double*)(w + p.qnx));
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
