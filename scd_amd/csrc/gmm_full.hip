// Gaussian mixtures with a full covariance matrix per component on gfx950, for rows of at most 64 dimensions (the output of
// scd_amd.pca.PCA): one EM step of scikit-learn's GaussianMixture(covariance_type='full'; 'tied' is the same call with one factor
// replicated) with labelled rows clamped to their class, and the forward pass alone.  docs/design/gmm_full.md has the semantics, the
// error model and the resources.  The MFMA row map, the chain rule, the float64 range sums and the range plan are f32mm.h's.
//
//   scd_gmm_full_em_step   c_ikl = fl32(x_il - mu_kl) (one IEEE subtraction in a register), y_ikj = sum_l c_ikl U_k[l][j] (U_k upper
//                          triangular, U_k U_k^T = Sigma_k^-1, given transposed: Ut[k][j][l] = U_k[l][j]), q_ik = sum_j y_ikj^2,
//                          z_ik = a_k - 0.5 q_ik; the softmax, the clamp, ll and argmax as scd_gmm_em_step; nk = column sums of r,
//                          s1c = sum_i r_ik c_ik, S = sum_i r_ik c_ik c_ik^T, in four steps:
//                            1. gmmf_pack_kernel: Ut [k, d, d] -> Utp [k, jp, dp] and mu [k, d] -> mup [k, dp] (jp = d up to 32, dp = d up
//                               to 8, zero filled), each octet of l stored as l+0, l+2, l+4, l+6, l+1, l+3, l+5, l+7 (f32mm_pack's order):
//                               lane half h of the MFMA reads its four l values with one 16-byte load;
//                            2. gmmf_fwd_kernel: a block owns F32MM_RT = 32 rows and all k components, wave w the components w, w + 4, ...
//                               The MFMA's M axis is j (A = rows of Utp), N the 32 data rows (B = x - mu_k, x from LDS, one subtraction
//                               per MFMA operand), K = l: a fma chain with l ascending from a zero accumulator, stopped after the
//                               j-tile's last column (l < 32 (jt + 1): the entries beyond are exact zeros of the triangle).  A lane then
//                               holds 16 values of j of ONE data row per j-tile: q = a fmaf chain of the squares over j-tiles ascending
//                               and accumulator registers ascending (lane half h holds j = 32 jt + 8 (reg / 4) + 4 h + reg % 4), then the
//                               two halves' sums added.  z = fmaf(-0.5, q, a_k) -> LDS [kp][33] (dynamic, at most 132 KiB); no logit
//                               reaches global memory.  The row softmax runs from LDS: eight threads a row (components t, t + 8, ...),
//                               their maxima, lowest argmax and sums of expf(z - max) combined in ascending order; then r = s (e / sum)
//                               or the label's one-hot -> r [n, kp] float32 (padding columns 0), stored a row at a time;
//                            3. gmmf_moment_kernel: a block owns four components (a wave each) and one row range; A = r_ik c_ij (one
//                               float32 product), B = c_il, K = rows; the lower-triangle 32 x 32 tiles (j-tile >= l-tile) run over chains
//                               of F32MM_CHAIN = 256 rows into float64 registers -> part [R, k, d, d] (entries j >= l only).  s1c is
//                               summed in float64 (the product r c is exact there): a lane sums its rows in ascending order, then the
//                               two lane halves are added -> s1part [R, k, d].  gmmf_nk_kernel: float64 column sums of r and sums of the
//                               row log-likelihoods over RB row ranges;
//                            4. gmmf_finish_kernel: the ranges' partials in ascending order; S[k][j][l] and S[k][l][j] are the same sum.
//                          With a == Ut == NULL step 2 is gmmf_hard_kernel (r = s_i [k == y_i]), ll = 0; mu holds the centres.
//   scd_gmm_full_predict   steps 1 and 2 alone: argmax, lse and the softmax of each row.
//
// No floating-point atomics (the two info counters are integers).  R, RB and every tile depend on (n, d, k) alone.
#include "f32mm.h"

#define GMMF_DMAX 64
#define GMMF_ZLD 33                             // row stride of the logits in LDS: [component][32 rows + 1]
#define GMMF_ZL_MAX_BYTES (F32MM_WMAX * GMMF_ZLD * 4)
#define GMMF_MXLD 96                            // row stride of the moment kernel's X tile: lane halves (rows r, r + 1) on distinct banks
#define GMMF_CG 4                               // components of a moment block, one a wave

// ------------------------------------------------------------------------------------------------ 1. pack Ut and mu
__global__ void __launch_bounds__(256) gmmf_pack_kernel(const float* __restrict__ Ut, const float* __restrict__ mu, int k, int d, int jp, int dp,
                                                        float* __restrict__ Utp, float* __restrict__ mup) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nu = (long long)k * jp * dp;
    if (e < nu) {
        const int pos = (int)(e % dp), j = (int)((e / dp) % jp), comp = (int)(e / ((long long)dp * jp));
        const int l = (pos & ~7) + 2 * (pos & 3) + ((pos & 7) >> 2);
        Utp[e] = (Ut && j < d && l < d) ? Ut[((size_t)comp * d + j) * d + l] : 0.f;
    } else if (e < nu + (long long)k * dp) {
        const long long f = e - nu;
        const int pos = (int)(f % dp), comp = (int)(f / dp);
        const int l = (pos & ~7) + 2 * (pos & 3) + ((pos & 7) >> 2);
        mup[f] = l < d ? mu[(size_t)comp * d + l] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ 2. logits, softmax, responsibilities
// PREDICT = false: r [n, kp] (the clamped responsibilities times the weight), rowll double [n].
// PREDICT = true:  r = resp [n, k] dense (the softmax) or NULL, rowlse float [n] or NULL; y, sw are not read.
template <bool PREDICT>
__global__ void __launch_bounds__(F32MM_THREADS) gmmf_fwd_kernel(const float* __restrict__ X, const int* __restrict__ y, const float* __restrict__ sw,
                                                                 long long n, int d, int dp, int jp, int k, int kp, const float* __restrict__ Utp,
                                                                 const float* __restrict__ mup, const float* __restrict__ a, float* __restrict__ r,
                                                                 double* __restrict__ rowll, float* __restrict__ rowlse, int* __restrict__ pred,
                                                                 int* __restrict__ info) {
    extern __shared__ float zl[];               // [kp][GMMF_ZLD]: the logit of (component, row)
    __shared__ float xs[F32MM_RT * F32MM_XLD];
    __shared__ float pm[8][F32MM_RT];           // per row part: maximum, then sum of e
    __shared__ int pc[8][F32MM_RT];             // per row part: lowest component at its maximum
    __shared__ int pb[8][F32MM_RT];             // per row part: a non-finite logit seen
    __shared__ float m_s[F32MM_RT], sum_s[F32MM_RT], s_s[F32MM_RT];
    __shared__ int y_s[F32MM_RT];
    const long long row0 = (long long)blockIdx.x * F32MM_RT;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;

    // the 32 rows, all d <= 64 columns, zero beyond n and d (addresses clamped, values masked)
#pragma unroll
    for (int i = 0; i < F32MM_RT * F32MM_BK / F32MM_THREADS; ++i) {
        const int idx = tid + F32MM_THREADS * i, row = idx >> 6, kk = idx & 63;
        const long long g = row0 + row < n ? row0 + row : n - 1;
        const float v = X[(size_t)g * d + (kk < d ? kk : d - 1)];
        xs[row * F32MM_XLD + kk] = (row0 + row < n && kk < d) ? v : 0.f;
    }
    if (tid < F32MM_RT) {
        const long long g = row0 + tid;
        int yy = -1;
        float s = 0.f;
        if (g < n) {
            s = (!PREDICT && sw) ? sw[g] : 1.f;
            if (!PREDICT && y) {
                yy = y[g];
                if (yy >= k) atomicAdd(&info[0], 1);            // treated as unlabelled, and counted
                if (yy < 0 || yy >= k) yy = -1;
            }
        }
        y_s[tid] = yy;
        s_s[tid] = s;
    }
    __syncthreads();

    const int jtiles = jp >> 5;
    for (int comp = wave; comp < k; comp += 4) {
        const float* mp = mup + (size_t)comp * dp + 4 * h;
        float q = 0.f;
        for (int jt = 0; jt < jtiles; ++jt) {
            f32x16 acc;
#pragma unroll
            for (int t = 0; t < 16; ++t) acc[t] = 0.f;
            const float* up = Utp + ((size_t)comp * jp + jt * 32 + li) * dp + 4 * h;
            const int lend = dp < 32 * (jt + 1) ? dp : 32 * (jt + 1);           // a multiple of 8; beyond it the triangle is zero
            f32x4 u4 = *reinterpret_cast<const f32x4*>(up), m4 = *reinterpret_cast<const f32x4*>(mp);
            for (int l0 = 0; l0 < lend; l0 += 8) {
                const int ln = l0 + 8 < lend ? l0 + 8 : l0;                     // the next octet's operands while the MFMAs run
                const f32x4 un = *reinterpret_cast<const f32x4*>(up + ln), mn = *reinterpret_cast<const f32x4*>(mp + ln);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float c = xs[li * F32MM_XLD + l0 + 2 * j + h] - m4[j];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(u4[j], c, acc, 0, 0, 0);
                }
                u4 = un;
                m4 = mn;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) q = fmaf(acc[t], acc[t], q);
        }
        q += __shfl_xor(q, 32, 64);
        if (h == 0) zl[comp * GMMF_ZLD + li] = fmaf(-0.5f, q, a[comp]);
    }
    __syncthreads();

    // the row statistics: eight threads a row, the parts combined in ascending order
    const int row = tid & 31, part = tid >> 5;
    {
        float m = -INFINITY;
        int cand = 0x7fffffff, bad = 0;
        for (int comp = part; comp < k; comp += 8) {
            const float z = zl[comp * GMMF_ZLD + row];
            if (!(fabsf(z) < INFINITY)) bad = 1;
            if (z > m || (cand == 0x7fffffff && z == m)) {      // ascending components: the lowest at the maximum is kept
                m = z;
                cand = comp;
            }
        }
        pm[part][row] = m;
        pc[part][row] = cand;
        pb[part][row] = bad;
    }
    __syncthreads();
    float mx = pm[0][row];
#pragma unroll
    for (int p = 1; p < 8; ++p) mx = fmaxf(mx, pm[p][row]);
    int best = 0x7fffffff, bad = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        if (pm[p][row] == mx && pc[p][row] < best) best = pc[p][row];
        bad |= pb[p][row];
    }
    __syncthreads();
    {
        float sum = 0.f;
        for (int comp = part; comp < k; comp += 8) sum += expf(zl[comp * GMMF_ZLD + row] - mx);
        pm[part][row] = sum;
    }
    __syncthreads();
    if (tid < F32MM_RT) {
        float sm = pm[0][tid];
#pragma unroll
        for (int p = 1; p < 8; ++p) sm += pm[p][tid];
        m_s[tid] = mx;
        sum_s[tid] = sm;
        const long long g = row0 + tid;
        if (g < n) {
            if (best == 0x7fffffff) best = 0;                   // no component compares equal: a NaN row, counted below
            if (pred) pred[g] = best;
            if (bad) atomicAdd(&info[1], 1);
            const double lse = (double)mx + (double)logf(sm);
            if (PREDICT) {
                if (rowlse) rowlse[g] = (float)lse;
            } else {
                const float s = s_s[tid];
                const int yy = y_s[tid];
                rowll[g] = s == 0.f ? 0.0 : (double)s * (yy >= 0 ? (double)zl[yy * GMMF_ZLD + tid] : lse);
            }
        }
    }
    __syncthreads();

    if (r) {
        const int width = PREDICT ? k : kp;
        for (int rr = 0; rr < F32MM_RT; ++rr) {
            const long long g = row0 + rr;
            if (g >= n) break;
            const float m = m_s[rr], sm = sum_s[rr], s = s_s[rr];
            const int yy = y_s[rr];
            for (int comp = tid; comp < width; comp += F32MM_THREADS) {
                float v = 0.f;
                if (comp < k) {
                    const float p = expf(zl[comp * GMMF_ZLD + rr] - m) / sm;
                    v = PREDICT ? p : (yy >= 0 ? (comp == yy ? s : 0.f) : s * p);
                }
                r[(size_t)g * width + comp] = v;
            }
        }
    }
}

// the hard M-step's responsibilities: one block per row.  r = s [comp == y] where 0 <= y < k, 0 elsewhere
__global__ void __launch_bounds__(256) gmmf_hard_kernel(const int* __restrict__ y, const float* __restrict__ sw, int k, int kp, float* __restrict__ r,
                                                        int* __restrict__ info) {
    const long long g = blockIdx.x;
    const int yy = y[g];
    const float s = sw ? sw[g] : 1.f;
    if (threadIdx.x == 0 && yy >= k) atomicAdd(&info[0], 1);
    for (int comp = threadIdx.x; comp < kp; comp += 256) r[(size_t)g * kp + comp] = (yy >= 0 && yy < k && comp == yy) ? s : 0.f;
}

// ------------------------------------------------------------------------------------------------ 3. moment partials, nk and ll partials
// grid (kp / 4, R).  Wave w owns component 4 blockIdx.x + w.  JT = j-tiles of 32 (1: d <= 32, 2: d <= 64); the tiles (jt, lt) with
// jt >= lt are kept: (0,0) | (0,0), (1,0), (1,1).  part [R, k, d, d] float64, entries j >= l; s1part [R, k, d] float64.
template <int JT>
__global__ void __launch_bounds__(F32MM_THREADS) gmmf_moment_kernel(const float* __restrict__ r, const float* __restrict__ X, const float* __restrict__ mu,
                                                                    long long n, int d, int k, int kp, long long rows_per_range,
                                                                    double* __restrict__ part, double* __restrict__ s1part) {
    constexpr int NTL = JT * (JT + 1) / 2, XPT = F32MM_GK * 32 * JT / F32MM_THREADS;
    __shared__ float xs[F32MM_GK * GMMF_MXLD];
    __shared__ float rs[F32MM_GK * GMMF_CG];
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int c0 = blockIdx.x * GMMF_CG, comp = c0 + wave;
    const bool active = comp < k;                               // wave-uniform; a padding component's r column is zero
    float mu_l[JT];
#pragma unroll
    for (int t = 0; t < JT; ++t) mu_l[t] = (active && 32 * t + li < d) ? mu[(size_t)comp * d + 32 * t + li] : 0.f;

    f32x16 acc[NTL];
    double acc64[NTL][16], s1[JT];
#pragma unroll
    for (int t = 0; t < NTL; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            acc[t][q] = 0.f;
            acc64[t][q] = 0.0;
        }
#pragma unroll
    for (int t = 0; t < JT; ++t) s1[t] = 0.0;

    // no branch around a load: the next 32 rows are in registers while the MFMAs run (addresses clamped, values masked)
    float xr[XPT], rr = 0.f;
    auto load_rows = [&](long long base) {
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx / (32 * JT), col = idx % (32 * JT);
            const long long g = base + row < hi ? base + row : hi - 1;
            xr[i] = X[(size_t)g * d + (col < d ? col : d - 1)];
        }
        if (tid < F32MM_GK * GMMF_CG) {
            const long long g = base + (tid >> 2) < hi ? base + (tid >> 2) : hi - 1;
            rr = r[(size_t)g * kp + c0 + (tid & 3)];
        }
    };
    load_rows(lo);
    for (long long base = lo; base < hi; base += F32MM_GK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx / (32 * JT), col = idx % (32 * JT);
            xs[row * GMMF_MXLD + col] = (base + row < hi && col < d) ? xr[i] : 0.f;
        }
        if (tid < F32MM_GK * GMMF_CG) rs[tid] = base + (tid >> 2) < hi ? rr : 0.f;
        __syncthreads();
        load_rows(base + F32MM_GK);
        if (active) {
#pragma unroll 4
            for (int s = 0; s < F32MM_GK / 2; ++s) {
                const int row = 2 * s + h;
                const float w = rs[row * GMMF_CG + wave];
                float cv[JT], av[JT];
#pragma unroll
                for (int t = 0; t < JT; ++t) {
                    cv[t] = 32 * t + li < d ? xs[row * GMMF_MXLD + 32 * t + li] - mu_l[t] : 0.f;
                    av[t] = w * cv[t];
                    s1[t] += (double)w * (double)cv[t];
                }
                int tl = 0;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int lt = 0; lt <= jt; ++lt, ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[jt], cv[lt], acc[tl], 0, 0, 0);
            }
        }
        if ((base - lo + F32MM_GK) % F32MM_CHAIN == 0 || base + F32MM_GK >= hi) {  // the end of a chain: into float64
#pragma unroll
            for (int t = 0; t < NTL; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    acc64[t][q] += (double)acc[t][q];
                    acc[t][q] = 0.f;
                }
        }
    }
    if (!active) return;
    double* out = part + ((size_t)blockIdx.y * k + comp) * d * d;
    int tl = 0;
#pragma unroll
    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
        for (int lt = 0; lt <= jt; ++lt, ++tl)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = jt * 32 + f32mm_row(q, h), l = lt * 32 + li;
                if (j < d && l < d && j >= l) out[(size_t)j * d + l] = acc64[tl][q];
            }
#pragma unroll
    for (int t = 0; t < JT; ++t) {
        const double tot = s1[t] + __shfl_xor(s1[t], 32, 64);
        if (h == 0 && 32 * t + li < d) s1part[((size_t)blockIdx.y * k + comp) * d + 32 * t + li] = tot;
    }
}

// grid (kp / 32, RB): float64 column sums of r over a row range -> nkpart [RB, kp]; the blocks of column group 0 also sum the range's
// row log-likelihoods -> llpart [RB]
__global__ void __launch_bounds__(F32MM_THREADS) gmmf_nk_kernel(const float* __restrict__ r, const double* __restrict__ rowll, long long n, int kp,
                                                                long long rows_per_range, double* __restrict__ nkpart, double* __restrict__ llpart) {
    __shared__ double sh[F32MM_THREADS];
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
    const int tid = threadIdx.x, comp = blockIdx.x * 32 + (tid & 31);
    const double t = f32mm_colsum(lo, hi, [&](long long g) { return r[(size_t)g * kp + comp]; }, sh);
    if (tid < 32) nkpart[(size_t)blockIdx.y * kp + comp] = t;
    if (blockIdx.x != 0) return;
    const double l = f32mm_rowsum(rowll, lo, hi, sh);
    if (tid == 0) llpart[blockIdx.y] = l;
}

// ------------------------------------------------------------------------------------------------ 4. the ranges in ascending order
__global__ void __launch_bounds__(256) gmmf_finish_kernel(const double* __restrict__ part, const double* __restrict__ s1part,
                                                          const double* __restrict__ nkpart, const double* __restrict__ llpart, int k, int d, int kp,
                                                          int R, int RB, double* __restrict__ S, double* __restrict__ s1c, double* __restrict__ nk,
                                                          double* __restrict__ ll) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long kd = (long long)k * d, kdd = kd * d;
    if (e < kdd) {
        const int l = (int)(e % d), j = (int)((e / d) % d);
        const long long comp = e / ((long long)d * d);
        const int hi = j > l ? j : l, lw = j > l ? l : j;       // both halves of the matrix from the one sum of the lower triangle
        S[e] = f32mm_range_sum(part, (size_t)kdd, (size_t)((comp * d + hi) * d + lw), R);
    } else if (e < kdd + kd) {
        s1c[e - kdd] = f32mm_range_sum(s1part, (size_t)kd, (size_t)(e - kdd), R);
    } else if (e < kdd + kd + k) {
        const int comp = (int)(e - kdd - kd);
        nk[comp] = f32mm_range_sum(nkpart, kp, comp, RB);
    } else if (e == kdd + kd + k) {
        ll[0] = f32mm_range_sum(llpart, 1, 0, RB);
    }
}

struct gmmf_plan {
    int kp, dp, jp, R, RB;
    long long rows_per_range, nk_rows;
    size_t utp, mup, r, rowll, part, s1part, nkpart, llpart, end;
};

static bool gmmf_shape_ok(int64_t n, int d, int k) { return n >= 1 && n < (1ll << 31) && d >= 1 && d <= GMMF_DMAX && k >= 1 && k <= F32MM_WMAX; }

static void gmmf_layout(int64_t n, int d, int k, gmmf_plan& p) {
    p.kp = f32mm_pad(k, 32);
    p.dp = f32mm_pad(d, 8);
    p.jp = f32mm_pad(d, 32);
    // about 1024 moment blocks; at k = 1000, d = 64 a range's S partial is 32 MB and R = 4
    f32mm_ranges(n, p.kp / GMMF_CG, 1024, p.R, p.rows_per_range);
    f32mm_colsum_ranges(n, p.RB, p.nk_rows);
    p.utp = 0;                                                                      // Utp    f32 [k, jp, dp]
    p.mup = p.utp + scd_align((size_t)k * p.jp * p.dp * 4);                         // mup    f32 [k, dp]
    p.r = p.mup + scd_align((size_t)k * p.dp * 4);                                  // r      f32 [n, kp]
    p.rowll = p.r + scd_align((size_t)n * p.kp * 4);                                // rowll  f64 [n]
    p.part = p.rowll + scd_align((size_t)n * 8);                                    // part   f64 [R, k, d, d]
    p.s1part = p.part + scd_align((size_t)p.R * k * d * d * 8);                     // s1part f64 [R, k, d]
    p.nkpart = p.s1part + scd_align((size_t)p.R * k * d * 8);                       // nkpart f64 [RB, kp]
    p.llpart = p.nkpart + scd_align((size_t)p.RB * p.kp * 8);                       // llpart f64 [RB]
    p.end = p.llpart + scd_align((size_t)p.RB * 8);
}

extern "C" int scd_gmm_full_row_tile(void) { return F32MM_RT; }
extern "C" int scd_gmm_full_chain_rows(void) { return F32MM_CHAIN; }

extern "C" size_t scd_gmm_full_ws_bytes(int64_t n, int d, int k) {
    if (!gmmf_shape_ok(n, d, k)) return 0;
    gmmf_plan p;
    gmmf_layout(n, d, k, p);
    return p.end;
}

#define GMMF_SHAPE_REQUIRE(who)                                                                 \
    F32MM_ND_REQUIRE(who, n, d);                                                                \
    SCD_REQUIRE(d <= GMMF_DMAX, who ": d = %d outside [1, %d]; reduce the rows first", d, GMMF_DMAX); \
    F32MM_WIDTH_REQUIRE(who, "k", k, 1);                                                        \
    F32MM_WS_REQUIRE(who, ws)

extern "C" int scd_gmm_full_em_step(scd_handle h, const float* X, const int32_t* y, const float* sample_weight, int64_t n, int d, int k,
                                    const float* a, const float* mu, const float* Ut, double* ll_out, double* nk_out, double* s1c_out,
                                    double* S_out, int32_t* pred_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_gmm_full_em_step");
    SCD_REQUIRE(X && mu && ll_out && nk_out && s1c_out && S_out && info_out && ws, "scd_gmm_full_em_step: null argument");
    const bool hard = !a && !Ut;
    SCD_REQUIRE(hard || (a && Ut), "scd_gmm_full_em_step: a and Ut must be both given or both NULL");
    SCD_REQUIRE(!hard || y, "scd_gmm_full_em_step: the hard M-step (a == Ut == NULL) needs labels");
    GMMF_SHAPE_REQUIRE("scd_gmm_full_em_step");
    gmmf_plan p;
    gmmf_layout(n, d, k, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_gmm_full_em_step: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    float* Utp = (float*)(w + p.utp);
    float* mup = (float*)(w + p.mup);
    float* r = (float*)(w + p.r);
    double* rowll = (double*)(w + p.rowll);
    double* part = (double*)(w + p.part);
    double* s1part = (double*)(w + p.s1part);
    double* nkpart = (double*)(w + p.nkpart);
    double* llpart = (double*)(w + p.llpart);

    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    if (hard) {
        SCD_HIP(hipMemsetAsync(rowll, 0, (size_t)n * 8, st));
        gmmf_hard_kernel<<<(unsigned)n, 256, 0, st>>>(y, sample_weight, k, p.kp, r, info_out);
    } else {
        { const int rc_ = scd_set_max_lds((const void*)gmmf_fwd_kernel<false>, GMMF_ZL_MAX_BYTES); if (rc_) return rc_; }
        gmmf_pack_kernel<<<(unsigned)scd_cdiv((int64_t)k * p.jp * p.dp + (int64_t)k * p.dp, 256), 256, 0, st>>>(Ut, mu, k, d, p.jp, p.dp, Utp, mup);
        gmmf_fwd_kernel<false><<<(unsigned)scd_cdiv(n, F32MM_RT), F32MM_THREADS, (size_t)p.kp * GMMF_ZLD * 4, st>>>(
            X, y, sample_weight, n, d, p.dp, p.jp, k, p.kp, Utp, mup, a, r, rowll, nullptr, pred_out, info_out);
    }
    const dim3 mgrid((unsigned)(p.kp / GMMF_CG), (unsigned)p.R);
    if (d <= 32)
        gmmf_moment_kernel<1><<<mgrid, F32MM_THREADS, 0, st>>>(r, X, mu, n, d, k, p.kp, p.rows_per_range, part, s1part);
    else
        gmmf_moment_kernel<2><<<mgrid, F32MM_THREADS, 0, st>>>(r, X, mu, n, d, k, p.kp, p.rows_per_range, part, s1part);
    gmmf_nk_kernel<<<dim3((unsigned)(p.kp / 32), (unsigned)p.RB), F32MM_THREADS, 0, st>>>(r, rowll, n, p.kp, p.nk_rows, nkpart, llpart);
    gmmf_finish_kernel<<<(unsigned)scd_cdiv((int64_t)k * d * d + (int64_t)k * d + k + 1, 256), 256, 0, st>>>(
        part, s1part, nkpart, llpart, k, d, p.kp, p.R, p.RB, S_out, s1c_out, nk_out, ll_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_gmm_full_predict(scd_handle h, const float* X, int64_t n, int d, int k, const float* a, const float* mu, const float* Ut,
                                    int32_t* pred_out, float* row_ll_out, float* resp_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_gmm_full_predict");
    SCD_REQUIRE(X && a && mu && Ut && ws, "scd_gmm_full_predict: null argument");
    GMMF_SHAPE_REQUIRE("scd_gmm_full_predict");
    gmmf_plan p;
    gmmf_layout(1, d, k, p);                                    // only the packed Ut and mu are needed
    SCD_REQUIRE(ws_bytes >= p.end, "scd_gmm_full_predict: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    float* Utp = (float*)((char*)ws + p.utp);
    float* mup = (float*)((char*)ws + p.mup);
    int* info = (int*)((char*)ws + p.r);                        // the two counters of the forward kernel: not reported
    SCD_HIP(hipMemsetAsync(info, 0, 8, st));
    { const int rc_ = scd_set_max_lds((const void*)gmmf_fwd_kernel<true>, GMMF_ZL_MAX_BYTES); if (rc_) return rc_; }
    gmmf_pack_kernel<<<(unsigned)scd_cdiv((int64_t)k * p.jp * p.dp + (int64_t)k * p.dp, 256), 256, 0, st>>>(Ut, mu, k, d, p.jp, p.dp, Utp, mup);
    gmmf_fwd_kernel<true><<<(unsigned)scd_cdiv(n, F32MM_RT), F32MM_THREADS, (size_t)p.kp * GMMF_ZLD * 4, st>>>(
        X, nullptr, nullptr, n, d, p.dp, p.jp, k, p.kp, Utp, mup, a, resp_out, nullptr, row_ll_out, pred_out, info);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
