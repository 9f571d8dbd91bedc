// Gaussian mixtures with diagonal covariances on gfx950: one EM step of scikit-learn's GaussianMixture(covariance_type='diag' |
// 'spherical') with labelled rows clamped to their class (the semi-supervised mixture of GPC), and the forward pass alone.
// docs/design/gmm.md has the semantics, the error model and the resources.
// The tile shapes, the k-octet packing, the float64 range sums and the host's range plan are f32mm.h's, shared with probe.hip and pca.hip.
//
//   scd_gmm_em_step   z_ik = a_k + sum_d x_id B_kd + sum_d x_id^2 C_kd (the weighted log-density; the caller forms a, B = mu / v and
//                     C = -1 / (2 v) in float64 and rounds them to float32), r_ik = s_i softmax_k(z_i) on an unlabelled row and
//                     s_i [k == y_i] on a labelled one, ll = sum_i s_i (lse_k z_ik | z_{i,y_i}), nk = column sums of r, s1 = r^T X,
//                     s2 = r^T (X o X), in four steps:
//                       1. gmm_pack_kernel: B, C [k, d] -> BCp [kp, 2 dp] (kp = k up to 32, dp = d up to 8, zero filled), B and C
//                          interleaved by k-octet: 16 floats per octet, B as k+0, k+2, k+4, k+6, k+1, k+3, k+5, k+7, then C the same
//                          way.  Lane half h of the MFMA reads its four k values of a stream with one 16-byte load, and the two
//                          streams of an octet share one 64-byte segment: a wave's 32 components touch 32 segments per octet, where
//                          two slabs would touch 64 half-used ones a slab apart;
//                       2. gmm_fwd_kernel: a block owns F32MM_RT = 32 rows and all kp components, wave w the 32-component tiles w, w + 4,
//                          ... in up to 8 accumulator tiles of v_mfma_f32_32x32x2_f32.  X goes through LDS once, in chunks of 64 k;
//                          each staged x feeds two MFMAs, x against B and x * x (one float32 multiply in a register) against C.
//                          The accumulator starts at zero; octets of k ascend; within an octet the eight x B products come first (k
//                          ascending), then the eight x^2 C products (k ascending); a_k is added last.  The softmax stays in
//                          registers as in probe.hip: maximum over the real components (by index), e = expf(z - max), row sum,
//                          r = s (e / sum) or the one-hot of the label -> r [n, kp] fp32 (padding columns 0), the row's
//                          log-likelihood in float64 -> [n], argmax = the lowest component that attains the maximum;
//                       3. gmm_moment_kernel: 128 x 128 tiles of (component, dim) times R row ranges times the two moments
//                          (blockIdx.z = 1 squares x as it is staged); the float32 MFMA runs over chains of at most F32MM_CHAIN = 256
//                          rows, each chain's tile is added into float64 registers -> part [2, R, k, d].  gmm_nk_kernel: float64
//                          column sums of r and float64 sums of the row log-likelihoods over RB row ranges;
//                       4. gmm_finish_kernel: the ranges' partials added in ascending order -> ll, nk, s1, s2 (float64).
//                     With a == B == C == NULL step 2 is gmm_hard_kernel: r = s_i [k == y_i] on rows with a label in range, 0
//                     elsewhere, ll = 0 (the hard M-step a k-means start needs).
//   scd_gmm_predict   steps 1 and 2 alone: argmax, lse and the softmax of each row.
//
// No floating-point atomics (the two info counters are integers).  R, RB and every tile depend on (n, d, k) alone: two calls return the
// same bits on any device.
#include "f32mm.h"

// ------------------------------------------------------------------------------------------------ 1. pack B and C
__global__ void __launch_bounds__(256) gmm_pack_kernel(const float* __restrict__ B, const float* __restrict__ Cq, int k, int d, int kp, int dp,
                                                       float* __restrict__ BCp) {
    const float* const src[2] = {B, Cq};
    f32mm_pack<2>(src, k, d, kp, dp, BCp);
}

// ------------------------------------------------------------------------------------------------ 2. logits, softmax, responsibilities
// PREDICT = false: r [n, kp] (the clamped responsibilities times the weight), rowll double [n].
// PREDICT = true:  resp [n, k] dense (the softmax), rowlse float [n]; y, sw are not read.
template <int NT, bool PREDICT>
__global__ void __launch_bounds__(F32MM_THREADS) gmm_fwd_kernel(const float* __restrict__ X, const int* __restrict__ y, const float* __restrict__ sw,
                                                             long long n, int d, int dp, int k, int kp, const float* __restrict__ BCp,
                                                             const float* __restrict__ a, float* __restrict__ r, double* __restrict__ rowll,
                                                             float* __restrict__ rowlse, int* __restrict__ pred, int* __restrict__ info) {
    __shared__ float xs[F32MM_RT * F32MM_XLD];
    __shared__ float red_a[4][F32MM_RT];        // per wave: row maximum
    __shared__ float red_b[4][F32MM_RT];        // per wave: row sum of e
    __shared__ int red_i[4][F32MM_RT];          // per wave: lowest component at the maximum
    __shared__ float zy_s[F32MM_RT], s_s[F32MM_RT];
    __shared__ int y_s[F32MM_RT], bad_s[F32MM_RT];
    const long long row0 = (long long)blockIdx.x * F32MM_RT;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;

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
        zy_s[tid] = 0.f;
        bad_s[tid] = 0;
    }

    f32x16 acc[NT];
    int woff[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
        const int comp = (t * 4 + wave) * 32 + li;
        woff[t] = (comp < kp ? comp : kp - 1) * 2 * dp + 4 * h; // a tile past kp repeats the last row: computed, never used
    }

    // no branch around a load: the chunk after the current one is in registers while the MFMAs run (addresses clamped, values masked);
    // the operand after the current one (C of this octet, then B of the next) is in registers as well
    float xr[F32MM_RT * F32MM_BK / F32MM_THREADS];
    f32x4 cur[NT], nx[NT];
    auto load_x = [&](int k0) {
#pragma unroll
        for (int i = 0; i < F32MM_RT * F32MM_BK / F32MM_THREADS; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx >> 6, kk = k0 + (idx & 63);
            const long long g = row0 + row < n ? row0 + row : n - 1;
            xr[i] = X[(size_t)g * d + (kk < d ? kk : d - 1)];
        }
    };
    load_x(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) cur[t] = *reinterpret_cast<const f32x4*>(BCp + woff[t]);
    for (int k0 = 0; k0 < dp; k0 += F32MM_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < F32MM_RT * F32MM_BK / F32MM_THREADS; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx >> 6, kk = idx & 63;
            xs[row * F32MM_XLD + kk] = (row0 + row < n && k0 + kk < d) ? xr[i] : 0.f;
        }
        __syncthreads();
        load_x(k0 + F32MM_BK);
        const int kend = dp - k0 < F32MM_BK ? dp - k0 : F32MM_BK;               // a multiple of 8
        for (int k8 = 0; k8 < kend; k8 += 8) {
            const int oct = 2 * (k0 + k8);                      // floats from the row's start to this octet's B
            const int onext = k0 + k8 + 8 < dp ? oct + 16 : oct;
            float xv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[j] = xs[li * F32MM_XLD + k8 + 2 * j + h];
            // x against B
#pragma unroll
            for (int t = 0; t < NT; ++t) nx[t] = *reinterpret_cast<const f32x4*>(BCp + woff[t] + oct + 8);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j], cur[t][j], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) cur[t] = nx[t];
            // x * x against C
#pragma unroll
            for (int t = 0; t < NT; ++t) nx[t] = *reinterpret_cast<const f32x4*>(BCp + woff[t] + onext);
#pragma unroll
            for (int j = 0; j < 4; ++j) xv[j] = xv[j] * xv[j];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[j], cur[t][j], acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) cur[t] = nx[t];
        }
    }

    // acc[t][q] = z of row f32mm_row(q, h), component (4 t + wave) * 32 + li, without a
    float m[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) m[q] = -INFINITY;
    int bad = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int comp = (t * 4 + wave) * 32 + li;
        const bool valid = comp < k;
        const float aa = valid ? a[comp] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float z = acc[t][q] + aa;
            acc[t][q] = z;
            if (valid) {
                if (!(fabsf(z) < INFINITY)) bad |= 1 << q;
                m[q] = fmaxf(m[q], z);
            }
        }
    }
    if (bad) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (bad & (1 << q)) atomicOr(&bad_s[f32mm_row(q, h)], 1);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < 16; ++q) m[q] = fmaxf(m[q], __shfl_xor(m[q], o, 64));
    if (li == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) red_a[wave][f32mm_row(q, h)] = m[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = f32mm_row(q, h);
        float v = red_a[0][row];
#pragma unroll
        for (int w = 1; w < 4; ++w) v = fmaxf(v, red_a[w][row]);
        m[q] = v;
    }

    // the lowest component at the maximum; e and its row sum; the label's logit
    float sum[16], sv[16];
    int cand[16], yv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        sum[q] = 0.f;
        cand[q] = 0x7fffffff;
        yv[q] = y_s[f32mm_row(q, h)];
        sv[q] = s_s[f32mm_row(q, h)];
    }
#pragma unroll
    for (int t = NT - 1; t >= 0; --t) {                         // descending: the lowest component is kept last
        const int comp = (t * 4 + wave) * 32 + li;
        const bool valid = comp < k;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float z = acc[t][q];
            if (valid && z == m[q]) cand[q] = comp;
            if (!PREDICT && valid && comp == yv[q]) zy_s[f32mm_row(q, h)] = z;
            const float ev = valid ? expf(z - m[q]) : 0.f;
            acc[t][q] = ev;
            sum[q] += ev;
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int oc = __shfl_xor(cand[q], o, 64);
            cand[q] = oc < cand[q] ? oc : cand[q];
            sum[q] += __shfl_xor(sum[q], o, 64);
        }
    if (li == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            red_i[wave][f32mm_row(q, h)] = cand[q];
            red_b[wave][f32mm_row(q, h)] = sum[q];
        }
    }
    __syncthreads();

    if (r) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = f32mm_row(q, h);
            sum[q] = ((red_b[0][row] + red_b[1][row]) + red_b[2][row]) + red_b[3][row];
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int comp = (t * 4 + wave) * 32 + li;
            const bool valid = comp < k;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const long long g = row0 + f32mm_row(q, h);
                const float p = acc[t][q] / sum[q];
                if (PREDICT) {
                    if (g < n && valid) r[(size_t)g * k + comp] = p;
                } else if (g < n && comp < kp) {
                    const float soft = sv[q] * p, hard = comp == yv[q] ? sv[q] : 0.f;
                    r[(size_t)g * kp + comp] = valid ? (yv[q] >= 0 ? hard : soft) : 0.f;
                }
            }
        }
    }
    if (tid < F32MM_RT) {
        const long long g = row0 + tid;
        if (g < n) {
            float mx = red_a[0][tid];
            int best = red_i[0][tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                mx = fmaxf(mx, red_a[w][tid]);
                best = red_i[w][tid] < best ? red_i[w][tid] : best;
            }
            if (best == 0x7fffffff) best = 0;                   // no component compares equal: a NaN row, counted below
            if (pred) pred[g] = best;
            if (bad_s[tid]) atomicAdd(&info[1], 1);
            const float sm = ((red_b[0][tid] + red_b[1][tid]) + red_b[2][tid]) + red_b[3][tid];
            const double lse = (double)mx + (double)logf(sm);
            if (PREDICT) {
                if (rowlse) rowlse[g] = (float)lse;
            } else {
                const float s = s_s[tid];
                rowll[g] = s == 0.f ? 0.0 : (double)s * (y_s[tid] >= 0 ? (double)zy_s[tid] : lse);
            }
        }
    }
}

// the hard M-step's responsibilities: one block per row.  r = s [comp == y] where 0 <= y < k, 0 elsewhere
__global__ void __launch_bounds__(256) gmm_hard_kernel(const int* __restrict__ y, const float* __restrict__ sw, int k, int kp, float* __restrict__ r,
                                                       int* __restrict__ info) {
    const long long g = blockIdx.x;
    const int yy = y[g];
    const float s = sw ? sw[g] : 1.f;
    if (threadIdx.x == 0 && yy >= k) atomicAdd(&info[0], 1);
    for (int comp = threadIdx.x; comp < kp; comp += 256) r[(size_t)g * kp + comp] = (yy >= 0 && yy < k && comp == yy) ? s : 0.f;
}

// ------------------------------------------------------------------------------------------------ 3. moment partials, nk and ll partials
// grid (component tiles * dim tiles, R, 2).  part [2, R, k, d] float64: z = 0 is r^T X, z = 1 is r^T (X o X), x squared in float32 as it
// is staged.
__global__ void __launch_bounds__(F32MM_THREADS) gmm_moment_kernel(const float* __restrict__ r, const float* __restrict__ X, long long n, int d, int k,
                                                                int kp, int ctiles, long long rows_per_range, double* __restrict__ part) {
    __shared__ float rs[F32MM_GK * F32MM_GLD];
    __shared__ float xs[F32MM_GK * F32MM_GLD];
    const int c0 = (blockIdx.x % ctiles) * F32MM_GT, d0 = (blockIdx.x / ctiles) * F32MM_GT;
    const bool sq = blockIdx.z != 0;
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    bool on[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) on[i][j] = c0 + wm * 64 + i * 32 < kp && d0 + wn * 64 + j * 32 < d;

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

    // no branch around a load: the next 32 rows are in registers while the MFMAs run (addresses clamped, values masked)
    float rr[F32MM_GK * F32MM_GT / F32MM_THREADS], xr[F32MM_GK * F32MM_GT / F32MM_THREADS];
    auto load_rows = [&](long long base) {
#pragma unroll
        for (int i = 0; i < F32MM_GK * F32MM_GT / F32MM_THREADS; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx >> 7, col = idx & 127;
            const long long g = base + row < hi ? base + row : hi - 1;
            rr[i] = r[(size_t)g * kp + (c0 + col < kp ? c0 + col : kp - 1)];
            xr[i] = X[(size_t)g * d + (d0 + col < d ? d0 + col : d - 1)];
        }
    };
    load_rows(lo);
    for (long long base = lo; base < hi; base += F32MM_GK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < F32MM_GK * F32MM_GT / F32MM_THREADS; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx >> 7, col = idx & 127;
            const bool in = base + row < hi;
            const float xv = sq ? xr[i] * xr[i] : xr[i];
            rs[row * F32MM_GLD + col] = (in && c0 + col < kp) ? rr[i] : 0.f;
            xs[row * F32MM_GLD + col] = (in && d0 + col < d) ? xv : 0.f;
        }
        __syncthreads();
        load_rows(base + F32MM_GK);
#pragma unroll 4
        for (int s = 0; s < F32MM_GK / 2; ++s) {
            const int kk = 2 * s + h;
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                av[i] = rs[kk * F32MM_GLD + wm * 64 + i * 32 + li];
                bv[i] = xs[kk * F32MM_GLD + wn * 64 + i * 32 + li];
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
    double* out = part + (size_t)blockIdx.z * gridDim.y * k * d + (size_t)blockIdx.y * k * d;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int comp = c0 + wm * 64 + i * 32 + f32mm_row(q, h), dim = d0 + wn * 64 + j * 32 + li;
                if (comp < k && dim < d) out[(size_t)comp * d + dim] = acc64[i][j][q];
            }
}

// grid (kp / 32, RB): float64 column sums of r over a row range -> nkpart [RB, kp]; the blocks of column group 0 also sum the range's
// row log-likelihoods -> llpart [RB]
__global__ void __launch_bounds__(F32MM_THREADS) gmm_nk_kernel(const float* __restrict__ r, const double* __restrict__ rowll, long long n, int kp,
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
__global__ void __launch_bounds__(256) gmm_finish_kernel(const double* __restrict__ part, const double* __restrict__ nkpart,
                                                         const double* __restrict__ llpart, int k, int d, int kp, int R, int RB,
                                                         double* __restrict__ s1, double* __restrict__ s2, double* __restrict__ nk,
                                                         double* __restrict__ ll) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long kd = (long long)k * d;
    if (e < 2 * kd) {
        const bool first = e < kd;
        const long long el = first ? e : e - kd;
        double* dst = first ? s1 : s2;
        dst[el] = f32mm_range_sum(first ? part : part + (size_t)R * kd, kd, el, R);
    } else if (e < 2 * kd + k) {
        const int comp = (int)(e - 2 * kd);
        nk[comp] = f32mm_range_sum(nkpart, kp, comp, RB);
    } else if (e == 2 * kd + k) {
        ll[0] = f32mm_range_sum(llpart, 1, 0, RB);
    }
}

struct gmm_plan {
    int kp, dp, ctiles, dtiles, R, RB;
    long long rows_per_range, nk_rows;
    size_t bcp, r, rowll, part, nkpart, llpart, end;
};

static void gmm_layout(int64_t n, int d, int k, gmm_plan& p) {
    p.kp = f32mm_pad(k, 32);
    p.dp = f32mm_pad(d, 8);
    p.ctiles = (int)scd_cdiv(p.kp, F32MM_GT);
    p.dtiles = (int)scd_cdiv(d, F32MM_GT);
    f32mm_ranges(n, (long long)p.ctiles * p.dtiles, 512, p.R, p.rows_per_range);    // 512: about 1024 blocks over the two moments
    f32mm_colsum_ranges(n, p.RB, p.nk_rows);
    p.bcp = 0;                                                                      // BCp    f32 [kp, 2 dp]
    p.r = p.bcp + scd_align((size_t)p.kp * 2 * p.dp * 4);                           // r      f32 [n, kp]
    p.rowll = p.r + scd_align((size_t)n * p.kp * 4);                                // rowll  f64 [n]
    p.part = p.rowll + scd_align((size_t)n * 8);                                    // part   f64 [2, R, k, d]
    p.nkpart = p.part + scd_align((size_t)2 * p.R * k * d * 8);                     // nkpart f64 [RB, kp]
    p.llpart = p.nkpart + scd_align((size_t)p.RB * p.kp * 8);                       // llpart f64 [RB]
    p.end = p.llpart + scd_align((size_t)p.RB * 8);
}

extern "C" int scd_gmm_row_tile(void) { return F32MM_RT; }
extern "C" int scd_gmm_chain_rows(void) { return F32MM_CHAIN; }

extern "C" size_t scd_gmm_ws_bytes(int64_t n, int d, int k) {
    if (!f32mm_shape_ok(n, d, k, 1)) return 0;
    gmm_plan p;
    gmm_layout(n, d, k, p);
    return p.end;
}

#define GMM_SHAPE_REQUIRE(who)              \
    F32MM_ND_REQUIRE(who, n, d);            \
    F32MM_WIDTH_REQUIRE(who, "k", k, 1);    \
    F32MM_WS_REQUIRE(who, ws)

extern "C" int scd_gmm_em_step(scd_handle h, const float* X, const int32_t* y, const float* sample_weight, int64_t n, int d, int k,
                               const float* a, const float* B, const float* C, double* ll_out, double* nk_out, double* s1_out,
                               double* s2_out, int32_t* pred_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_gmm_em_step");
    SCD_REQUIRE(X && ll_out && nk_out && s1_out && s2_out && info_out && ws, "scd_gmm_em_step: null argument");
    const bool hard = !a && !B && !C;
    SCD_REQUIRE(hard || (a && B && C), "scd_gmm_em_step: a, B and C must be all given or all NULL");
    SCD_REQUIRE(!hard || y, "scd_gmm_em_step: the hard M-step (a == B == C == NULL) needs labels");
    GMM_SHAPE_REQUIRE("scd_gmm_em_step");
    gmm_plan p;
    gmm_layout(n, d, k, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_gmm_em_step: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    float* BCp = (float*)(w + p.bcp);
    float* r = (float*)(w + p.r);
    double* rowll = (double*)(w + p.rowll);
    double* part = (double*)(w + p.part);
    double* nkpart = (double*)(w + p.nkpart);
    double* llpart = (double*)(w + p.llpart);

    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    if (hard) {
        SCD_HIP(hipMemsetAsync(rowll, 0, (size_t)n * 8, st));
        gmm_hard_kernel<<<(unsigned)n, 256, 0, st>>>(y, sample_weight, k, p.kp, r, info_out);
    } else {
        gmm_pack_kernel<<<(unsigned)scd_cdiv((int64_t)p.kp * 2 * p.dp, 256), 256, 0, st>>>(B, C, k, d, p.kp, p.dp, BCp);
        f32mm_fwd_dispatch(n, p.kp, [&](unsigned grid, auto nt) {
            gmm_fwd_kernel<decltype(nt)::value, false><<<grid, F32MM_THREADS, 0, st>>>(X, y, sample_weight, n, d, p.dp, k, p.kp, BCp, a, r, rowll,
                                                                                       nullptr, pred_out, info_out);
        });
    }
    gmm_moment_kernel<<<dim3((unsigned)(p.ctiles * p.dtiles), (unsigned)p.R, 2), F32MM_THREADS, 0, st>>>(r, X, n, d, k, p.kp, p.ctiles,
                                                                                                        p.rows_per_range, part);
    gmm_nk_kernel<<<dim3((unsigned)(p.kp / 32), (unsigned)p.RB), F32MM_THREADS, 0, st>>>(r, rowll, n, p.kp, p.nk_rows, nkpart, llpart);
    gmm_finish_kernel<<<(unsigned)scd_cdiv((int64_t)2 * k * d + k + 1, 256), 256, 0, st>>>(part, nkpart, llpart, k, d, p.kp, p.R, p.RB, s1_out,
                                                                                          s2_out, nk_out, ll_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_gmm_predict(scd_handle h, const float* X, int64_t n, int d, int k, const float* a, const float* B, const float* C,
                               int32_t* pred_out, float* row_ll_out, float* resp_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_gmm_predict");
    SCD_REQUIRE(X && a && B && C && ws, "scd_gmm_predict: null argument");
    GMM_SHAPE_REQUIRE("scd_gmm_predict");
    gmm_plan p;
    gmm_layout(1, d, k, p);                                     // only the packed B and C are needed
    SCD_REQUIRE(ws_bytes >= p.end, "scd_gmm_predict: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    float* BCp = (float*)((char*)ws + p.bcp);
    int* info = (int*)((char*)ws + p.r);                        // the two counters of the forward kernel: not reported
    SCD_HIP(hipMemsetAsync(info, 0, 8, st));
    gmm_pack_kernel<<<(unsigned)scd_cdiv((int64_t)p.kp * 2 * p.dp, 256), 256, 0, st>>>(B, C, k, d, p.kp, p.dp, BCp);
    f32mm_fwd_dispatch(n, p.kp, [&](unsigned grid, auto nt) {
        gmm_fwd_kernel<decltype(nt)::value, true><<<grid, F32MM_THREADS, 0, st>>>(X, nullptr, nullptr, n, d, p.dp, k, p.kp, BCp, a, resp_out, nullptr,
                                                                                  row_ll_out, pred_out, info);
    });
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
