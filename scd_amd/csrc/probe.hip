// The linear probe's evaluation on gfx950: the data term of multinomial logistic regression on frozen features and its gradient
// (the linear evaluation of DINO / DINOv2, scikit-learn's LogisticRegression(C) as a sum).  docs/design/probe.md has the semantics, the
// error model and the resources.
// The tile shapes, the k-octet packing, the float64 range sums and the host's range plan are f32mm.h's, shared with gmm.hip and pca.hip.
//
//   scd_probe_loss_grad   loss = sum_i s_i [lse_c(z_ic) - z_{i,y_i}],  gW = r^T X,  gb = column sums of r,  z_ic = W_c . x_i + b_c,
//                         r_ic = s_i (softmax(z_i)_c - [c == y_i]), in four steps:
//                           1. probe_pack_kernel: W [c, d] -> Wp [cp, dp] (cp = c up to 32, dp = d up to 8, zero filled), the 8 values of
//                              a k-octet stored as k+0, k+2, k+4, k+6, k+1, k+3, k+5, k+7: lane half h of the MFMA reads its four k
//                              values (k + 2 j + h) of an octet with one 16-byte load;
//                           2. probe_fwd_kernel: a block owns F32MM_RT = 32 rows and all cp classes, wave w the 32-class tiles w, w + 4, ...
//                              in up to 8 accumulator tiles of v_mfma_f32_32x32x2_f32 (128 accumulator registers at c = 1024).  X goes through LDS in
//                              chunks of 64 k, Wp streams from L2.  The sum over k ascends from a zero accumulator (the MFMA is a
//                              k-ordered fmaf chain), b_c is added last.  The softmax stays in registers: row maximum over the real
//                              classes (by index), e = expf(z - max), row sum, r = fmaf(s, e / sum, -s [c == y]) -> r [n, cp] fp32
//                              (padding columns 0), row loss s (max + logf(sum) - z_y) -> fp32 [n], argmax = the lowest class that
//                              attains the maximum.  The 32 lanes of a half reduce with shuffles, the four waves through LDS in wave
//                              order;
//                           3. probe_grad_kernel: 128 x 128 tiles of (class, dim) times R row ranges; r and X rows go through LDS 32 at
//                              a time, the float32 MFMA runs over chains of at most F32MM_CHAIN = 256 rows, each chain's tile is added
//                              into float64 registers; a range's float64 tile -> part [R, c, d].  probe_gb_kernel: float64 column sums
//                              of r and float64 sums of the row losses over RB row ranges;
//                           4. probe_finish_kernel: the ranges' partials added in ascending order -> loss, gW, gb (float64).
//   scd_probe_predict     steps 1 and 2 without the softmax: argmax and the two largest logits of each row.
//
// No floating-point atomics (the two info counters are integers).  R, RB and every tile depend on (n, d, c) alone: two calls return the
// same bits on any device.
#include "f32mm.h"

// ------------------------------------------------------------------------------------------------ 1. pack W
__global__ void __launch_bounds__(256) probe_pack_kernel(const float* __restrict__ W, int c, int d, int cp, int dp, float* __restrict__ Wp) {
    const float* const src[1] = {W};
    f32mm_pack<1>(src, c, d, cp, dp, Wp);
}

// ------------------------------------------------------------------------------------------------ 2. logits and softmax residual
template <int NT, bool PREDICT>
__global__ void __launch_bounds__(F32MM_THREADS) probe_fwd_kernel(const float* __restrict__ X, const int* __restrict__ y, const float* __restrict__ sw,
                                                               long long n, int d, int dp, int c, int cp, const float* __restrict__ Wp,
                                                               const float* __restrict__ b, float* __restrict__ r, float* __restrict__ rowloss,
                                                               int* __restrict__ pred, float* __restrict__ top2, int* __restrict__ info) {
    __shared__ float xs[F32MM_RT * F32MM_XLD];
    __shared__ float red_a[4][F32MM_RT];        // per wave: row maximum (PREDICT: largest logit)
    __shared__ float red_b[4][F32MM_RT];        // per wave: row sum of e (PREDICT: second largest logit)
    __shared__ int red_i[4][F32MM_RT];          // per wave: lowest class at the maximum
    __shared__ float zy_s[F32MM_RT], s_s[F32MM_RT];
    __shared__ int y_s[F32MM_RT], bad_s[F32MM_RT];
    const long long row0 = (long long)blockIdx.x * F32MM_RT;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;

    if (tid < F32MM_RT) {
        const long long g = row0 + tid;
        int yy = -1;
        float s = 0.f;
        if (!PREDICT && g < n) {
            yy = y[g];
            s = sw ? sw[g] : 1.f;
            if (yy < 0 || yy >= c) {
                atomicAdd(&info[0], 1);
                yy = -1;
                s = 0.f;
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
        const int cls = (t * 4 + wave) * 32 + li;
        woff[t] = (cls < cp ? cls : cp - 1) * dp + 4 * h;       // a tile past cp repeats the last row: computed, never used
    }

    // no branch around a load: the chunk after the current one is in registers while the MFMAs run (addresses clamped, values masked)
    float xr[F32MM_RT * F32MM_BK / F32MM_THREADS];
    f32x4 bw[NT], bn[NT];
    auto load_x = [&](int k0) {
#pragma unroll
        for (int i = 0; i < F32MM_RT * F32MM_BK / F32MM_THREADS; ++i) {
            const int idx = tid + F32MM_THREADS * i, row = idx >> 6, k = k0 + (idx & 63);
            const long long g = row0 + row < n ? row0 + row : n - 1;
            xr[i] = X[(size_t)g * d + (k < d ? k : d - 1)];
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
            xs[row * F32MM_XLD + kk] = (row0 + row < n && k0 + kk < d) ? xr[i] : 0.f;
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

    // acc[t][q] = z of row f32mm_row(q, h), class (4 t + wave) * 32 + li, without b
    float m[16], m2[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) m[q] = m2[q] = -INFINITY;
    int bad = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        {
            const int cls = (t * 4 + wave) * 32 + li;
            const bool valid = cls < c;
            const float bb = (b && valid) ? b[cls] : 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float z = acc[t][q] + bb;
                acc[t][q] = z;
                if (valid) {
                    if (!(fabsf(z) < INFINITY)) bad |= 1 << q;
                    if (PREDICT) {
                        if (z > m[q]) {
                            m2[q] = m[q];
                            m[q] = z;
                        } else if (z > m2[q]) {
                            m2[q] = z;
                        }
                    } else {
                        m[q] = fmaxf(m[q], z);
                    }
                }
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
        for (int q = 0; q < 16; ++q) {
            const float o1 = __shfl_xor(m[q], o, 64);
            if (PREDICT) {
                const float o2 = __shfl_xor(m2[q], o, 64);
                m2[q] = fmaxf(fminf(m[q], o1), fmaxf(m2[q], o2));
            }
            m[q] = fmaxf(m[q], o1);
        }
    if (li == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            red_a[wave][f32mm_row(q, h)] = m[q];
            if (PREDICT) red_b[wave][f32mm_row(q, h)] = m2[q];
        }
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

    // the lowest class at the maximum; e and its row sum; the label's logit
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
    for (int t = NT - 1; t >= 0; --t) {                         // descending: the lowest class is kept last
        {
            const int cls = (t * 4 + wave) * 32 + li;
            const bool valid = cls < c;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float z = acc[t][q];
                if (valid && z == m[q]) cand[q] = cls;
                if (!PREDICT) {
                    if (valid && cls == yv[q]) zy_s[f32mm_row(q, h)] = z;
                    const float ev = valid ? expf(z - m[q]) : 0.f;
                    acc[t][q] = ev;
                    sum[q] += ev;
                }
            }
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int oc = __shfl_xor(cand[q], o, 64);
            cand[q] = oc < cand[q] ? oc : cand[q];
            if (!PREDICT) sum[q] += __shfl_xor(sum[q], o, 64);
        }
    if (li == 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            red_i[wave][f32mm_row(q, h)] = cand[q];
            if (!PREDICT) red_b[wave][f32mm_row(q, h)] = sum[q];
        }
    }
    __syncthreads();

    if (!PREDICT) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = f32mm_row(q, h);
            sum[q] = ((red_b[0][row] + red_b[1][row]) + red_b[2][row]) + red_b[3][row];
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            {
                const int cls = (t * 4 + wave) * 32 + li;
                const bool valid = cls < c;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = f32mm_row(q, h);
                    const long long g = row0 + row;
                    if (g < n && cls < cp) {
                        const float p = acc[t][q] / sum[q];
                        r[(size_t)g * cp + cls] = valid ? fmaf(sv[q], p, cls == yv[q] ? -sv[q] : 0.f) : 0.f;
                    }
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
            if (best == 0x7fffffff) best = 0;                   // no class compares equal: a NaN row, counted below
            if (pred) pred[g] = best;
            if (bad_s[tid]) atomicAdd(&info[1], 1);
            if (PREDICT) {
                if (top2) {
                    float t1 = red_a[0][tid], t2 = red_b[0][tid];
#pragma unroll
                    for (int w = 1; w < 4; ++w) {
                        const float o1 = red_a[w][tid], o2 = red_b[w][tid];
                        t2 = fmaxf(fminf(t1, o1), fmaxf(t2, o2));
                        t1 = fmaxf(t1, o1);
                    }
                    top2[(size_t)g * 2] = t1;
                    top2[(size_t)g * 2 + 1] = t2;
                }
            } else {
                const float sm = ((red_b[0][tid] + red_b[1][tid]) + red_b[2][tid]) + red_b[3][tid];
                const float s = s_s[tid];
                const double l = (double)mx + (double)logf(sm) - (double)zy_s[tid];
                rowloss[g] = s == 0.f ? 0.f : (float)((double)s * l);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ 3. gW partials, gb and loss partials
// grid (class tiles * dim tiles, R).  part [R, c, d] float64.
__global__ void __launch_bounds__(F32MM_THREADS) probe_grad_kernel(const float* __restrict__ r, const float* __restrict__ X, long long n, int d, int c,
                                                                int cp, int ctiles, long long rows_per_range, double* __restrict__ part) {
    __shared__ float rs[F32MM_GK * F32MM_GLD];
    __shared__ float xs[F32MM_GK * F32MM_GLD];
    const int c0 = (blockIdx.x % ctiles) * F32MM_GT, d0 = (blockIdx.x / ctiles) * F32MM_GT;
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, li = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    bool on[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) on[i][j] = c0 + wm * 64 + i * 32 < cp && d0 + wn * 64 + j * 32 < d;

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
            rr[i] = r[(size_t)g * cp + (c0 + col < cp ? c0 + col : cp - 1)];
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
            rs[row * F32MM_GLD + col] = (in && c0 + col < cp) ? rr[i] : 0.f;
            xs[row * F32MM_GLD + col] = (in && d0 + col < d) ? xr[i] : 0.f;
        }
        __syncthreads();
        load_rows(base + F32MM_GK);
#pragma unroll 4
        for (int s = 0; s < F32MM_GK / 2; ++s) {
            const int k = 2 * s + h;
            float a[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = rs[k * F32MM_GLD + wm * 64 + i * 32 + li];
                bv[i] = xs[k * F32MM_GLD + wn * 64 + i * 32 + li];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (on[i][j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv[j], acc[i][j], 0, 0, 0);
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
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int cls = c0 + wm * 64 + i * 32 + f32mm_row(q, h), dim = d0 + wn * 64 + j * 32 + li;
                if (cls < c && dim < d) part[((size_t)blockIdx.y * c + cls) * d + dim] = acc64[i][j][q];
            }
}

// grid (cp / 32, RB): float64 column sums of r over a row range -> gbpart [RB, cp]; the blocks of column group 0 also sum the range's
// row losses -> losspart [RB]
__global__ void __launch_bounds__(F32MM_THREADS) probe_gb_kernel(const float* __restrict__ r, const float* __restrict__ rowloss, long long n, int cp,
                                                                 long long rows_per_range, double* __restrict__ gbpart,
                                                                 double* __restrict__ losspart) {
    __shared__ double sh[F32MM_THREADS];
    long long lo, hi;
    f32mm_range(rows_per_range, n, lo, hi);
    const int tid = threadIdx.x, cls = blockIdx.x * 32 + (tid & 31);
    const double t = f32mm_colsum(lo, hi, [&](long long g) { return r[(size_t)g * cp + cls]; }, sh);
    if (tid < 32) gbpart[(size_t)blockIdx.y * cp + cls] = t;
    if (blockIdx.x != 0) return;
    const double l = f32mm_rowsum(rowloss, lo, hi, sh);
    if (tid == 0) losspart[blockIdx.y] = l;
}

// ------------------------------------------------------------------------------------------------ 4. the ranges in ascending order
__global__ void __launch_bounds__(256) probe_finish_kernel(const double* __restrict__ part, const double* __restrict__ gbpart,
                                                           const double* __restrict__ losspart, int c, int d, int cp, int R, int RB,
                                                           double* __restrict__ gW, double* __restrict__ gb, double* __restrict__ loss) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long cd = (long long)c * d;
    if (e < cd) {
        gW[e] = f32mm_range_sum(part, cd, e, R);
    } else if (e < cd + c) {
        const int cls = (int)(e - cd);
        if (gb) gb[cls] = f32mm_range_sum(gbpart, cp, cls, RB);
    } else if (e == cd + c) {
        loss[0] = f32mm_range_sum(losspart, 1, 0, RB);
    }
}

struct probe_plan {
    int cp, dp, ctiles, dtiles, R, RB;
    long long rows_per_range, gb_rows;
    size_t wp, r, rowloss, part, gbpart, losspart, end;
};

static void probe_layout(int64_t n, int d, int c, probe_plan& p) {
    p.cp = f32mm_pad(c, 32);
    p.dp = f32mm_pad(d, 8);
    p.ctiles = (int)scd_cdiv(p.cp, F32MM_GT);
    p.dtiles = (int)scd_cdiv(d, F32MM_GT);
    f32mm_ranges(n, (long long)p.ctiles * p.dtiles, 1024, p.R, p.rows_per_range);
    f32mm_colsum_ranges(n, p.RB, p.gb_rows);
    p.wp = 0;                                                                       // Wp       f32 [cp, dp]
    p.r = p.wp + scd_align((size_t)p.cp * p.dp * 4);                                // r        f32 [n, cp]
    p.rowloss = p.r + scd_align((size_t)n * p.cp * 4);                              // rowloss  f32 [n]
    p.part = p.rowloss + scd_align((size_t)n * 4);                                  // part     f64 [R, c, d]
    p.gbpart = p.part + scd_align((size_t)p.R * c * d * 8);                         // gbpart   f64 [RB, cp]
    p.losspart = p.gbpart + scd_align((size_t)p.RB * p.cp * 8);                     // losspart f64 [RB]
    p.end = p.losspart + scd_align((size_t)p.RB * 8);
}

extern "C" int scd_probe_row_tile(void) { return F32MM_RT; }
extern "C" int scd_probe_chain_rows(void) { return F32MM_CHAIN; }

extern "C" size_t scd_probe_ws_bytes(int64_t n, int d, int c) {
    if (!f32mm_shape_ok(n, d, c, 2)) return 0;
    probe_plan p;
    probe_layout(n, d, c, p);
    return p.end;
}

#define PROBE_SHAPE_REQUIRE(who)            \
    F32MM_ND_REQUIRE(who, n, d);            \
    F32MM_WIDTH_REQUIRE(who, "c", c, 2);    \
    F32MM_WS_REQUIRE(who, ws)

extern "C" int scd_probe_loss_grad(scd_handle h, const float* X, const int32_t* y, const float* sample_weight, int64_t n, int d, int c,
                                   const float* W, const float* b, double* loss_out, double* gW_out, double* gb_out, int32_t* pred_out,
                                   int32_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_probe_loss_grad");
    SCD_REQUIRE(X && y && W && loss_out && gW_out && info_out && ws, "scd_probe_loss_grad: null argument");
    PROBE_SHAPE_REQUIRE("scd_probe_loss_grad");
    probe_plan p;
    probe_layout(n, d, c, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_probe_loss_grad: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    float* Wp = (float*)(w + p.wp);
    float* r = (float*)(w + p.r);
    float* rowloss = (float*)(w + p.rowloss);
    double* part = (double*)(w + p.part);
    double* gbpart = (double*)(w + p.gbpart);
    double* losspart = (double*)(w + p.losspart);

    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    probe_pack_kernel<<<(unsigned)scd_cdiv((int64_t)p.cp * p.dp, 256), 256, 0, st>>>(W, c, d, p.cp, p.dp, Wp);
    f32mm_fwd_dispatch(n, p.cp, [&](unsigned grid, auto nt) {
        probe_fwd_kernel<decltype(nt)::value, false><<<grid, F32MM_THREADS, 0, st>>>(X, y, sample_weight, n, d, p.dp, c, p.cp, Wp, b, r, rowloss,
                                                                                     pred_out, nullptr, info_out);
    });
    probe_grad_kernel<<<dim3((unsigned)(p.ctiles * p.dtiles), (unsigned)p.R), F32MM_THREADS, 0, st>>>(r, X, n, d, c, p.cp, p.ctiles,
                                                                                                     p.rows_per_range, part);
    probe_gb_kernel<<<dim3((unsigned)(p.cp / 32), (unsigned)p.RB), F32MM_THREADS, 0, st>>>(r, rowloss, n, p.cp, p.gb_rows, gbpart, losspart);
    probe_finish_kernel<<<(unsigned)scd_cdiv((int64_t)c * d + c + 1, 256), 256, 0, st>>>(part, gbpart, losspart, c, d, p.cp, p.R, p.RB, gW_out,
                                                                                         gb_out, loss_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

extern "C" int scd_probe_predict(scd_handle h, const float* X, int64_t n, int d, int c, const float* W, const float* b, int32_t* pred_out,
                                 float* top_logit_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_probe_predict");
    SCD_REQUIRE(X && W && pred_out && ws, "scd_probe_predict: null argument");
    PROBE_SHAPE_REQUIRE("scd_probe_predict");
    probe_plan p;
    probe_layout(1, d, c, p);                                   // only the packed W is needed
    SCD_REQUIRE(ws_bytes >= p.end, "scd_probe_predict: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    float* Wp = (float*)((char*)ws + p.wp);
    int* info = (int*)((char*)ws + p.r);                        // the two counters of the forward kernel: not reported
    SCD_HIP(hipMemsetAsync(info, 0, 8, st));
    probe_pack_kernel<<<(unsigned)scd_cdiv((int64_t)p.cp * p.dp, 256), 256, 0, st>>>(W, c, d, p.cp, p.dp, Wp);
    f32mm_fwd_dispatch(n, p.cp, [&](unsigned grid, auto nt) {
        probe_fwd_kernel<decltype(nt)::value, true><<<grid, F32MM_THREADS, 0, st>>>(X, nullptr, nullptr, n, d, p.dp, c, p.cp, Wp, b, nullptr, nullptr,
                                                                                    pred_out, top_logit_out, info);
    });
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
