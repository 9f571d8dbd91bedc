// Silhouette coefficients on gfx950: sklearn.metrics.silhouette_samples(X, labels, metric='euclidean') and its mean, for the
// label-free search of the number of categories (docs/design/estimate_k.md, "Without labels").  O(n^2 d): one n x n x d fp16 MFMA pass
// whose epilogue turns dots into distances and folds them into per-cluster row sums in registers; no n x n and no n x k matrix
// reaches memory.
//
// For row i with cluster c(i) of cnt rows:  a = sum_{j in c(i)} dist(i, j) / (cnt - 1)  (the pair j = i contributes exactly 0),
// b = min over the other NON-EMPTY clusters c of sum_{j in c} dist(i, j) / cnt_c,  s = (b - a) / max(a, b);  s = 0 for a row in a
// singleton cluster and when max(a, b) = 0.  Label ids without rows are skipped (what scikit-learn's label encoding does).  A row whose
// label lies outside [0, k) is counted in info_out[0], takes part in nothing and gets s = 0.  With fewer than two non-empty clusters
// every s and the mean are 0.
//
// Arithmetic:
//   * rows are used as fp16: fp32 input is rounded to nearest even (the identity for features an fp16 tower wrote);
//   * dots are accumulated in fp32 by v_mfma_f32_16x16x32_f16;
//   * dist^2 = max(0, |x_i|^2 + |x_j|^2 - 2 dot), the norms those of the fp16 rows, summed in fp32; dist = sqrtf (correctly rounded);
//   * the pair i = j and the columns outside a cluster's segment are excluded BY INDEX, not left to cancellation;
//   * per-cluster sums, the means and s are fp32; the mean over n is float64 over a fixed strided partition (row i belongs to thread
//     i mod SL_FIN_BLOCKS * SL_FIN_THREADS) and fixed trees - the scd_contingency_stats convention;
//   * no floating-point atomics anywhere, and the summation order of every row depends on the labels alone (not on the grid): two
//     calls on one input give the same bits in samples_out and mean_out.
//
// Three steps, all buffers in the caller's workspace:
//   1. prep: a stable counting sort of the rows by label (sl_rank_kernel: rank inside a 1,024-row chunk and the chunk's count per
//      label; sl_scan_kernel: exclusive scan of the [k][chunks] counts; sl_offsets_kernel: segment offsets [k + 1]), then
//      sl_gather_kernel writes the sorted fp16 copy [n_alloc][ld] (ld = d rounded up to 64, zero-filled; rows past the last valid one
//      zero), its fp32 norms and each sorted row's label;
//   2. sl_main_kernel: a block owns a panel of SL_BM = 128 sorted rows (4 waves x 32 rows) and walks the clusters of its range
//      (grid.y splits the sorted rows into ranges; a cluster belongs to the range its first row falls in) in order.  Per cluster it
//      walks column tiles of SL_BN = 128 columns that START AT THE SEGMENT'S FIRST ROW; of a tile only the 16-column MFMA sub-tiles
//      that intersect the segment are loaded and multiplied, so a cluster of cnt rows costs ceil(cnt / 16) * 16 columns of MFMA work:
//      at most 15 masked columns per cluster, 7.5 on average (6 % at the 127 rows per cluster of K = 1,000 on 126,976 rows).  The
//      reduction dimension runs in chunks of 64 through a two-buffer LDS ring filled from registers (the next chunk's global loads are
//      issued before the current chunk's MFMAs).
//      Every lane keeps its 8 rows' partial sums across the cluster's tiles; the 16 lanes that share a row are reduced once per
//      cluster, then the own-cluster sum or the running minimum of the means is updated in registers.  Each (panel, range) block
//      writes its rows' minimum; the one block whose range holds a row's own cluster writes its a-sum;
//   3. sl_finish_kernel / sl_mean_kernel: minimum over the ranges, s in the ORIGINAL row order, the float64 mean.
#include "common.h"

#define SL_BM 128
#define SL_BN 128
#define SL_BK 64
#define SL_LDK 72                               // LDS row stride in halfs: 144 bytes, so the 16 rows of a fragment read spread over the banks
#define SL_THREADS 256
#define SL_SORT 1024                            // rows per chunk of the counting sort
#define SL_YMAX 32                              // most cluster ranges (grid.y)
#define SL_LDS_BYTES (2 * (SL_BM + SL_BN) * SL_LDK * 2)
#define SL_FIN_THREADS 256
#define SL_FIN_BLOCKS 64
#define SL_DP_MAX 1024

// ------------------------------------------------------------------------------------------------ prep: stable counting sort
// rowpos[i] <- the number of earlier rows of i's chunk with i's label (-1: label outside [0, k)); hist[label][chunk] <- the chunk's count
// (written by the label's last row in the chunk; hist is zero on entry)
__global__ void __launch_bounds__(SL_SORT) sl_rank_kernel(const int* __restrict__ labels, long long n, int k, long long chunks,
                                                          int* __restrict__ rowpos, unsigned* __restrict__ hist) {
    __shared__ int lab[SL_SORT];
    const int t = threadIdx.x;
    const long long i = (long long)blockIdx.x * SL_SORT + t;
    int l = -1;
    if (i < n) {
        l = labels[i];
        if ((unsigned)l >= (unsigned)k) l = -1;
    }
    lab[t] = l;
    __syncthreads();
    if (i >= n) return;
    if (l < 0) {
        rowpos[i] = -1;
        return;
    }
    int before = 0, after = 0;
    for (int j = 0; j < SL_SORT; ++j) {
        const int same = lab[j] == l;
        before += same & (j < t);
        after += same & (j > t);
    }
    rowpos[i] = before;
    if (!after) hist[(size_t)l * chunks + blockIdx.x] = (unsigned)(before + 1);
}

// exclusive scan of hist[0 .. len) in place (one block; thread t owns a contiguous piece); meta[0] <- the total = the number of valid rows
__global__ void __launch_bounds__(SL_SORT) sl_scan_kernel(unsigned* __restrict__ hist, long long len, int* __restrict__ meta) {
    __shared__ unsigned sh[SL_SORT];
    const int t = threadIdx.x;
    const long long piece = (len + SL_SORT - 1) / SL_SORT;
    long long b0 = (long long)t * piece, b1 = b0 + piece;
    if (b0 > len) b0 = len;
    if (b1 > len) b1 = len;
    unsigned s = 0;
    for (long long q = b0; q < b1; ++q) s += hist[q];
    sh[t] = s;
    __syncthreads();
    for (int o = 1; o < SL_SORT; o <<= 1) {
        const unsigned v = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    unsigned run = sh[t] - s;
    for (long long q = b0; q < b1; ++q) {
        const unsigned v = hist[q];
        hist[q] = run;
        run += v;
    }
    if (t == SL_SORT - 1) meta[0] = (int)sh[SL_SORT - 1];
}

// off[c] = first sorted row of cluster c, off[k] = valid rows; info[0] = rows with a label outside [0, k), info[1] = non-empty clusters
// (info is zero on entry; integer adds only)
__global__ void __launch_bounds__(256) sl_offsets_kernel(const unsigned* __restrict__ hist, long long chunks, int k, const int* __restrict__ meta,
                                                         long long n, int* __restrict__ off, long long* __restrict__ info) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c > k) return;
    const int total = meta[0];
    const int o = c < k ? (int)hist[(size_t)c * chunks] : total;
    off[c] = o;
    if (c < k) {
        const int nx = c + 1 < k ? (int)hist[(size_t)(c + 1) * chunks] : total;
        if (nx > o) atomicAdd((unsigned long long*)&info[1], 1ull);
    }
    if (c == 0) info[0] = n - total;
}

// a wave per original row: its sorted position, the fp16 copy of the row (zero-filled to ld), its norm and label there; the waves after
// them: one per sorted slot, zeroing the slots past the last valid row
template <typename T>
__global__ void __launch_bounds__(256) sl_gather_kernel(const T* __restrict__ X, const int* __restrict__ labels, long long n, int d, int ld,
                                                        long long chunks, long long n_alloc, const unsigned* __restrict__ hist,
                                                        const int* __restrict__ meta, int* __restrict__ rowpos, half_t* __restrict__ Xs,
                                                        float* __restrict__ nrm, int* __restrict__ slab) {
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w < n) {
        const int r = rowpos[w];
        if (r < 0) return;
        const int l = labels[w];
        const long long pos = (long long)hist[(size_t)l * chunks + w / SL_SORT] + r;
        const T* src = X + (size_t)w * d;
        half_t* dst = Xs + (size_t)pos * ld;
        float s = 0.f;
        for (int c = lane; c < ld; c += 64) {
            const half_t hv = c < d ? (half_t)src[c] : (half_t)0.f;
            dst[c] = hv;
            const float f = (float)hv;
            s = fmaf(f, f, s);
        }
        s = wave_sum_f32(s);
        if (lane == 0) {
            rowpos[w] = (int)pos;
            nrm[pos] = s;
            slab[pos] = l;
        }
    } else {
        const long long q = w - n;
        if (q >= n_alloc || q < meta[0]) return;
        half_t* dst = Xs + (size_t)q * ld;
        for (int c = lane; c < ld; c += 64) dst[c] = (half_t)0.f;
        if (lane == 0) {
            nrm[q] = 0.f;
            slab[q] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------ main kernel
// first c in [0, k] with off[c] >= v (off is non-decreasing and off[k] >= v)
__device__ __forceinline__ int sl_lower_bound(const int* __restrict__ off, int k, int v) {
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(SL_THREADS) sl_main_kernel(const half_t* __restrict__ Xs, const float* __restrict__ nrm,
                                                             const int* __restrict__ slab, const int* __restrict__ off,
                                                             const int* __restrict__ meta, int k, int ld, int dp, long long n_alloc,
                                                             float* __restrict__ a_sum, float* __restrict__ part_b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sl_lds[];
    half_t* sA = reinterpret_cast<half_t*>(sl_lds);             // [2][SL_BM][SL_LDK]
    half_t* sB = sA + 2 * SL_BM * SL_LDK;                       // [2][SL_BN][SL_LDK]
    const int n_valid = meta[0];
    const int row0 = blockIdx.x * SL_BM;
    if (row0 >= n_valid) return;
    const int ny = gridDim.y, y = blockIdx.y;
    const int per = (n_valid + ny - 1) / ny;
    long long r_lo = (long long)y * per, r_hi = r_lo + per;
    if (r_lo > n_valid) r_lo = n_valid;
    if (r_hi > n_valid) r_hi = n_valid;
    const int c_lo = sl_lower_bound(off, k, (int)r_lo), c_hi = sl_lower_bound(off, k, (int)r_hi);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    int prow[2][4], own[2][4];
    float ni[2][4], asum[2][4], bmin[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
            prow[mt][r] = p;
            ni[mt][r] = nrm[p];
            own[mt][r] = slab[p];
            asum[mt][r] = 0.f;
            bmin[mt][r] = INFINITY;
        }
    const int nk = ld / SL_BK;
    const int lrow = tid >> 3, lk = (tid & 7) * 8;              // 16-byte vector tid + 256 i of a chunk: row lrow + 32 i, halfs lk .. lk + 7
    const half_t* gA = Xs + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * SL_LDK + lq * 8, b_frag = lr * SL_LDK + lq * 8, st_off = lrow * SL_LDK + lk;

    for (int c = c_lo; c < c_hi; ++c) {
        const int s0 = off[c], s1 = off[c + 1], cnt = s1 - s0;
        if (cnt <= 0) continue;
        float rs[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) rs[mt][r] = 0.f;
        for (int j0 = s0; j0 < s1; j0 += SL_BN) {
            const int ncol = (s1 - j0 < SL_BN) ? s1 - j0 : SL_BN;   // columns of this tile inside the segment
            const int nsub = (ncol + 15) >> 4;                      // 16-column sub-tiles that intersect it
            const half_t* gB = Xs + (size_t)(j0 + lrow) * ld + lk;
            f32x4 acc[2][8];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            half8 ra[4], rb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ra[i] = *reinterpret_cast<const half8*>(gA + (size_t)i * 32 * ld);
                if (i * 32 < ncol) rb[i] = *reinterpret_cast<const half8*>(gB + (size_t)i * 32 * ld);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<half8*>(sA + st_off + i * 32 * SL_LDK) = ra[i];
                if (i * 32 < ncol) *reinterpret_cast<half8*>(sB + st_off + i * 32 * SL_LDK) = rb[i];
            }
            __syncthreads();
            for (int kc = 0; kc < nk; ++kc) {
                const int cur = kc & 1;
                const bool more = kc + 1 < nk;
                if (more) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        ra[i] = *reinterpret_cast<const half8*>(gA + (size_t)i * 32 * ld + (kc + 1) * SL_BK);
                        if (i * 32 < ncol) rb[i] = *reinterpret_cast<const half8*>(gB + (size_t)i * 32 * ld + (kc + 1) * SL_BK);
                    }
                }
                const half_t* cA = sA + cur * (SL_BM * SL_LDK) + a_frag;
                const half_t* cB = sB + cur * (SL_BN * SL_LDK) + b_frag;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (kc * SL_BK + ks * 32 < dp) {
                        const half8 fa0 = *reinterpret_cast<const half8*>(cA + ks * 32);
                        const half8 fa1 = *reinterpret_cast<const half8*>(cA + 16 * SL_LDK + ks * 32);
#pragma unroll
                        for (int nt = 0; nt < 8; ++nt) {
                            if (nt < nsub) {
                                const half8 fb = *reinterpret_cast<const half8*>(cB + nt * 16 * SL_LDK + ks * 32);
                                acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa0, fb, acc[0][nt], 0, 0, 0);
                                acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1, fb, acc[1][nt], 0, 0, 0);
                            }
                        }
                    }
                }
                if (more) {
                    half_t* nA = sA + (cur ^ 1) * (SL_BM * SL_LDK) + st_off;
                    half_t* nB = sB + (cur ^ 1) * (SL_BN * SL_LDK) + st_off;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        *reinterpret_cast<half8*>(nA + i * 32 * SL_LDK) = ra[i];
                        if (i * 32 < ncol) *reinterpret_cast<half8*>(nB + i * 32 * SL_LDK) = rb[i];
                    }
                }
                __syncthreads();
            }
            // epilogue: distances of the tile's columns, folded into the lane's row sums
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) {
                if (nt < nsub) {
                    const int col = j0 + nt * 16 + lr;
                    const float nj = nrm[col];
                    const bool inside = col < s1;
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float d2 = fmaxf(0.f, fmaf(-2.f, acc[mt][nt][r], ni[mt][r] + nj));
                            float dist = sqrtf(d2);
                            if (!inside || col == prow[mt][r]) dist = 0.f;
                            rs[mt][r] += dist;
                        }
                }
            }
        }
        // end of the cluster: the 16 lanes that share a row, then the mean
        const float inv = (float)cnt;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = rs[mt][r];
                s += __shfl_xor(s, 1, 64);
                s += __shfl_xor(s, 2, 64);
                s += __shfl_xor(s, 4, 64);
                s += __shfl_xor(s, 8, 64);
                if (c == own[mt][r]) asum[mt][r] = s;
                else bmin[mt][r] = fminf(bmin[mt][r], s / inv);
            }
    }
    if (lr == 0) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = prow[mt][r];
                if (p < n_valid) {
                    if (own[mt][r] >= c_lo && own[mt][r] < c_hi) a_sum[p] = asum[mt][r];
                    part_b[(size_t)y * n_alloc + p] = bmin[mt][r];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------ finish
__device__ __forceinline__ double sl_tree_f64(double v, double* sh, int nthreads) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = nthreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ void __launch_bounds__(SL_FIN_THREADS) sl_finish_kernel(const int* __restrict__ labels, const int* __restrict__ rowpos,
                                                                   const int* __restrict__ off, const float* __restrict__ a_sum,
                                                                   const float* __restrict__ part_b, int ny, long long n_alloc, long long n,
                                                                   const long long* __restrict__ info, float* __restrict__ samples,
                                                                   double* __restrict__ part_d) {
    __shared__ double sh[SL_FIN_THREADS];
    const bool scored = info[1] >= 2;
    double sum = 0.0;
    for (long long i = (long long)blockIdx.x * SL_FIN_THREADS + threadIdx.x; i < n; i += (long long)SL_FIN_BLOCKS * SL_FIN_THREADS) {
        float s = 0.f;
        const int p = rowpos[i];
        if (scored && p >= 0) {
            const int c = labels[i];
            const int cnt = off[c + 1] - off[c];
            if (cnt > 1) {
                const float a = a_sum[p] / (float)(cnt - 1);
                float b = INFINITY;
                for (int y = 0; y < ny; ++y) b = fminf(b, part_b[(size_t)y * n_alloc + p]);
                const float m = fmaxf(a, b);
                s = m > 0.f ? (b - a) / m : 0.f;
            }
        }
        samples[i] = s;
        sum += (double)s;
    }
    sum = sl_tree_f64(sum, sh, SL_FIN_THREADS);
    if (threadIdx.x == 0) part_d[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(SL_FIN_BLOCKS) sl_mean_kernel(const double* __restrict__ part_d, long long n, double* __restrict__ mean_out) {
    __shared__ double sh[SL_FIN_BLOCKS];
    const double total = sl_tree_f64(part_d[threadIdx.x], sh, SL_FIN_BLOCKS);
    if (threadIdx.x == 0) mean_out[0] = total / (double)n;
}

// ------------------------------------------------------------------------------------------------ host
struct sl_plan {
    int ld, dp, ny_max;
    long long n_alloc, chunks;
    size_t xs, nrm, slab, rowpos, hist, off, meta, a_sum, part_b, part_d, end;
};

static void sl_layout(int64_t n, int d, int k, sl_plan& p) {
    p.dp = (int)scd_cdiv(d, 32) * 32;
    p.ld = (int)scd_cdiv(d, SL_BK) * SL_BK;
    p.n_alloc = scd_cdiv(n, SL_BM) * SL_BM + SL_BN;             // a panel's rows and a column tile's rows past the last valid row stay inside
    p.chunks = scd_cdiv(n, SL_SORT);
    p.ny_max = k < SL_YMAX ? k : SL_YMAX;
    p.xs = 0;                                                                       // Xs     f16   [n_alloc, ld]
    p.nrm = p.xs + scd_align((size_t)p.n_alloc * p.ld * 2);                        // nrm    f32   [n_alloc]
    p.slab = p.nrm + scd_align((size_t)p.n_alloc * 4);                             // slab   int32 [n_alloc]
    p.rowpos = p.slab + scd_align((size_t)p.n_alloc * 4);                          // rowpos int32 [n]
    p.hist = p.rowpos + scd_align((size_t)n * 4);                                  // hist   u32   [k, chunks]
    p.off = p.hist + scd_align((size_t)k * p.chunks * 4);                          // off    int32 [k + 1]
    p.meta = p.off + scd_align((size_t)(k + 1) * 4);                               // meta   int32 [4]
    p.a_sum = p.meta + scd_align(16);                                              // a_sum  f32   [n_alloc]
    p.part_b = p.a_sum + scd_align((size_t)p.n_alloc * 4);                         // part_b f32   [ny_max, n_alloc]
    p.part_d = p.part_b + scd_align((size_t)p.ny_max * p.n_alloc * 4);             // part_d f64   [SL_FIN_BLOCKS]
    p.end = p.part_d + scd_align((size_t)SL_FIN_BLOCKS * 8);
}

static bool sl_shape_ok(int64_t n, int d, int k) {
    return n >= 2 && n <= (1ll << 30) && d >= 1 && scd_cdiv(d, 32) * 32 <= SL_DP_MAX && k >= 2 && k <= n;
}

extern "C" size_t scd_silhouette_ws_bytes(int64_t n, int d, int k) {
    if (!sl_shape_ok(n, d, k)) return 0;
    sl_plan p;
    sl_layout(n, d, k, p);
    return p.end;
}

// ranges of clusters (grid.y of sl_main_kernel): enough blocks to fill the device a few times over when there are few panels.  The
// result does not depend on it: a row's a-sum comes from one block, and the minimum over the ranges is exact.
static int sl_ranges(int n_cu, int64_t n, int k) {
    const long long panels = scd_cdiv(n, SL_BM);
    long long ny = scd_cdiv(4ll * n_cu, panels);
    const int ny_max = k < SL_YMAX ? k : SL_YMAX;
    if (ny > ny_max) ny = ny_max;
    if (ny < 1) ny = 1;
    return (int)ny;
}

extern "C" int scd_silhouette_ranges(scd_handle h, int64_t n, int k) {
    if (!h || !sl_shape_ok(n, 1, k)) return 0;
    return sl_ranges(h->n_cu, n, k);
}

extern "C" int scd_silhouette(scd_handle h, const void* X, int x_dtype, const int32_t* labels, int64_t n, int d, int k, float* samples_out,
                              double* mean_out, int64_t* info_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_silhouette");
    SCD_REQUIRE(X && labels && samples_out && mean_out && info_out && ws, "scd_silhouette: null argument");
    SCD_REQUIRE(x_dtype == SCD_F32 || x_dtype == SCD_F16, "scd_silhouette: x_dtype must be SCD_F32 or SCD_F16");
    SCD_REQUIRE(n >= 2 && n <= (1ll << 30), "scd_silhouette: n = %lld outside [2, 2^30]", (long long)n);
    SCD_REQUIRE(d >= 1 && scd_cdiv(d, 32) * 32 <= SL_DP_MAX, "scd_silhouette: d = %d outside [1, %d]", d, SL_DP_MAX);
    SCD_REQUIRE(k >= 2 && k <= n, "scd_silhouette: k = %d outside [2, n = %lld]", k, (long long)n);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_silhouette: workspace not 16-byte aligned");
    sl_plan p;
    sl_layout(n, d, k, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_silhouette: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    const long long gather_blocks = scd_cdiv(n + p.n_alloc, 4);
    SCD_REQUIRE(gather_blocks < (1ll << 31) && (size_t)k * p.chunks < ((size_t)1 << 40), "scd_silhouette: grid too large");
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    half_t* Xs = (half_t*)(w + p.xs);
    float* nrm = (float*)(w + p.nrm);
    int* slab = (int*)(w + p.slab);
    int* rowpos = (int*)(w + p.rowpos);
    unsigned* hist = (unsigned*)(w + p.hist);
    int* off = (int*)(w + p.off);
    int* meta = (int*)(w + p.meta);
    float* a_sum = (float*)(w + p.a_sum);
    float* part_b = (float*)(w + p.part_b);
    double* part_d = (double*)(w + p.part_d);

    SCD_HIP(hipMemsetAsync(hist, 0, (size_t)k * p.chunks * 4, st));
    SCD_HIP(hipMemsetAsync(info_out, 0, 16, st));
    sl_rank_kernel<<<(unsigned)p.chunks, SL_SORT, 0, st>>>(labels, n, k, p.chunks, rowpos, hist);
    sl_scan_kernel<<<1, SL_SORT, 0, st>>>(hist, (long long)k * p.chunks, meta);
    sl_offsets_kernel<<<(unsigned)scd_cdiv((long long)k + 1, 256), 256, 0, st>>>(hist, p.chunks, k, meta, n, off, (long long*)info_out);
    if (x_dtype == SCD_F32)
        sl_gather_kernel<float><<<(unsigned)gather_blocks, 256, 0, st>>>((const float*)X, labels, n, d, p.ld, p.chunks, p.n_alloc, hist, meta,
                                                                        rowpos, Xs, nrm, slab);
    else
        sl_gather_kernel<half_t><<<(unsigned)gather_blocks, 256, 0, st>>>((const half_t*)X, labels, n, d, p.ld, p.chunks, p.n_alloc, hist, meta,
                                                                         rowpos, Xs, nrm, slab);
    SCD_LAUNCH_CHECK();
    const long long panels = scd_cdiv(n, SL_BM);
    const int ny = sl_ranges(h->n_cu, n, k);                    // <= p.ny_max, which sizes part_b
    { const int rc_ = scd_set_max_lds((const void*)sl_main_kernel, SL_LDS_BYTES); if (rc_) return rc_; }
    sl_main_kernel<<<dim3((unsigned)panels, (unsigned)ny), SL_THREADS, SL_LDS_BYTES, st>>>(Xs, nrm, slab, off, meta, k, p.ld, p.dp, p.n_alloc,
                                                                                          a_sum, part_b);
    sl_finish_kernel<<<SL_FIN_BLOCKS, SL_FIN_THREADS, 0, st>>>(labels, rowpos, off, a_sum, part_b, (int)ny, p.n_alloc, n,
                                                               (const long long*)info_out, samples_out, part_d);
    sl_mean_kernel<<<1, SL_FIN_BLOCKS, 0, st>>>(part_d, n, mean_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
