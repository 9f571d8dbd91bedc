// FINCH first-neighbour clustering on gfx950 (Sarfraz et al., "Efficient Parameter-free Clustering Using First Neighbor Relations",
// CVPR 2019; the reference's local_utils/finch.py), cosine distance.  docs/design/finch.md has the semantics and the derivations.
//
//   scd_first_neighbor      nn[i] = argmax_{j != i} dot(U_i, U_j) with the dot taken in float64 on the fp32 rows, ties to the lowest j
//                           (finch.py:25-27), d1[i] = 1 - that dot.  Filter and refine:
//                             1. fn_prep_kernel: an fp16 copy H of the rows (subnormal halfs flushed to zero, rows zero-filled to ld, the rows
//                                past n zero), per row e_i = |U_i - H_i| and h_i = |H_i|, their maxima over the rows, and a flag when a value
//                                does not fit fp16;
//                             2. fn_main_kernel: the n x n x d pass with v_mfma_f32_16x16x32_f16.  A block owns a panel of 128 rows and a
//                                range of 128-column tiles (grid.y).  Of the 16 x 16 MFMA output a lane holds 4 rows x 1 column, so the 16
//                                lanes that share a row see the columns of one residue class mod 16 each; per row a lane keeps the largest
//                                approximate dot of its class with its column (lowest column on ties) and the second largest value.  Self
//                                and the padding columns are excluded by index.  No n x n matrix reaches memory: per row and range the 16
//                                (value, column) pairs and the largest second value are written;
//                             3. fn_refine_kernel, a wave per row: with s1 the largest approximate dot of the row and B_i the error bound
//                                below, every column whose exact dot can reach the row's maximum has an approximate dot >= s1 - 2 B_i.  If
//                                every lane's second value lies below that threshold the kept pairs at or above it are ALL such columns:
//                                their float64 dots decide, ties to the lowest column.  Otherwise the row takes the exact pass over all
//                                columns (counted in info_out[0]).  The result never depends on the filter.
//                           Error bound of an approximate dot s_ij against t_ij = U_i . U_j:  with U = H + R,
//                             |t_ij - H_i . H_j| <= e_i (h_j + e_j) + h_i e_j   (Cauchy-Schwarz on R_i . H_j + H_i . R_j + R_i . R_j),
//                           products of two halfs are exact in fp32 and the fp32 accumulation of dp / 32 MFMA steps is charged
//                             2^-22 (dp / 32 + 1) h_i h_j   (2^-23 per step relative to the step's sum of magnitudes, doubled),
//                           so B_i = e_i (h_max + e_max) + h_i e_max + 2^-22 (dp / 32 + 1) h_i h_max, evaluated in float64 and inflated by 1e-3.
//   scd_pair_dist_f64       1 - float64 dot of the fp32 rows for index pairs (the sibling term of min_sim, the cut mutual pairs)
//   scd_link_components     connected components of an undirected edge list, numbered by the rank of the lowest member: hooking onto the
//                           smaller index (atomicMin on integers) and pointer jumping until a device-side change flag stays clear
//   scd_segment_mean_unit   per-segment float64 sums in row order -> fp32 means (finch.py:56-69) and their unit rows
//
// One float64 dot (fn_dot64: four strided partial sums, one lane) serves the refine stage, the exact pass and scd_pair_dist_f64, so a
// pair has one value wherever it is evaluated.  No floating-point atomics: two calls on one input return the same bits.
#include "common.h"
#include "finch_shared.h"                       // fn_dot64, fn_vec_ok, fn_prep_kernel

#define FN_BM 128
#define FN_BN 128
#define FN_BK 64
#define FN_LDK 72                               // LDS row stride in halfs (144 bytes): the 16 rows of a fragment read spread over the banks
#define FN_THREADS 256
#define FN_YMAX 32
#define FN_TARGET_BLOCKS 1024                   // grid.y is chosen so that panels x ranges stays near this
#define FN_LDS_BYTES (2 * (FN_BM + FN_BN) * FN_LDK * 2)
#define FN_DP_MAX 1024

// ------------------------------------------------------------------------------------------------ the n x n x d filter pass
__global__ void __launch_bounds__(FN_THREADS) fn_main_kernel(const half_t* __restrict__ H, long long n, int ld, int dp, long long n_alloc,
                                                             long long tiles, long long tiles_per_y, float* __restrict__ cand_v,
                                                             int* __restrict__ cand_i, float* __restrict__ v2_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fn_lds[];
    half_t* sA = reinterpret_cast<half_t*>(fn_lds);             // [2][FN_BM][FN_LDK]
    half_t* sB = sA + 2 * FN_BM * FN_LDK;                       // [2][FN_BN][FN_LDK]
    const long long row0 = (long long)blockIdx.x * FN_BM;
    const int y = blockIdx.y;
    long long t_lo = (long long)y * tiles_per_y, t_hi = t_lo + tiles_per_y;
    if (t_hi > tiles) t_hi = tiles;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    float v1[2][4], v2[2][4];
    int i1[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v1[mt][r] = -INFINITY;
            v2[mt][r] = -INFINITY;
            i1[mt][r] = -1;
        }
    const int nk = ld / FN_BK;
    const int lrow = tid >> 3, lk = (tid & 7) * 8;              // 16-byte vector tid + 256 i of a chunk: row lrow + 32 i, halfs lk .. lk + 7
    const half_t* gA = H + (size_t)(row0 + lrow) * ld + lk;
    const int a_frag = (wave * 32 + lr) * FN_LDK + lq * 8, b_frag = lr * FN_LDK + lq * 8, st_off = lrow * FN_LDK + lk;

    for (long long t = t_lo; t < t_hi; ++t) {
        const long long j0 = t * FN_BN;
        const half_t* gB = H + (size_t)(j0 + lrow) * ld + lk;
        f32x4 acc[2][8];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        half8 ra[4], rb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ra[i] = *reinterpret_cast<const half8*>(gA + (size_t)i * 32 * ld);
            rb[i] = *reinterpret_cast<const half8*>(gB + (size_t)i * 32 * ld);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<half8*>(sA + st_off + i * 32 * FN_LDK) = ra[i];
            *reinterpret_cast<half8*>(sB + st_off + i * 32 * FN_LDK) = rb[i];
        }
        __syncthreads();
        for (int kc = 0; kc < nk; ++kc) {
            const int cur = kc & 1;
            const bool more = kc + 1 < nk;
            if (more) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ra[i] = *reinterpret_cast<const half8*>(gA + (size_t)i * 32 * ld + (kc + 1) * FN_BK);
                    rb[i] = *reinterpret_cast<const half8*>(gB + (size_t)i * 32 * ld + (kc + 1) * FN_BK);
                }
            }
            const half_t* cA = sA + cur * (FN_BM * FN_LDK) + a_frag;
            const half_t* cB = sB + cur * (FN_BN * FN_LDK) + b_frag;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (kc * FN_BK + ks * 32 < dp) {
                    const half8 fa0 = *reinterpret_cast<const half8*>(cA + ks * 32);
                    const half8 fa1 = *reinterpret_cast<const half8*>(cA + 16 * FN_LDK + ks * 32);
#pragma unroll
                    for (int nt = 0; nt < 8; ++nt) {
                        const half8 fb = *reinterpret_cast<const half8*>(cB + nt * 16 * FN_LDK + ks * 32);
                        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa0, fb, acc[0][nt], 0, 0, 0);
                        acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1, fb, acc[1][nt], 0, 0, 0);
                    }
                }
            }
            if (more) {
                half_t* nA = sA + (cur ^ 1) * (FN_BM * FN_LDK) + st_off;
                half_t* nB = sB + (cur ^ 1) * (FN_BN * FN_LDK) + st_off;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    *reinterpret_cast<half8*>(nA + i * 32 * FN_LDK) = ra[i];
                    *reinterpret_cast<half8*>(nB + i * 32 * FN_LDK) = rb[i];
                }
            }
            __syncthreads();
        }
        // epilogue: the lane's running best and second best per row; columns arrive in increasing order, so `>` keeps the lowest column
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const long long col = j0 + nt * 16 + lr;
            const bool valid = col < n;
            const long long dc = col - row0;
            const int dcol = (dc >= 0 && dc < FN_BM) ? (int)dc : -1;                      // the column's place in this panel, or -1
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int loc = wave * 32 + mt * 16 + lq * 4 + r;
                    const float vv = (valid && dcol != loc) ? acc[mt][nt][r] : -INFINITY;
                    const bool gt = vv > v1[mt][r];
                    v2[mt][r] = gt ? v1[mt][r] : fmaxf(v2[mt][r], vv);
                    i1[mt][r] = gt ? (int)col : i1[mt][r];
                    v1[mt][r] = gt ? vv : v1[mt][r];
                }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long p = row0 + wave * 32 + mt * 16 + lq * 4 + r;
            float s = v2[mt][r];
            s = fmaxf(s, __shfl_xor(s, 1, 64));
            s = fmaxf(s, __shfl_xor(s, 2, 64));
            s = fmaxf(s, __shfl_xor(s, 4, 64));
            s = fmaxf(s, __shfl_xor(s, 8, 64));
            if (p < n) {
                const size_t q = (size_t)y * n_alloc + p;
                cand_v[q * 16 + lr] = v1[mt][r];
                cand_i[q * 16 + lr] = i1[mt][r];
                if (lr == 0) v2_out[q] = s;
            }
        }
}

// ------------------------------------------------------------------------------------------------ refine / exact pass
__device__ __forceinline__ void fn_take(double& v, int& j, double ov, int oj) {
    if (ov > v || (ov == v && oj < j)) {
        v = ov;
        j = oj;
    }
}

__global__ void __launch_bounds__(256) fn_refine_kernel(const float* __restrict__ U, long long n, int d, int dp, long long n_alloc, int ny,
                                                        const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                        const float* __restrict__ v2_in, const float* __restrict__ e_in,
                                                        const float* __restrict__ h_in, const unsigned* __restrict__ gstat,
                                                        int* __restrict__ nn_out, double* __restrict__ d1_out, int* __restrict__ info) {
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const double hmax = (double)__uint_as_float(gstat[0]), emax = (double)__uint_as_float(gstat[1]);
    const bool overflow = gstat[2] != 0;
    const double ei = (double)e_in[i], hi = (double)h_in[i];
    const double acc_err = 2.384185791015625e-07 * (double)(dp / 32 + 1);                  // 2^-22 (dp / 32 + 1)
    const double B = (ei * (hmax + emax) + hi * emax + acc_err * hi * hmax) * 1.001 + 1e-300;
    const int ne = ny * 16;
    float s1 = -INFINITY, s2 = -INFINITY;
    for (int q = lane; q < ne; q += 64) s1 = fmaxf(s1, cand_v[((size_t)(q >> 4) * n_alloc + i) * 16 + (q & 15)]);
    for (int q = lane; q < ny; q += 64) s2 = fmaxf(s2, v2_in[(size_t)q * n_alloc + i]);
    s1 = wave_max_f32(s1);
    s2 = wave_max_f32(s2);
    const double theta = (double)s1 - 2.0 * B;
    const bool certified = !overflow && s1 > -INFINITY && s1 < INFINITY && (double)s2 < theta;
    const float* ui = U + (size_t)i * d;
    const bool vec = fn_vec_ok(U, d);
    double bv = -INFINITY;
    int bj = 0x7fffffff;
    if (certified) {
        for (int q = lane; q < ne; q += 64) {
            const size_t at = ((size_t)(q >> 4) * n_alloc + i) * 16 + (q & 15);
            const float v = cand_v[at];
            const int j = cand_i[at];
            if (j >= 0 && (double)v >= theta) fn_take(bv, bj, fn_dot64(ui, U + (size_t)j * d, d, vec), j);
        }
    } else {                                                    // a lane per column: 64 columns in flight per wave
        if (lane == 0) atomicAdd(&info[0], 1);
        for (long long j = lane; j < n; j += 64)
            if (j != i) fn_take(bv, bj, fn_dot64(ui, U + (size_t)j * d, d, vec), (int)j);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        fn_take(bv, bj, ov, oj);
    }
    if (lane == 0) {
        nn_out[i] = bj;
        d1_out[i] = 1.0 - bv;
        if (overflow && i == 0) info[1] = 1;
    }
}

struct fn_plan {
    int ld, dp, ny_max;
    long long n_alloc, tiles;
    size_t h, e, hn, gstat, cand_v, cand_i, v2, end;
};

static void fn_layout(int64_t n, int d, fn_plan& p) {
    p.dp = (int)scd_cdiv(d, 32) * 32;
    p.ld = (int)scd_cdiv(d, FN_BK) * FN_BK;
    p.tiles = scd_cdiv(n, FN_BM);
    p.n_alloc = p.tiles * FN_BM;
    long long ny = scd_cdiv(FN_TARGET_BLOCKS, p.tiles);
    if (ny > FN_YMAX) ny = FN_YMAX;
    if (ny > p.tiles) ny = p.tiles;
    p.ny_max = (int)ny;
    p.h = 0;                                                                        // H      f16   [n_alloc, ld]
    p.e = p.h + scd_align((size_t)p.n_alloc * p.ld * 2);                            // e      f32   [n]
    p.hn = p.e + scd_align((size_t)n * 4);                                          // h      f32   [n]
    p.gstat = p.hn + scd_align((size_t)n * 4);                                      // gstat  u32   [4]
    p.cand_v = p.gstat + scd_align(16);                                             // cand_v f32   [ny_max, n_alloc, 16]
    p.cand_i = p.cand_v + scd_align((size_t)p.ny_max * p.n_alloc * 64);             // cand_i int32 [ny_max, n_alloc, 16]
    p.v2 = p.cand_i + scd_align((size_t)p.ny_max * p.n_alloc * 64);                 // v2     f32   [ny_max, n_alloc]
    p.end = p.v2 + scd_align((size_t)p.ny_max * p.n_alloc * 4);
}

static bool fn_shape_ok(int64_t n, int d) { return n >= 2 && n < (1ll << 31) && d >= 1 && scd_cdiv(d, 32) * 32 <= FN_DP_MAX; }

extern "C" size_t scd_first_neighbor_ws_bytes(int64_t n, int d) {
    if (!fn_shape_ok(n, d)) return 0;
    fn_plan p;
    fn_layout(n, d, p);
    return p.end;
}

extern "C" int scd_first_neighbor(scd_handle h, const float* U, int64_t n, int d, int32_t* nn_out, double* d1_out, int32_t* info_out, void* ws,
                                  size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_first_neighbor");
    SCD_REQUIRE(U && nn_out && d1_out && info_out && ws, "scd_first_neighbor: null argument");
    SCD_REQUIRE(n >= 2 && n < (1ll << 31), "scd_first_neighbor: n = %lld outside [2, 2^31)", (long long)n);
    SCD_REQUIRE(d >= 1 && scd_cdiv(d, 32) * 32 <= FN_DP_MAX, "scd_first_neighbor: d = %d outside [1, %d]", d, FN_DP_MAX);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_first_neighbor: workspace not 16-byte aligned");
    fn_plan p;
    fn_layout(n, d, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_first_neighbor: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    SCD_REQUIRE(scd_cdiv(p.n_alloc, 4) < (1ll << 31), "scd_first_neighbor: grid too large");
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    half_t* H = (half_t*)(w + p.h);
    float* e = (float*)(w + p.e);
    float* hn = (float*)(w + p.hn);
    unsigned* gstat = (unsigned*)(w + p.gstat);
    float* cand_v = (float*)(w + p.cand_v);
    int* cand_i = (int*)(w + p.cand_i);
    float* v2 = (float*)(w + p.v2);

    SCD_HIP(hipMemsetAsync(gstat, 0, 16, st));
    SCD_HIP(hipMemsetAsync(info_out, 0, 8, st));
    fn_prep_kernel<<<(unsigned)scd_cdiv(p.n_alloc, 4), 256, 0, st>>>(U, n, d, p.ld, p.n_alloc, H, e, hn, gstat);
    SCD_LAUNCH_CHECK();
    // ranges of column tiles (grid.y): enough blocks to fill the device a few times over when there are few panels.  The result does
    // not depend on it: the refine stage looks at every range's pairs.
    long long ny = scd_cdiv(4ll * h->n_cu, p.tiles);
    if (ny > p.ny_max) ny = p.ny_max;
    if (ny < 1) ny = 1;
    const long long tiles_per_y = scd_cdiv(p.tiles, ny);
    ny = scd_cdiv(p.tiles, tiles_per_y);                        // no empty range
    { const int rc_ = scd_set_max_lds((const void*)fn_main_kernel, FN_LDS_BYTES); if (rc_) return rc_; }
    fn_main_kernel<<<dim3((unsigned)p.tiles, (unsigned)ny), FN_THREADS, FN_LDS_BYTES, st>>>(H, n, p.ld, p.dp, p.n_alloc, p.tiles, tiles_per_y,
                                                                                          cand_v, cand_i, v2);
    fn_refine_kernel<<<(unsigned)scd_cdiv(n, 4), 256, 0, st>>>(U, n, d, p.dp, p.n_alloc, (int)ny, cand_v, cand_i, v2, e, hn, gstat, nn_out,
                                                               d1_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ pair distances
__global__ void __launch_bounds__(256) fn_pair_kernel(const float* __restrict__ U, long long n, int d, const int* __restrict__ a,
                                                      const int* __restrict__ b, long long m, double* __restrict__ out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= m) return;
    const long long ia = a[p], ib = b[p];
    double v = NAN;                                             // an index outside [0, n) reads nothing
    if (ia >= 0 && ia < n && ib >= 0 && ib < n) v = 1.0 - fn_dot64(U + (size_t)ia * d, U + (size_t)ib * d, d, fn_vec_ok(U, d));
    out[p] = v;
}

extern "C" int scd_pair_dist_f64(scd_handle h, const float* U, int64_t n, int d, const int32_t* a, const int32_t* b, int64_t m, double* out,
                                 void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_pair_dist_f64");
    SCD_REQUIRE(n >= 1 && n < (1ll << 31) && d >= 1 && m >= 0 && scd_cdiv(m, 256) < (1ll << 31), "scd_pair_dist_f64: bad shape");
    if (m == 0) return SCD_OK;
    SCD_REQUIRE(U && a && b && out, "scd_pair_dist_f64: null argument");
    fn_pair_kernel<<<(unsigned)scd_cdiv(m, 256), 256, 0, (hipStream_t)stream_>>>(U, n, d, a, b, m, out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ connected components
// parent[x] <= x always and parent[x] is a member of x's component, so there are no cycles and the lowest member stays its own parent.
// At the fixed point (no hook and no jump changed anything) every parent is a root and the ends of every edge share it: one root per
// component, the lowest member.  Integer atomicMin only: the fixed point does not depend on the order of the steps.
__global__ void __launch_bounds__(256) lc_init_kernel(int* __restrict__ parent, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (int)i;
}

__global__ void __launch_bounds__(256) lc_hook_kernel(int* __restrict__ parent, long long n, const int* __restrict__ ea,
                                                      const int* __restrict__ eb, long long m, int* __restrict__ flag) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    const long long a = ea[e], b = eb[e];
    if (a < 0 || a >= n || b < 0 || b >= n) {                   // not an edge of this graph: skipped and reported
        flag[1] = 1;
        return;
    }
    const int ra = parent[a], rb = parent[b];
    if (ra == rb) return;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    atomicMin(&parent[hi], lo);
    flag[0] = 1;
}

__global__ void __launch_bounds__(256) lc_jump_kernel(int* __restrict__ parent, long long n, int* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p0 = parent[i];
    int p = p0;
    for (;;) {
        const int q = parent[p];
        if (q == p) break;
        p = q;
    }
    if (p != p0) {
        atomicMin(&parent[i], p);
        flag[0] = 1;
    }
}

#define LC_SCAN 1024
// rank[x] <- the number of roots below x, for every root x (one block; thread t owns a contiguous piece); ncomp <- the number of roots
__global__ void __launch_bounds__(LC_SCAN) lc_rank_kernel(const int* __restrict__ parent, long long n, int* __restrict__ rank,
                                                          int* __restrict__ ncomp) {
    __shared__ unsigned sh[LC_SCAN];
    const int t = threadIdx.x;
    const long long piece = (n + LC_SCAN - 1) / LC_SCAN;
    long long b0 = (long long)t * piece, b1 = b0 + piece;
    if (b0 > n) b0 = n;
    if (b1 > n) b1 = n;
    unsigned s = 0;
    for (long long q = b0; q < b1; ++q) s += parent[q] == (int)q;
    sh[t] = s;
    __syncthreads();
    for (int o = 1; o < LC_SCAN; o <<= 1) {
        const unsigned v = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += v;
        __syncthreads();
    }
    unsigned run = sh[t] - s;
    for (long long q = b0; q < b1; ++q)
        if (parent[q] == (int)q) rank[q] = (int)run++;
    if (t == LC_SCAN - 1) ncomp[0] = (int)sh[LC_SCAN - 1];
}

__global__ void __launch_bounds__(256) lc_label_kernel(const int* __restrict__ parent, const int* __restrict__ rank, long long n,
                                                       int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) labels[i] = rank[parent[i]];
}

extern "C" size_t scd_link_components_ws_bytes(int64_t n) {
    if (n < 1 || n >= (1ll << 31)) return 0;
    return 2 * scd_align((size_t)n * 4) + scd_align(16);
}

extern "C" int scd_link_components(scd_handle h, int64_t n, const int32_t* ea, const int32_t* eb, int64_t m, int32_t* labels_out,
                                   int32_t* ncomp_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_link_components");
    SCD_REQUIRE(n >= 1 && n < (1ll << 31), "scd_link_components: n = %lld outside [1, 2^31)", (long long)n);
    SCD_REQUIRE(m >= 0 && scd_cdiv(m, 256) < (1ll << 31), "scd_link_components: m = %lld out of range", (long long)m);
    SCD_REQUIRE(labels_out && ncomp_out && ws && (m == 0 || (ea && eb)), "scd_link_components: null argument");
    SCD_REQUIRE(ws_bytes >= scd_link_components_ws_bytes(n), "scd_link_components: workspace too small");
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_link_components: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream_;
    int* parent = (int*)ws;
    int* rank = (int*)((char*)ws + scd_align((size_t)n * 4));
    int* flag = (int*)((char*)ws + 2 * scd_align((size_t)n * 4));
    const unsigned gn = (unsigned)scd_cdiv(n, 256), gm = (unsigned)scd_cdiv(m, 256);
    lc_init_kernel<<<gn, 256, 0, st>>>(parent, n);
    SCD_HIP(hipMemsetAsync(flag, 0, 16, st));
    int bad_edge = 0;
    while (m > 0) {
        // two rounds per look at the flag; a round after the fixed point changes nothing
        for (int r = 0; r < 2; ++r) {
            lc_hook_kernel<<<gm, 256, 0, st>>>(parent, n, ea, eb, m, flag);
            lc_jump_kernel<<<gn, 256, 0, st>>>(parent, n, flag);
        }
        SCD_LAUNCH_CHECK();
        int host_flag[2] = {0, 0};
        SCD_HIP(hipMemcpyAsync(host_flag, flag, 8, hipMemcpyDeviceToHost, st));
        SCD_HIP(hipStreamSynchronize(st));
        bad_edge |= host_flag[1];
        if (!host_flag[0]) break;
        SCD_HIP(hipMemsetAsync(flag, 0, 16, st));
    }
    SCD_REQUIRE(!bad_edge, "scd_link_components: an edge end lies outside [0, n)");
    lc_rank_kernel<<<1, LC_SCAN, 0, st>>>(parent, n, rank, ncomp_out);
    lc_label_kernel<<<gn, 256, 0, st>>>(parent, rank, n, labels_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ segment means and their unit rows
// a block per segment; a thread owns columns tid, tid + 256, ...; the rows of the segment are added in their order in `order`
__global__ void __launch_bounds__(256) sm_mean_unit_kernel(const float* __restrict__ X, long long n, const int* __restrict__ order,
                                                           const long long* __restrict__ offsets, int d, float* __restrict__ mean_out,
                                                           float* __restrict__ unit_out) {
    __shared__ double sh[256];
    const long long c = blockIdx.x;
    long long s0 = offsets[c], s1 = offsets[c + 1];
    if (s0 < 0) s0 = 0;
    if (s1 > n) s1 = n;
    const double cnt = (double)(s1 - s0);
    double sq = 0.0;
    for (int col = threadIdx.x; col < d; col += 256) {
        double s = 0.0;
        long long q = s0;
        for (; q + 4 <= s1; q += 4) {
            const long long r0 = order[q], r1 = order[q + 1], r2 = order[q + 2], r3 = order[q + 3];
            const float x0 = (r0 >= 0 && r0 < n) ? X[(size_t)r0 * d + col] : 0.f;
            const float x1 = (r1 >= 0 && r1 < n) ? X[(size_t)r1 * d + col] : 0.f;
            const float x2 = (r2 >= 0 && r2 < n) ? X[(size_t)r2 * d + col] : 0.f;
            const float x3 = (r3 >= 0 && r3 < n) ? X[(size_t)r3 * d + col] : 0.f;
            s += (double)x0;
            s += (double)x1;
            s += (double)x2;
            s += (double)x3;
        }
        for (; q < s1; ++q) {
            const long long r0 = order[q];
            s += (double)((r0 >= 0 && r0 < n) ? X[(size_t)r0 * d + col] : 0.f);
        }
        const float mean = s1 > s0 ? (float)(s / cnt) : 0.f;
        mean_out[(size_t)c * d + col] = mean;
        sq = fma((double)mean, (double)mean, sq);
    }
    sh[threadIdx.x] = sq;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double nrm = sqrt(sh[0]);
    for (int col = threadIdx.x; col < d; col += 256) {
        const float mean = mean_out[(size_t)c * d + col];      // this thread's own store
        unit_out[(size_t)c * d + col] = nrm > 0.0 ? (float)((double)mean / nrm) : 0.f;
    }
}

extern "C" int scd_segment_mean_unit(scd_handle h, const float* X, int64_t n, const int32_t* order, const int64_t* offsets, int k, int d,
                                     float* mean_out, float* unit_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_segment_mean_unit");
    SCD_REQUIRE(X && order && offsets && mean_out && unit_out, "scd_segment_mean_unit: null argument");
    SCD_REQUIRE(n >= 1 && n < (1ll << 31) && k >= 1 && d >= 1, "scd_segment_mean_unit: bad shape (n = %lld, k = %d, d = %d)", (long long)n, k, d);
    sm_mean_unit_kernel<<<(unsigned)k, 256, 0, (hipStream_t)stream_>>>(X, n, order, (const long long*)offsets, d, mean_out, unit_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
