// Clustering scores for gfx950: the contingency table of a clustering against targets, and the statistics ACC / NMI / ARI / purity
// are computed from.
//
// Replaces, under the reference's gcd/:
//   project_utils/cluster_utils.py:39-62   cluster_acc: `for i in range(y_pred.size): w[y_pred[i], y_true[i]] += 1`
//   project_utils/cluster_utils.py:65-69   purity_score: contingency_matrix, sum of the column maxima
//   methods/estimate_k/estimate_k.py:87-94 cluster_acc / nmi_score / ari_score on `[mask]` and on `[~mask]`: three passes over the
//                                          labels per subset, each building the same table again on the host
// Counts are integers and added with integer atomics only: the tables are exact and do not depend on the arrival order.  The float64
// sums of the statistics use no atomics at all: a fixed strided partition of the cells over ST_BLOCKS x ST_THREADS threads and fixed
// trees above it, so the three doubles are the same bits on every call.  No float atomics in this file.
#include "common.h"
#include <float.h>

// ------------------------------------------------------------------------------------------------ scd_contingency
#define CT_THREADS 512
#define CT_LDS_BYTES 131072                     // of the CU's 160 KB: the private table of one block (one block per CU)
#define CT_PRIVATE_CELLS (CT_LDS_BYTES / 4)
#define CT_UNIT 16                              // rows per lane and step: one 16-byte load of subset, four of pred and four of truth
#define CT_ROWS_PER_BLOCK_MIN (CT_UNIT * CT_THREADS)

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void ct_add(unsigned* cells, int p, int t, int tab, int kp, int kt, unsigned& bad) {
    if ((unsigned)p < (unsigned)kp && (unsigned)t < (unsigned)kt) atomicAdd(&cells[((size_t)tab * kp + p) * kt + t], 1u);
    else ++bad;
}

// Block b counts rows [b * rows_per_block, (b + 1) * rows_per_block) (rows_per_block: a multiple of CT_UNIT, so that with 16-byte
// aligned arrays every lane's unit is aligned too).  PRIVATE: into the block's LDS copy of the table(s), flushed with one global add per
// non-zero cell; otherwise straight into the table.  VEC: 16-byte loads, the rows past the last whole unit one by one.
template <bool PRIVATE, bool VEC>
__global__ void __launch_bounds__(CT_THREADS) contingency_kernel(const int* __restrict__ pred, const int* __restrict__ truth,
                                                                 const unsigned char* __restrict__ subset, long long n,
                                                                 long long rows_per_block, int kp, int kt, int cells,
                                                                 unsigned* __restrict__ table, unsigned long long* __restrict__ n_bad) {
    extern __shared__ unsigned ct_lds[];
    const int tid = threadIdx.x;
    unsigned* dst = table;
    if (PRIVATE) {
        for (int c = tid; c < cells; c += CT_THREADS) ct_lds[c] = 0u;
        __syncthreads();
        dst = ct_lds;
    }
    long long r0 = (long long)blockIdx.x * rows_per_block;
    if (r0 > n) r0 = n;
    const long long r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
    unsigned bad = 0;
    long long tail0 = r0;
    if (VEC) {
        const long long units = (r1 - r0) / CT_UNIT;
        for (long long u = tid; u < units; u += CT_THREADS) {
            const long long row = r0 + u * CT_UNIT;
            u32x4 sv = {0u, 0u, 0u, 0u};
            if (subset) sv = *reinterpret_cast<const u32x4*>(subset + row);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const i32x4 pv = *reinterpret_cast<const i32x4*>(pred + row + 4 * q);
                const i32x4 tv = *reinterpret_cast<const i32x4*>(truth + row + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int tab = (subset && ((sv[q] >> (8 * e)) & 0xffu) == 0u) ? 1 : 0;
                    ct_add(dst, pv[e], tv[e], tab, kp, kt, bad);
                }
            }
        }
        tail0 = r0 + units * CT_UNIT;
    }
    for (long long row = tail0 + tid; row < r1; row += CT_THREADS) {
        const int tab = (subset && subset[row] == 0) ? 1 : 0;
        ct_add(dst, pred[row], truth[row], tab, kp, kt, bad);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((tid & 63) == 0 && bad) atomicAdd(n_bad, (unsigned long long)bad);
    if (PRIVATE) {
        __syncthreads();
        for (int c = tid; c < cells; c += CT_THREADS) {
            const unsigned v = ct_lds[c];
            if (v) atomicAdd(&table[c], v);
        }
    }
}

extern "C" size_t scd_contingency_private_cells(void) { return CT_PRIVATE_CELLS; }

extern "C" int scd_contingency_last_path(scd_handle h) { return h ? h->cont_path : -1; }

extern "C" int scd_contingency(scd_handle h, const int32_t* pred, const int32_t* truth, const uint8_t* subset, int64_t n, int kp, int kt,
                               int32_t* table_out, int64_t* n_bad_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_contingency");
    SCD_REQUIRE(table_out && n_bad_out && (n == 0 || (pred && truth)), "scd_contingency: null argument");
    SCD_REQUIRE(n >= 0 && n < (1ll << 31), "scd_contingency: n = %lld outside [0, 2^31) (cells are int32)", (long long)n);
    SCD_REQUIRE(kp > 0 && kt > 0, "scd_contingency: bad table shape %d x %d", kp, kt);
    const int S = subset ? 2 : 1;
    const long long cells = (long long)S * kp * kt;
    SCD_REQUIRE(cells < (1ll << 31), "scd_contingency: %d tables of %d x %d cells: more than 2^31 - 1", S, kp, kt);
    hipStream_t st = (hipStream_t)stream_;
    SCD_HIP(hipMemsetAsync(table_out, 0, (size_t)cells * 4, st));
    SCD_HIP(hipMemsetAsync(n_bad_out, 0, 8, st));
    const bool priv = cells <= CT_PRIVATE_CELLS;
    h->cont_path = priv ? SCD_CONTINGENCY_PRIVATE : SCD_CONTINGENCY_GLOBAL;
    if (n == 0) return SCD_OK;
    const bool vec = ((uintptr_t)pred % 16 == 0) && ((uintptr_t)truth % 16 == 0) && ((uintptr_t)subset % 16 == 0);
    // a private block pays for zeroing and flushing its table: at most one per CU; the global path has no such cost
    const long long max_blocks = priv ? h->n_cu : 4ll * h->n_cu;
    long long rpb = scd_cdiv(n, max_blocks);
    if (rpb < CT_ROWS_PER_BLOCK_MIN) rpb = CT_ROWS_PER_BLOCK_MIN;
    rpb = scd_cdiv(rpb, CT_UNIT) * CT_UNIT;
    const unsigned grid = (unsigned)scd_cdiv(n, rpb);
    unsigned* tab = (unsigned*)table_out;
    unsigned long long* nb = (unsigned long long*)n_bad_out;
    if (priv) {
        const size_t lds = (size_t)cells * 4;
        if (vec) {
            { const int rc_ = scd_set_max_lds((const void*)contingency_kernel<true, true>, CT_LDS_BYTES); if (rc_) return rc_; }
            contingency_kernel<true, true><<<grid, CT_THREADS, lds, st>>>(pred, truth, subset, n, rpb, kp, kt, (int)cells, tab, nb);
        } else {
            { const int rc_ = scd_set_max_lds((const void*)contingency_kernel<true, false>, CT_LDS_BYTES); if (rc_) return rc_; }
            contingency_kernel<true, false><<<grid, CT_THREADS, lds, st>>>(pred, truth, subset, n, rpb, kp, kt, (int)cells, tab, nb);
        }
    } else if (vec) {
        contingency_kernel<false, true><<<grid, CT_THREADS, 0, st>>>(pred, truth, subset, n, rpb, kp, kt, (int)cells, tab, nb);
    } else {
        contingency_kernel<false, false><<<grid, CT_THREADS, 0, st>>>(pred, truth, subset, n, rpb, kp, kt, (int)cells, tab, nb);
    }
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ scd_contingency_stats
#define ST_THREADS 256
#define ST_BLOCKS 64                            // cell c of a table belongs to thread c mod (ST_BLOCKS * ST_THREADS): fixed, whatever the device

// fixed binary tree over the block's ST_THREADS values; every thread returns the total
__device__ __forceinline__ long long st_tree_i64(long long v, long long* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = ST_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double st_tree_f64(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = ST_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

// blocks [0, ceil(kp / 4)): a wave per table row -> its sum a_i and its maximum; the blocks after them: a thread per column -> b_j
__global__ void __launch_bounds__(ST_THREADS) st_marginals_kernel(const int* __restrict__ table, int kp, int kt, long long* __restrict__ a,
                                                                  int* __restrict__ rmax, long long* __restrict__ b) {
    const int s = blockIdx.y, row_blocks = (kp + 3) / 4;
    const int* T = table + (size_t)s * kp * kt;
    if ((int)blockIdx.x < row_blocks) {
        const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (row >= kp) return;
        long long sum = 0;
        int mx = 0;
        for (int j = lane; j < kt; j += 64) {
            const int v = T[(size_t)row * kt + j];
            sum += v;
            mx = v > mx ? v : mx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            const int om = __shfl_xor(mx, o, 64);
            mx = om > mx ? om : mx;
        }
        if (lane == 0) {
            a[(size_t)s * kp + row] = sum;
            rmax[(size_t)s * kp + row] = mx;
        }
    } else {
        const int j = ((int)blockIdx.x - row_blocks) * ST_THREADS + threadIdx.x;
        if (j >= kt) return;
        long long sum = 0;
        for (int i = 0; i < kp; ++i) sum += T[(size_t)i * kt + j];
        b[(size_t)s * kt + j] = sum;
    }
}

// block (x, s): the cells x * ST_THREADS + tid + m * ST_BLOCKS * ST_THREADS of table s -> partial sum n_ij^2, count of non-zero cells,
// partial mutual information (sklearn mutual_info_score, term by term)
__global__ void __launch_bounds__(ST_THREADS) st_cells_kernel(const int* __restrict__ table, int kp, int kt, const long long* __restrict__ a,
                                                              const long long* __restrict__ b, long long* __restrict__ part_i,
                                                              double* __restrict__ part_d) {
    __shared__ long long sh_i[ST_THREADS];
    __shared__ double sh_d[ST_THREADS];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int* T = table + (size_t)s * kp * kt;
    const long long* as = a + (size_t)s * kp;
    const long long* bs = b + (size_t)s * kt;
    long long loc = 0;
    for (int i = tid; i < kp; i += ST_THREADS) loc += as[i];
    const long long n = st_tree_i64(loc, sh_i);
    const double dn = (double)n, log_n = log(dn);
    long long ss = 0, nnz = 0;
    double mi = 0.0;
    const long long cells = (long long)kp * kt;
    for (long long c = (long long)blockIdx.x * ST_THREADS + tid; c < cells; c += (long long)ST_BLOCKS * ST_THREADS) {
        const int v = T[c];
        if (v > 0) {
            const long long i = c / kt, j = c - i * kt;
            ss += (long long)v * v;
            ++nnz;
            const double p = (double)v / dn;
            const double log_outer = -log((double)(as[i] * bs[j])) + log_n + log_n;
            double term = p * (log((double)v) - log_n) + p * log_outer;
            if (fabs(term) < DBL_EPSILON) term = 0.0;
            mi += term;
        }
    }
    ss = st_tree_i64(ss, sh_i);
    nnz = st_tree_i64(nnz, sh_i);
    mi = st_tree_f64(mi, sh_d);
    if (tid == 0) {
        part_i[((size_t)s * ST_BLOCKS + blockIdx.x) * 2 + 0] = ss;
        part_i[((size_t)s * ST_BLOCKS + blockIdx.x) * 2 + 1] = nnz;
        part_d[(size_t)s * ST_BLOCKS + blockIdx.x] = mi;
    }
}

// sklearn `entropy` of the positive entries of m[0 .. k): -sum (m / n) * (log m - log n); also sum m^2
__device__ __forceinline__ void st_entropy(const long long* m, int k, double dn, double log_n, long long* sh_i, double* sh_d, long long& sq,
                                           double& ent) {
    long long q = 0;
    double e = 0.0;
    for (int i = threadIdx.x; i < k; i += ST_THREADS) {
        const long long v = m[i];
        q += v * v;
        if (v > 0) e += ((double)v / dn) * (log((double)v) - log_n);
    }
    sq = st_tree_i64(q, sh_i);
    e = st_tree_f64(e, sh_d);
    ent = e == 0.0 ? 0.0 : -e;
}

__global__ void __launch_bounds__(ST_THREADS) st_final_kernel(int kp, int kt, const long long* __restrict__ a, const int* __restrict__ rmax,
                                                              const long long* __restrict__ b, const long long* __restrict__ part_i,
                                                              const double* __restrict__ part_d, long long* __restrict__ ints_out,
                                                              double* __restrict__ info_out) {
    __shared__ long long sh_i[ST_THREADS];
    __shared__ double sh_d[ST_THREADS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long* as = a + (size_t)s * kp;
    const long long* bs = b + (size_t)s * kt;
    long long loc = 0, pur = 0;
    for (int i = tid; i < kp; i += ST_THREADS) {
        loc += as[i];
        pur += rmax[(size_t)s * kp + i];
    }
    const long long n = st_tree_i64(loc, sh_i);
    pur = st_tree_i64(pur, sh_i);
    const double dn = (double)n, log_n = log(dn);
    long long sa2, sb2;
    double h_pred, h_truth;
    st_entropy(as, kp, dn, log_n, sh_i, sh_d, sa2, h_pred);
    st_entropy(bs, kt, dn, log_n, sh_i, sh_d, sb2, h_truth);
    const bool has = tid < ST_BLOCKS;
    const long long ss = st_tree_i64(has ? part_i[((size_t)s * ST_BLOCKS + tid) * 2 + 0] : 0, sh_i);
    const long long nnz = st_tree_i64(has ? part_i[((size_t)s * ST_BLOCKS + tid) * 2 + 1] : 0, sh_i);
    const double mi = st_tree_f64(has ? part_d[(size_t)s * ST_BLOCKS + tid] : 0.0, sh_d);
    if (tid == 0) {
        long long* io = ints_out + (size_t)s * 6;
        io[0] = n; io[1] = ss; io[2] = sa2; io[3] = sb2; io[4] = pur; io[5] = nnz;
        double* fo = info_out + (size_t)s * 3;
        fo[0] = h_pred; fo[1] = h_truth; fo[2] = mi;
    }
}

static void st_layout(int s, int kp, int kt, size_t off[6]) {
    off[0] = 0;                                                         // a      int64 [s, kp]
    off[1] = off[0] + scd_align((size_t)s * kp * 8);                    // b      int64 [s, kt]
    off[2] = off[1] + scd_align((size_t)s * kt * 8);                    // rmax   int32 [s, kp]
    off[3] = off[2] + scd_align((size_t)s * kp * 4);                    // part_i int64 [s, ST_BLOCKS, 2]
    off[4] = off[3] + scd_align((size_t)s * ST_BLOCKS * 16);            // part_d f64   [s, ST_BLOCKS]
    off[5] = off[4] + scd_align((size_t)s * ST_BLOCKS * 8);             // end
}

extern "C" size_t scd_contingency_stats_ws_bytes(int s, int kp, int kt) {
    if (s <= 0 || kp <= 0 || kt <= 0) return 0;
    size_t off[6];
    st_layout(s, kp, kt, off);
    return off[5];
}

extern "C" int scd_contingency_stats(scd_handle h, const int32_t* table, int s, int kp, int kt, int64_t* ints_out, double* info_out,
                                     void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_contingency_stats");
    SCD_REQUIRE(table && ints_out && info_out && ws, "scd_contingency_stats: null argument");
    SCD_REQUIRE(s > 0 && s <= 65535 && kp > 0 && kt > 0, "scd_contingency_stats: bad shape %d x %d x %d", s, kp, kt);
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_contingency_stats: workspace not 16-byte aligned");
    SCD_REQUIRE(ws_bytes >= scd_contingency_stats_ws_bytes(s, kp, kt), "scd_contingency_stats: workspace too small");
    hipStream_t st = (hipStream_t)stream_;
    size_t off[6];
    st_layout(s, kp, kt, off);
    char* w = (char*)ws;
    long long* a = (long long*)(w + off[0]);
    long long* b = (long long*)(w + off[1]);
    int* rmax = (int*)(w + off[2]);
    long long* part_i = (long long*)(w + off[3]);
    double* part_d = (double*)(w + off[4]);
    const unsigned gm = (unsigned)((kp + 3) / 4 + scd_cdiv(kt, ST_THREADS));
    st_marginals_kernel<<<dim3(gm, s), ST_THREADS, 0, st>>>(table, kp, kt, a, rmax, b);
    st_cells_kernel<<<dim3(ST_BLOCKS, s), ST_THREADS, 0, st>>>(table, kp, kt, a, b, part_i, part_d);
    st_final_kernel<<<s, ST_THREADS, 0, st>>>(kp, kt, a, rmax, b, part_i, part_d, (long long*)ints_out, info_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
