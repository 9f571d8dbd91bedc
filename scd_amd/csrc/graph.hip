// The sparse half of spectral clustering on the exact k-NN graph (scikit-learn 1.7's SpectralClustering(affinity='nearest_neighbors'):
// sklearn/cluster/_spectral.py, sklearn/manifold/_spectral_embedding.py, and scipy.sparse.csgraph.laplacian(normed=True) under them).
// docs/design/spectral.md has the definitions, the summation order and the numbers.
//
//   scd_knn_affinity   graph_count_kernel   a thread per list entry: the entry's validity, whether the edge is mutual, and the two rows'
//                                           lengths and doubled degrees (integer atomics: the sums do not depend on their order);
//                      graph_scan_kernel    rowptr = the exclusive prefix sums of the lengths, one block;
//                      graph_fill_kernel    every row's columns into a scratch copy, in arrival order;
//                      graph_sort_kernel    rank of every column inside its row (the columns of a row are distinct), then
//                                           col, val = A / (sqrt(d_i) sqrt(d_j)) at the rank: columns ascend, one fixed array.
//   scd_spmm_f64       graph_spmm_kernel    Y = alpha (S X) + beta X + gamma Z, a wave per destination row, whole source rows gathered
//                                           with 16-byte loads per lane, four in flight; a row of more than GRAPH_CHUNK entries by the
//                                           four waves of its block, a chunk each, partial sums added in chunk order.
//
// No floating-point atomics anywhere: two calls return the same bits.  This file is compiled with -ffp-contract=off (build.py): the
// row sums are a separate multiply and add per term, the operations numpy performs.
#include "common.h"

#define GRAPH_KMAX 64
#define GRAPH_CHUNK 512                             // entries of a row summed by one wave before a partial sum is formed
#define GRAPH_WAVE_ROW 1024                         // the longest row one wave ranks alone; longer rows take the whole block
#define GRAPH_MUTUAL 0x80000000u
#define GRAPH_SCAN_THREADS 1024
#define GRAPH_SCAN_PER 4

// ------------------------------------------------------------------------------------------------ the affinity
// Entry (i, j) with t = idx[i][j] counts when 0 <= t < n, t != i and t is not in idx[i][0 .. j).  The edge is mutual when i is in
// idx[t][.]; then row t has the column i from an entry of its own.  Otherwise row t gets the column i from this entry.
// Returns t, or -1 for an entry that does not count; *mutual is set for one that does.
__device__ __forceinline__ int graph_entry(const int* __restrict__ idx, long long n, int k, long long i, int j, bool* mutual, int* err) {
    const int* row = idx + (size_t)i * k;
    const int t = row[j];
    if (t < 0 || t == i) return -1;
    if (t >= n) {
        *err = 1;                                               // a plain store of the same value from every thread that sees one
        return -1;
    }
    for (int jj = 0; jj < j; ++jj)
        if (row[jj] == t) return -1;
    const int* back = idx + (size_t)t * k;
    bool m = false;
    for (int jj = 0; jj < k; ++jj) m |= back[jj] == (int)i;
    *mutual = m;
    return t;
}

__global__ void __launch_bounds__(256) graph_count_kernel(const int* __restrict__ idx, long long n, int k, int* __restrict__ len,
                                                         int* __restrict__ deg2, int* __restrict__ err) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * k) return;
    const long long i = e / k;
    bool mutual = false;
    const int t = graph_entry(idx, n, k, i, (int)(e - i * k), &mutual, err);
    if (t < 0) return;
    atomicAdd(&len[i], 1);
    atomicAdd(&deg2[i], mutual ? 2 : 1);                        // twice the affinity: 1.0 or 0.5
    if (!mutual) {
        atomicAdd(&len[t], 1);
        atomicAdd(&deg2[t], 1);
    }
}

// One block: rowptr[i] = len[0] + .. + len[i - 1], rowptr[n] = nnz (also to *nnz_dev).  Tiles of 4096 rows with a running carry.
__global__ void __launch_bounds__(GRAPH_SCAN_THREADS) graph_scan_kernel(const int* __restrict__ len, long long n, long long* __restrict__ rowptr,
                                                                       long long* __restrict__ nnz_dev) {
    __shared__ long long s[GRAPH_SCAN_THREADS];
    __shared__ long long carry_s;
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (long long base = 0; base < n; base += GRAPH_SCAN_THREADS * GRAPH_SCAN_PER) {
        long long v[GRAPH_SCAN_PER], mine = 0;
#pragma unroll
        for (int r = 0; r < GRAPH_SCAN_PER; ++r) {
            const long long i = base + (long long)t * GRAPH_SCAN_PER + r;
            v[r] = i < n ? len[i] : 0;
            mine += v[r];
        }
        s[t] = mine;
        __syncthreads();
        for (int o = 1; o < GRAPH_SCAN_THREADS; o <<= 1) {     // inclusive scan of the threads' sums
            const long long add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const long long carry = carry_s;
        long long run = carry + s[t] - mine;
#pragma unroll
        for (int r = 0; r < GRAPH_SCAN_PER; ++r) {
            const long long i = base + (long long)t * GRAPH_SCAN_PER + r;
            if (i < n) rowptr[i] = run;
            run += v[r];
        }
        __syncthreads();
        if (t == GRAPH_SCAN_THREADS - 1) carry_s = carry + s[t];
        __syncthreads();
    }
    if (t == 0) {
        rowptr[n] = carry_s;
        nnz_dev[0] = carry_s;
    }
}

// len[] counts down to zero here: it is the rows' free-slot cursor.
__global__ void __launch_bounds__(256) graph_fill_kernel(const int* __restrict__ idx, long long n, int k, const long long* __restrict__ rowptr,
                                                        int* __restrict__ len, unsigned* __restrict__ tmp, int* __restrict__ err) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * k) return;
    const long long i = e / k;
    bool mutual = false;
    const int t = graph_entry(idx, n, k, i, (int)(e - i * k), &mutual, err);
    if (t < 0) return;
    tmp[rowptr[i] + atomicSub(&len[i], 1) - 1] = (unsigned)t | (mutual ? GRAPH_MUTUAL : 0u);
    if (!mutual) tmp[rowptr[t] + atomicSub(&len[t], 1) - 1] = (unsigned)i;
}

// 1 / sqrt(d), and 1 for a row without an edge (scipy.sparse.csgraph.laplacian's isolated nodes)
__device__ __forceinline__ double graph_sqrt_deg(int deg2) { return deg2 > 0 ? sqrt(0.5 * (double)deg2) : 1.0; }

// Entries first, first + step, ... of row i: the rank of the entry's column among the row's columns, then col and val at that rank.
__device__ __forceinline__ void graph_rank_row(const unsigned* __restrict__ tmp, const int* __restrict__ deg2, long long lo, long long L,
                                               long long i, int first, int step, int* __restrict__ col, double* __restrict__ val) {
    const double si = graph_sqrt_deg(deg2[i]);
    for (long long e = first; e < L; e += step) {
        const unsigned raw = tmp[lo + e];
        const unsigned c = raw & ~GRAPH_MUTUAL;
        long long rank = 0;
        for (long long f = 0; f < L; ++f) rank += (tmp[lo + f] & ~GRAPH_MUTUAL) < c;
        const double a = (raw & GRAPH_MUTUAL) ? 1.0 : 0.5;
        col[lo + rank] = (int)c;
        val[lo + rank] = a / (si * graph_sqrt_deg(deg2[c]));
    }
}

__global__ void __launch_bounds__(256) graph_sort_kernel(const unsigned* __restrict__ tmp, const int* __restrict__ deg2,
                                                        const long long* __restrict__ rowptr, long long n, int* __restrict__ col,
                                                        double* __restrict__ val, double* __restrict__ inv_sqrt_deg) {
    const long long row0 = (long long)blockIdx.x * 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long i = row0 + wave;
    if (i < n) {
        const long long lo = rowptr[i], L = rowptr[i + 1] - lo;
        if (L <= GRAPH_WAVE_ROW) graph_rank_row(tmp, deg2, lo, L, i, lane, 64, col, val);
        if (lane == 0) inv_sqrt_deg[i] = 1.0 / graph_sqrt_deg(deg2[i]);
    }
    for (int r = 0; r < 4; ++r) {                               // a hub's row: all 256 threads
        const long long ii = row0 + r;
        if (ii >= n) break;
        const long long lo = rowptr[ii], L = rowptr[ii + 1] - lo;
        if (L > GRAPH_WAVE_ROW) graph_rank_row(tmp, deg2, lo, L, ii, (int)threadIdx.x, 256, col, val);
    }
}

struct graph_plan {
    size_t len, deg2, tmp, misc, end;
};

static bool graph_shape_ok(int64_t n, int k) { return n >= 2 && n < (1ll << 31) && k >= 1 && k <= GRAPH_KMAX; }

static void graph_layout(int64_t n, int k, graph_plan& p) {
    p.len = 0;                                                  // len  int32 [n]
    p.deg2 = p.len + scd_align((size_t)n * 4);                  // deg2 int32 [n]
    p.tmp = p.deg2 + scd_align((size_t)n * 4);                  // tmp  uint32 [2 n k]
    p.misc = p.tmp + scd_align((size_t)n * k * 8);              // misc int64 [2] = {nnz, error flag}
    p.end = p.misc + scd_align(16);
}

extern "C" size_t scd_knn_affinity_ws_bytes(int64_t n, int k) {
    if (!graph_shape_ok(n, k)) return 0;
    graph_plan p;
    graph_layout(n, k, p);
    return p.end;
}

extern "C" int scd_knn_affinity(scd_handle h, const int32_t* idx, int64_t n, int k, int64_t* rowptr, int32_t* col, double* val,
                                double* inv_sqrt_deg, int64_t cap, int64_t* nnz_out, void* ws, size_t ws_bytes, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_knn_affinity");
    SCD_REQUIRE(idx && rowptr && col && val && inv_sqrt_deg && nnz_out && ws, "scd_knn_affinity: null argument");
    SCD_REQUIRE(n >= 2 && n < (1ll << 31), "scd_knn_affinity: n = %lld outside [2, 2^31)", (long long)n);
    SCD_REQUIRE(k >= 1 && k <= GRAPH_KMAX, "scd_knn_affinity: k = %d outside [1, %d]", k, GRAPH_KMAX);
    SCD_REQUIRE(cap >= 2 * n * k, "scd_knn_affinity: cap = %lld below 2 n k = %lld", (long long)cap, (long long)(2 * n * k));
    SCD_REQUIRE((uintptr_t)ws % 16 == 0, "scd_knn_affinity: workspace not 16-byte aligned");
    graph_plan p;
    graph_layout(n, k, p);
    SCD_REQUIRE(ws_bytes >= p.end, "scd_knn_affinity: workspace too small (%zu < %zu bytes)", ws_bytes, p.end);
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    int* len = (int*)(w + p.len);
    int* deg2 = (int*)(w + p.deg2);
    unsigned* tmp = (unsigned*)(w + p.tmp);
    long long* misc = (long long*)(w + p.misc);
    SCD_HIP(hipMemsetAsync(w, 0, p.tmp, st));                   // len, deg2
    SCD_HIP(hipMemsetAsync(misc, 0, 16, st));
    const unsigned entry_blocks = (unsigned)scd_cdiv(n * k, 256);
    graph_count_kernel<<<entry_blocks, 256, 0, st>>>(idx, n, k, len, deg2, (int*)(misc + 1));
    graph_scan_kernel<<<1, GRAPH_SCAN_THREADS, 0, st>>>(len, n, (long long*)rowptr, misc);
    graph_fill_kernel<<<entry_blocks, 256, 0, st>>>(idx, n, k, (const long long*)rowptr, len, tmp, (int*)(misc + 1));
    graph_sort_kernel<<<(unsigned)scd_cdiv(n, 4), 256, 0, st>>>(tmp, deg2, (const long long*)rowptr, n, col, val, inv_sqrt_deg);
    SCD_LAUNCH_CHECK();
    long long host[2] = {0, 0};
    SCD_HIP(hipMemcpyAsync(host, misc, 16, hipMemcpyDeviceToHost, st));
    SCD_HIP(hipStreamSynchronize(st));
    SCD_REQUIRE(host[1] == 0, "scd_knn_affinity: a neighbour index is >= n = %lld", (long long)n);
    *nnz_out = host[0];
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ the sparse product
typedef double f64x2 __attribute__((ext_vector_type(2)));

// The sum over entries [e_lo, e_hi) of S, left to right, of val * X[col][c0 .. c0 + 1]: a multiply and an add per term.  The entries are
// the same in every lane (scalar loads); four source rows are in flight.  A column outside [0, n) reads nothing and adds val * 0.
__device__ __forceinline__ f64x2 graph_load_row(const double* __restrict__ X, long long ldx, long long n, int c, int c0) {
    const f64x2 zero = {0.0, 0.0};
    return (unsigned)c < (unsigned long long)n ? *(const f64x2*)(X + (size_t)c * ldx + c0) : zero;
}

__device__ __forceinline__ f64x2 graph_chunk_sum(const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ X,
                                                 long long ldx, long long n, long long e_lo, long long e_hi, int c0) {
    f64x2 s = {0.0, 0.0};
    long long e = e_lo;
    for (; e + 4 <= e_hi; e += 4) {
        f64x2 x[4];
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = val[e + u];
            x[u] = graph_load_row(X, ldx, n, col[e + u], c0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const f64x2 p = x[u] * v[u];
            s = s + p;
        }
    }
    for (; e < e_hi; ++e) {
        const f64x2 p = graph_load_row(X, ldx, n, col[e], c0) * val[e];
        s = s + p;
    }
    return s;
}

__device__ __forceinline__ void graph_store_row(f64x2 s, const double* __restrict__ X, long long ldx, const double* __restrict__ Z, long long ldz,
                                                double* __restrict__ Y, long long ldy, long long i, int c0, double alpha, double beta,
                                                double gamma) {
    const f64x2 x = *(const f64x2*)(X + (size_t)i * ldx + c0);
    f64x2 y = s * alpha + x * beta;
    if (Z) y = y + *(const f64x2*)(Z + (size_t)i * ldz + c0) * gamma;
    *(f64x2*)(Y + (size_t)i * ldy + c0) = y;
}

__global__ void __launch_bounds__(256) graph_spmm_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                        const double* __restrict__ val, long long n, const double* __restrict__ X,
                                                        long long ldx, int m, double alpha, double beta, double gamma,
                                                        const double* __restrict__ Z, long long ldz, double* __restrict__ Y, long long ldy) {
    __shared__ f64x2 part[4][64];
    const long long row0 = (long long)blockIdx.x * 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long long i = row0 + wave;
    const long long nnz = rowptr[n];
    if (i < n) {
        long long lo = rowptr[i], hi = rowptr[i + 1];
        if (!(lo >= 0 && lo <= hi && hi <= nnz)) lo = hi = 0;   // a broken row pointer: the row is read as empty
        if (hi - lo <= GRAPH_CHUNK)
            for (int c0 = lane * 2; c0 < m; c0 += 128)          // m % 8 == 0: a lane's two columns are both inside or both outside
                graph_store_row(graph_chunk_sum(col, val, X, ldx, n, lo, hi, c0), X, ldx, Z, ldz, Y, ldy, i, c0, alpha, beta, gamma);
    }
    for (int r = 0; r < 4; ++r) {                               // a long row: a chunk per wave and round, partial sums in chunk order
        const long long ii = row0 + r;
        if (ii >= n) break;
        const long long lo = rowptr[ii], hi = rowptr[ii + 1];
        if (!(lo >= 0 && lo <= hi && hi <= nnz) || hi - lo <= GRAPH_CHUNK) continue;    // the same in every thread of the block
        const long long chunks = (hi - lo + GRAPH_CHUNK - 1) / GRAPH_CHUNK;
        for (int cb = 0; cb < m; cb += 128) {
            const int c0 = cb + lane * 2;
            f64x2 acc = {0.0, 0.0};
            for (long long base = 0; base < chunks; base += 4) {
                const long long ch = base + wave;
                if (ch < chunks && c0 < m) {
                    const long long e_lo = lo + ch * GRAPH_CHUNK;
                    const long long e_hi = e_lo + GRAPH_CHUNK < hi ? e_lo + GRAPH_CHUNK : hi;
                    part[wave][lane] = graph_chunk_sum(col, val, X, ldx, n, e_lo, e_hi, c0);
                }
                __syncthreads();
                if (wave == 0 && c0 < m)
                    for (int w = 0; w < 4 && base + w < chunks; ++w) acc = acc + part[w][lane];
                __syncthreads();
            }
            if (wave == 0 && c0 < m) graph_store_row(acc, X, ldx, Z, ldz, Y, ldy, ii, c0, alpha, beta, gamma);
        }
    }
}

static bool graph_overlap(const double* a, int64_t lda, int m, const double* b, int64_t ldb, int64_t n) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + ((size_t)(n - 1) * lda + m) * 8;
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + ((size_t)(n - 1) * ldb + m) * 8;
    return a0 < b1 && b0 < a1;
}

extern "C" int scd_spmm_f64(scd_handle h, const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const double* X, int64_t ldx,
                            int m, double alpha, double beta, double gamma, const double* Z, int64_t ldz, double* Y, int64_t ldy,
                            void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_spmm_f64");
    SCD_REQUIRE(rowptr && col && val && X && Y, "scd_spmm_f64: null argument");
    SCD_REQUIRE(n >= 1 && n < (1ll << 31), "scd_spmm_f64: n = %lld outside [1, 2^31)", (long long)n);
    SCD_REQUIRE(m >= 8 && m % 8 == 0, "scd_spmm_f64: m = %d must be a positive multiple of 8 (m %% 8 == 0)", m);
    SCD_REQUIRE(ldx >= m && ldy >= m && ldx % 8 == 0 && ldy % 8 == 0 && (!Z || (ldz >= m && ldz % 8 == 0)),
                "scd_spmm_f64: the leading dimensions must be multiples of 8 and at least m = %d", m);
    SCD_REQUIRE((uintptr_t)X % 16 == 0 && (uintptr_t)Y % 16 == 0 && (uintptr_t)Z % 16 == 0, "scd_spmm_f64: X, Y and Z must be 16-byte aligned");
    // the spans of the blocks, padding columns included: an interleaved Y (a column slice of the buffer X lives in) is refused too
    SCD_REQUIRE(!graph_overlap(Y, ldy, m, X, ldx, n) && (!Z || !graph_overlap(Y, ldy, m, Z, ldz, n)),
                "scd_spmm_f64: Y must not alias X or Z");
    graph_spmm_kernel<<<(unsigned)scd_cdiv(n, 4), 256, 0, (hipStream_t)stream_>>>((const long long*)rowptr, col, val, n, X, ldx, m, alpha, beta,
                                                                                    gamma, Z, ldz, Y, ldy);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
