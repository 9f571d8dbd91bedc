/* scd_hip.h - C ABI of libscd_hip.so: the MI355X (gfx950) hot path of Visual-AI/SCD.
 *
 * The reference has no C ABI: its hot path is Python calling torch/sklearn/OR-Tools
 * (SURVEY.md section 8b).  Each entry point below replaces the reference code cited
 * next to it (paths relative to /root/reference); INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success or a negative scd_status; scd_last_error()
 *    returns a thread-local message for the last failure;
 *  - device pointers are raw (tensor.data_ptr()); the library never allocates or frees
 *    caller-visible memory: scratch comes from the `ws` argument whose size the matching
 *    *_ws_bytes() query returns (16-byte aligned);
 *  - all device work is enqueued on `stream` (a hipStream_t passed as void*) and is
 *    asynchronous; no call synchronises the device unless stated;
 *  - one handle per device / rank; handles are not shared between host threads.
 */
#ifndef SCD_HIP_H
#define SCD_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scd_ctx* scd_handle;
typedef struct scd_encoder scd_encoder;

enum scd_status { SCD_OK = 0, SCD_EINVAL = -1, SCD_EHIP = -2, SCD_ERCCL = -3, SCD_EINFEASIBLE = -4 };
enum scd_dtype { SCD_F32 = 0, SCD_F16 = 1 };
enum scd_sim_mode { SCD_SIM_RAW = 0, SCD_SIM_SOFTMAX = 1 };

int scd_version(void);
const char* scd_last_error(void);
int scd_create(int device, scd_handle* out);
int scd_destroy(scd_handle h);
/* Profiling aid: launches an empty kernel named scd_mark_begin_kernel (end = 0) or scd_mark_end_kernel (end != 0) on `stream`, so that a
 * kernel trace shows where a measured region starts and ends (bench.py brackets its timed steps; tools/trace_window_stats.py). */
int scd_trace_mark(scd_handle h, int end, void* stream);

/* ---- L2 normalisation: F.normalize(feats, dim=-1) main_unsup.py:130; clip_lang_util.py:103-105 ---- */
int scd_l2norm_rows(scd_handle h, const void* x, int dtype, int64_t n, int d, void* out, void* stream);

/* ---- similarity + top-k: main_unsup.py:504-531, main_ptsup.py:526-545 (a5); argmax re-classification
 *      main_unsup.py:601-614, main_ptsup.py:668-676, get_clip_preds_fast main_ptsup.py:78-99 (a6).
 * F  [n,d] fp16 row-major (image features);  Wt [v,d] fp16 row-major = zeroshot_weights.T (name-major).
 * d: a multiple of 64 up to 512 (ViT-B/16: 512), or 768 (ViT-L/14).
 * logits = scale * F @ Wt^T; order = (value desc, index asc) on the exact (float64) dot products.
 * idx_out int64 [n,k]; val_out float32 [n,k] (softmax probability when mode == SCD_SIM_SOFTMAX). k <= 8.
 * fallback_rows_out (device int32, may be NULL) counts rows that took the exact full-row path. */
size_t scd_sim_topk_ws_bytes(int64_t n, int d, int64_t v, int k);
int scd_sim_topk(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int k,
                 int mode, int64_t* idx_out, float* val_out, int32_t* fallback_rows_out, void* ws, size_t ws_bytes,
                 void* stream);
/* The vocabulary is constant over a run (main_unsup.py:389-394 loads it once; :504-531 uses it for every block of rows): its only
 * data-dependent ingredient in the error bound, max_v ||w_v||^2, can be computed ONCE (wmax2_out: 4 bytes of device memory) and handed
 * to every later call instead of being recomputed by each (12 us of a 2.7-ms call at V = 21,000).  The caller vouches that Wt has not
 * changed since; scd_sim_topk computes the norm itself. */
int scd_sim_vocab_norm(scd_handle h, const void* Wt, int64_t v, int d, void* wmax2_out, void* stream);
int scd_sim_topk_prenorm(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int k,
                         int mode, int64_t* idx_out, float* val_out, int32_t* fallback_rows_out, void* ws, size_t ws_bytes,
                         const void* wmax2, void* stream);
/* argmax re-classification over the K candidate names (main_unsup.py:601-614, main_ptsup.py:668-676, get_clip_preds_fast
 * main_ptsup.py:78-99): idx_out int64 [n], val_out float32 [n] = scd_sim_topk with k = 1 on the raw logits (ws: scd_sim_topk_ws_bytes(n, d, v, 1)). */
int scd_sim_argmax(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int64_t* idx_out,
                   float* val_out, void* ws, size_t ws_bytes, void* stream);
/* Which kernels the last scd_sim_topk / _prenorm / scd_sim_argmax call of this process launched (a bit set; for tests of the
 * SCD_SIM_RB / SCD_SIM_SPLIT / SCD_SIM_REFINE4 switches): exactly one of RB8 (32x32x16 row blocks, d = 512), RC16 (16x16x32 row blocks,
 * d = 512, k <= 3), TILE (d < 512), TILE768; SPLIT: the last round of row blocks was split over the vocabulary; REFINE4: the
 * four-images-per-wave refine kernel.  0 before the first call. */
enum { SCD_SIM_PATH_RB8 = 1, SCD_SIM_PATH_RC16 = 2, SCD_SIM_PATH_TILE = 4, SCD_SIM_PATH_TILE768 = 8, SCD_SIM_PATH_SPLIT = 16,
       SCD_SIM_PATH_REFINE4 = 32 };
int scd_sim_last_path(void);
/* W [r,c] fp16 -> Wt [c,r]  (zeroshot_weights [512,V] -> name-major) */
int scd_transpose_f16(scd_handle h, const void* in, int64_t r, int64_t c, void* out, void* stream);
/* out[i,:] = Wt[idx[i],:]  (the `zeroshot_weights[:, nouns.index(n)]` gather, main_unsup.py:601-602) */
int scd_gather_rows_f16(scd_handle h, const void* Wt, const int64_t* idx, int64_t m, int d, void* out, void* stream);

/* The row selections of main_unsup.py:318-321,561 (`all_feats[~mask_lab]`, `all_feats[mask_lab]`, `name_idx_top5[~mask_lab]`: numpy /
 * torch fancy indexing in the reference) in one launch: for the m rows idx[i] of F (fp16 [n,d]) out16[i] = the row, out32[i] = its
 * float32 image (the K-Means input), nidx_out[i] = name_idx[idx[i]] (int64 rows of k); any of the three outputs may be NULL. */
int scd_select_rows(scd_handle h, const void* F, const int64_t* name_idx, const int64_t* idx, int64_t m, int d, int k, void* out16,
                    float* out32, int64_t* nidx_out, void* stream);

/* out = fp16((a + b) / 2) over n_elems fp16 values (n_elems % 8 == 0): the textual-enhancement feature of BASELINE configs[4],
 * `100 * (f @ W + t @ W) / 2` (commented at main_unsup.py:518,523,604,609) = 100 * mean(f, t) @ W -> scd_sim_topk on the mean. */
int scd_mean2_f16(scd_handle h, const void* a, const void* b, int64_t n_elems, void* out, void* stream);

/* zeroshot_classifier pooling (local_utils/clip_lang_util.py:103-107): emb fp16 [n_names*t_per, d] prompt embeddings ->
 * per name normalise, mean, normalise; written as columns col0.. of out fp16 [d, ld_out] (torch.stack(dim=1) layout). */
int scd_prompt_pool(scd_handle h, const void* emb, int n_names, int t_per, int d, int64_t col0, int64_t ld_out, void* out,
                    void* stream);

/* ---- K-Means: local_utils/sskm_constrained.py, gcd/methods/clustering/faster_mix_k_means_pytorch.py ---- */
/* one-off per data set: centred, power-of-two scaled fp16 copy of X and its row norms (E-step operand).  The copy carries
 * 32 rows of padding behind row n-1 (the streaming E-step reads whole 32-row units); prep must hold
 * scd_kmeans_prep_bytes(n, d) bytes.  X and C must be 16-byte aligned (float4 loads when d % 4 == 0). */
size_t scd_kmeans_prep_bytes(int64_t n, int d);
int scd_kmeans_prepare(scd_handle h, const float* X, int64_t n, int d, void* prep, void* stream);
/* E-step: labels[i] = argmin_k ||x_i - c_k||^2, ties -> lowest k, decided on float64 values
 * (torch.min(dist,1) faster_mix_k_means_pytorch.py:140,192).  refine_rows_out (device int32, may be NULL)
 * receives the number of rows re-evaluated exactly.  D <= 768 and K <= 2048 take the streaming filter (centre prep, one
 * filter launch per 128 centres, refine), larger shapes the tiled one; the result is the same by construction. */
size_t scd_kmeans_estep_ws_bytes(int64_t n, int d, int k);
int scd_kmeans_estep(scd_handle h, const float* X, const void* prep, const float* C, int64_t n, int d, int k,
                     int32_t* labels_out, int32_t* refine_rows_out, void* ws, size_t ws_bytes, void* stream);
/* Hints for the NEXT scd_kmeans_estep on this handle (one-shot: that call consumes them whichever path it takes).  Results are
 * identical with or without them.
 *   SCD_ESTEP_FEW                     few rows are expected inside the filter's error bound (Lloyd iterations after the first two;
 *                                     converged centres): they are re-evaluated in the tail of the filter kernel instead of by a
 *                                     refine launch.  A wrong hint only costs time.
 *   SCD_ESTEP_CENTRES_FROM_FINALIZE   the caller vouches that the centres it will pass are the C_out of the last
 *                                     scd_kmeans_finalize on this handle (same buffer, NOT modified since, same E-step workspace):
 *                                     that call has already written the E-step's centre operands and the prep launch is skipped.
 *                                     Without the flag a matching pointer is not trusted (the address may have been recycled). */
/* Measurement aid (bench.py): while enabled, the streaming filter launches of every scd_kmeans_estep on this handle - stand-alone
 * or inside scd_kmeans_lloyd_step - are bracketed by HIP events on the launch stream (one pair per call; K > 128: the call's
 * kp / 128 launches together).  Each call returns and clears what was collected: the calls' durations in milliseconds, in call
 * order (the first `cap` of them), and their number; it synchronises on the recorded events. */
int scd_kmeans_timing(scd_handle h, int enable, double* samples_ms_out, int cap, int* launches_out);
#define SCD_ESTEP_FEW 1
#define SCD_ESTEP_CENTRES_FROM_FINALIZE 2
int scd_kmeans_estep_hint(scd_handle h, int flags);
/* d2_out[i] = ||x_i - c_{labels[i]}||^2 (float64 sum rounded to float32) */
int scd_kmeans_rowdist(scd_handle h, const float* X, const float* C, const int32_t* labels, int64_t n, int d, int k,
                       float* d2_out, void* stream);
/* pairwise_distance (sskm_constrained.py:189-224): out[n,k] float32 (mode 0: d2, 1: sqrt(d2)); when cost_out != NULL
 * also writes the int32 flow costs round(1000*sqrt(d2)) (:324). */
int scd_kmeans_dist(scd_handle h, const float* X, const float* C, int64_t n, int d, int k, int mode, float* out,
                    int32_t* cost_out, void* stream);
/* M-step partials (sskm_constrained.py:125-128) + inertia of the same labels against C_old (:118-120):
 * sums[k,d] float64, counts[k] int64, inertia[2] float64 = {rows < split, rows >= split}.  Partials are what a
 * multi-GPU caller all-reduces before scd_kmeans_finalize. */
size_t scd_kmeans_mstep_ws_bytes(int64_t n, int d, int k);
int scd_kmeans_mstep(scd_handle h, const float* X, const int32_t* labels, const float* C_old, int64_t n, int d, int k,
                     int64_t split, double* sums, int64_t* counts, double* inertia, void* ws, size_t ws_bytes,
                     void* stream);
/* The same partials from an fp16 copy of X (half the row bytes): valid when every value of X is exactly representable in fp16,
 * as features that left an fp16 encoder are - the float64 sums are then bit-identical.  scd_f16_exact writes the copy
 * (n_elems % 4 == 0) and counts the blocks that saw a value that does not survive the round trip (*inexact_out == 0: exact). */
int scd_f16_exact(scd_handle h, const float* X, int64_t n_elems, void* out16, int32_t* inexact_out, void* stream);
/* The same, also returning max |x| (device float; +inf when a value is infinite).  The incremental M-step's "exact sums" argument
 * (scd_kmeans_lloyd_step_delta) needs rows * max|x| * 2^24 < 2^53 on top of the exact copy: unit-scale features satisfy it by orders
 * of magnitude, fp16 values near 65504 in clusters of 2^13 rows do not - the caller checks n * max|x| < 2^29. */
int scd_f16_exact_max(scd_handle h, const float* X, int64_t n_elems, void* out16, int32_t* inexact_out, float* absmax_out, void* stream);
int scd_kmeans_mstep_f16(scd_handle h, const void* X16, const int32_t* labels, const float* C_old, int64_t n, int d, int k,
                         int64_t split, double* sums, int64_t* counts, double* inertia, void* ws, size_t ws_bytes,
                         void* stream);
/* centres = sums / counts (empty -> NaN, as torch mean of an empty selection); shift_out (device double, may be NULL)
 * = (sum_k ||c_k - c_old_k||_2)^2  (shift_mode 0: sskm_constrained.py:135-136) or sum_k ||c_k - c_old_k||^2 (shift_mode 1:
 * sklearn's center_shift_tot, the `--cluster KM` path of main_unsup.py:362) */
int scd_kmeans_finalize(scd_handle h, const double* sums, const int64_t* counts, int k, int d, const float* C_old,
                        float* C_out, double* shift_out, int shift_mode, const void* prep, void* estep_ws,
                        size_t estep_ws_bytes, int64_t n, void* stream);
/* One whole Lloyd iteration of the unconstrained K-Means (faster_mix_k_means_pytorch.py:187-214) = scd_kmeans_estep on the n_u
 * unlabelled rows (labels_cat[n_cat - n_u ...] written; the first n_cat - n_u entries are the labelled rows' fixed cluster ids) +
 * scd_kmeans_mstep[_f16] over the n_cat rows [labelled ; unlabelled] (X16_cat: their exact fp16 copy, or NULL) + scd_kmeans_finalize
 * with the hand-over of the next E-step's centre operands, behind one call.  stats: device double [4] = {inertia labelled,
 * inertia unlabelled, centre shift, rows the E-step re-evaluated exactly}.  `expect_few`: SCD_ESTEP_* flags for this step's
 * E-step.  C_out must differ from C_in; ws_e / ws_m as for the single calls. */
int scd_kmeans_lloyd_step(scd_handle h, const float* X_u, const void* prep_u, int64_t n_u, const float* X_cat,
                          const void* X16_cat, int64_t n_cat, int d, int k, int32_t* labels_cat, const float* C_in,
                          float* C_out, double* sums, int64_t* counts, double* stats, int expect_few, void* ws_e,
                          size_t ws_e_bytes, void* ws_m, size_t ws_m_bytes, void* stream);
/* The same iteration with an INCREMENTAL M-step, for row sets whose exact fp16 copy exists (scd_f16_exact: then the float64
 * cluster sums are exact, hence independent of the order of additions): sums / counts of the previous iteration are updated with
 * the rows whose label changed (labels_prev: the labels sums / counts belong to, updated in place) and the inertia is evaluated
 * from the sums, the centres and the rows' sum of squares (scd_kmeans_sumsq, double-double) - bit-identical centres, labels and
 * float32 inertia at a cost proportional to the changes.  flags: SCD_ESTEP_* | SCD_LLOYD_FULL (a fresh M-step over the rows, as
 * scd_kmeans_lloyd_step; the first iterations of a restart, or whenever many labels move).  sums_lab / counts_lab: sums / counts of
 * the labelled rows alone (NULL when there are none).  stats: device double [5] = {inertia labelled, inertia unlabelled, centre
 * shift, rows re-evaluated exactly, rows whose label changed}.  Reference: faster_mix_k_means_pytorch.py:187-214. */
#define SCD_LLOYD_FULL 8
/* (scd_kmeans_sumsq reads the rows as one flat array with 16-byte loads: the base pointer must be 16-byte aligned - an unaligned one is
 * refused with SCD_EINVAL; n, d and split are free.) */
int scd_kmeans_sumsq(scd_handle h, const void* X16, const float* X, int64_t n, int d, int64_t split, double* out4, void* stream);
int scd_kmeans_lloyd_step_delta(scd_handle h, const float* X_u, const void* prep_u, int64_t n_u, const void* X16_cat,
                                int64_t n_cat, int d, int k, int32_t* labels_cat, int32_t* labels_prev, const float* C_in,
                                float* C_out, double* sums, int64_t* counts, const double* sums_lab, const int64_t* counts_lab,
                                const double* sumsq4, double* stats, int flags, void* ws_e, size_t ws_e_bytes, void* ws_m,
                                size_t ws_m_bytes, void* stream);
/* One restart's whole Lloyd loop behind one call (faster_mix_k_means_pytorch.py:187-214: up to max_iter iterations of
 * scd_kmeans_lloyd_step_delta from C_start, stop after the iteration whose centre shift is below tol, keep the labels / centres of
 * the iteration with the least float32 inertia).  The host stays one iteration behind the device (iteration i + 1 is enqueued
 * before iteration i's statistics are looked at; a speculative iteration behind a converged one is dropped); the statistics reach
 * the host through pinned memory written by the iteration's last kernel, so nothing but the iterations' kernels enters the stream.
 * Caller-owned device rings: lab_ring int32 [3][n_cat] (iteration i's labels in slot i % 3; labels_lab = the n_cat - n_u labelled
 * rows' labels, NULL when there are none), C_ring float [3][k,d], stats_ring double [2][5].  Outputs: best_labels int32 [n_cat] and
 * best_C [k,d] on the device (valid in stream order), result_host (HOST double [4]) = {least inertia, iterations done, iterations
 * with the incremental M-step, iterations launched}.  Returns when the last iteration's statistics have arrived.
 * An iteration whose M-step leaves a cluster without rows ends the restart the way the reference's loop does (:140-160, :192-214: that
 * centre is NaN, `torch.min` then yields NaN at the first NaN column for every row, so no later iteration is ever the best or ends the
 * loop): the best of the iterations so far is kept - its centres carry NaN rows if it is that iteration - and "iterations done" is
 * max_iter.  The one configuration in which the reference's loop can recover (exactly one cluster without labelled rows) is the
 * caller's to route elsewhere (scd_amd/kmeans.py does). */
int scd_kmeans_lloyd_run(scd_handle h, const float* X_u, const void* prep_u, int64_t n_u, const void* X16_cat, int64_t n_cat, int d,
                         int k, const int32_t* labels_lab, int32_t* lab_ring, int32_t* labels_prev, const float* C_start,
                         float* C_ring, double* sums, int64_t* counts, const double* sums_lab, const int64_t* counts_lab,
                         const double* sumsq4, double* stats_ring, int max_iter, double tol, int32_t* best_labels, float* best_C,
                         double* result_host, void* ws_e, size_t ws_e_bytes, void* ws_m, size_t ws_m_bytes, void* stream);
/* The same loop over a ROW SHARD, one process per GPU (the reference is single-process): X_u / X16_cat / labels are this
 * rank's rows, sums_lab / counts_lab / sumsq4 the GLOBAL ones (reduced by the caller once per fit).  Every iteration packs the rank's
 * [k*d sums | k counts as float64] into xbuf (device, k*d + 2k doubles) and calls exchange(exchange_ctx, xbuf, k*d + k, stream), which
 * must leave the element-wise sum over all ranks in xbuf in stream order (an all-reduce; scd_allreduce_centroids has this signature
 * with ctx = the handle, a torch.distributed caller passes a callback around dist.all_reduce) and return 0.  Centres, centre shift
 * and inertia are then formed from the global sums, so every rank takes the same stop / keep decisions and issues the same number of
 * exchanges; with exact sums (scd_f16_exact_max: GLOBAL rows x max|x| < 2^29) the result is bit-identical to the single-process
 * loop whatever the sharding.  The fresh-or-incremental M-step choice and the E-step hints are per rank.  Needs n_u > 0 on every
 * rank.  A non-zero return of the callback ends the loop with SCD_ERCCL. */
typedef int (*scd_exchange_fn)(void* ctx, double* buf, int64_t n_doubles, void* stream);
int scd_kmeans_lloyd_run_sharded(scd_handle h, const float* X_u, const void* prep_u, int64_t n_u, const void* X16_cat, int64_t n_cat,
                                 int d, int k, const int32_t* labels_lab, int32_t* lab_ring, int32_t* labels_prev, const float* C_start,
                                 float* C_ring, double* sums, int64_t* counts, const double* sums_lab, const int64_t* counts_lab,
                                 const double* sumsq4, double* stats_ring, int max_iter, double tol, int32_t* best_labels, float* best_C,
                                 double* result_host, void* ws_e, size_t ws_e_bytes, void* ws_m, size_t ws_m_bytes, void* stream,
                                 double* xbuf, scd_exchange_fn exchange, void* exchange_ctx);
/* ALL restarts of a fit in lock-step (faster_mix_k_means_pytorch.py:244-275: the n_init restarts are independent once seeded): iteration
 * i of every restart still running is enqueued, then iteration i - 1 of each is settled; a restart that has converged drops out.  Every
 * restart executes exactly the launches of scd_kmeans_lloyd_run with the same arguments, so its outputs are the same bits.  restarts[j]
 * = restart j's own handle (scratch, centre hand-over and statistics ring are per handle: R distinct handles of the current device) and
 * buffers - the per-restart arguments of scd_kmeans_lloyd_run, with E-step / M-step workspaces of its own; the rest is shared.
 * xbuf / exchange NULL: one process.  Otherwise a row shard as in scd_kmeans_lloyd_run_sharded, with ONE exchange per iteration for all
 * restarts: xbuf holds R * (k*d + 2k) doubles, the call is exchange(ctx, xbuf, (restarts still running) * (k*d + k), stream) with the
 * running restarts' [k*d sums | k counts] packed densely in restart order (the same set on every rank: the stop decisions come from
 * exchanged statistics) - R times fewer collectives per fit than one run per restart.
 * n_streams > 1: the restarts' launches are spread over that many library-owned streams, ordered behind what `stream` already holds;
 * `stream` continues behind all of them (under a group the exchange itself stays on `stream`). */
typedef struct scd_lloyd_restart {
    scd_handle h;
    int32_t* lab_ring;        /* [3][n_cat] */
    int32_t* labels_prev;     /* [n_cat] */
    const float* C_start;     /* [k][d] the seeding */
    float* C_ring;            /* [3][k][d] */
    double* sums;             /* [k][d] */
    int64_t* counts;          /* [k] */
    double* stats_ring;       /* [2][5] */
    int32_t* best_labels;     /* out [n_cat] */
    float* best_C;            /* out [k][d] */
    double* result_host;      /* out, host [4]: float32 inertia, iterations done, incremental iterations, iterations launched */
    void* ws_e;               /* scd_kmeans_estep_ws_bytes */
    void* ws_m;               /* scd_kmeans_mstep_ws_bytes */
} scd_lloyd_restart;
int scd_kmeans_lloyd_run_multi(const scd_lloyd_restart* restarts, int R, const float* X_u, const void* prep_u, int64_t n_u,
                               const void* X16_cat, int64_t n_cat, int d, int k, const int32_t* labels_lab, const double* sums_lab,
                               const int64_t* counts_lab, const double* sumsq4, int max_iter, double tol, size_t ws_e_bytes,
                               size_t ws_m_bytes, void* stream, double* xbuf, scd_exchange_fn exchange, void* exchange_ctx, int n_streams);

/* The lock-step k-means++ rounds of scd_kpp_seed_lockstep over a ROW SHARD (one process per GPU; sskm_constrained.py:28-44 is
 * single-process): per round three exchanges - shard sums, shard probability masses, candidate rows - each an all-gather of a few bytes
 * per restart through `gather(gather_ctx, send, recv, bytes_per_rank, stream)`: rank w's `bytes_per_rank` bytes at `send` must arrive at
 * recv + w * bytes_per_rank on every rank, in stream order; send / recv lie inside xbuf (device, scd_kpp_seed_sharded_xbuf_bytes).  The
 * new centres are the rows of their first owner in rank order (float32 values of the global X), written to C_buf[r][m0 + t]; picks_out
 * int64 [T][R] = 0, or -1 where no shard reported a hit (the reference indexes an empty nonzero() there).  d2 float [R][ld]: this
 * shard's closest squared distances, updated in place; r_dev float [T][R]: the restarts' uniforms; ws: scd_kpp_seed_sharded_ws_bytes.
 * X16 (may be NULL): this shard's exact fp16 copy - the update then goes through the MFMA filter as in scd_kpp_seed_lockstep.
 * Every rank needs at least one row (n > 0) and must make the call (three gathers per round, T rounds).  A non-zero return of the
 * callback ends the loop with SCD_ERCCL. */
typedef int (*scd_gather_fn)(void* ctx, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
size_t scd_kpp_seed_sharded_ws_bytes(int64_t n, int d, int R);
size_t scd_kpp_seed_sharded_xbuf_bytes(int d, int R, int world);
int scd_kpp_seed_lockstep_sharded(scd_handle h, const float* X, const void* X16, int64_t n, int d, int R, float* d2, int64_t ld,
                                  const float* r_dev, int T, float* C_buf, int k, int m0, int64_t* picks_out, void* ws, size_t ws_bytes,
                                  void* stream, void* xbuf, size_t xbuf_bytes, scd_gather_fn gather, void* gather_ctx, int rank, int world);
/* prep / estep_ws (both may be NULL): the data set's scd_kmeans_prepare buffer and the workspace the NEXT scd_kmeans_estep
 * of these centres will be given (n = its row count).  The blocks that produce the centres then also write their E-step
 * operands into it, and that E-step - same handle, same C_out pointer, same workspace, C_out unmodified in between - skips
 * its centre-prep launch.  Any other scd_kmeans_finalize / scd_kmeans_estep call on the handle drops the hand-over. */
/* sklearn.cluster.KMeans pieces (main_unsup.py:362, main_ptsup.py:381 `KMeans(n_clusters, random_state=0).fit(u_feats)`):
 * out (device int64) = number of rows whose label changed (strict convergence, `np.array_equal(labels, labels_old)`); */
int scd_labels_changed(scd_handle h, const int32_t* a, const int32_t* b, int64_t n, int64_t* out, void* stream);
/* the greedy k-means++ candidate draw: idx_out[l] = searchsorted(cumsum_f64(d2), u[l] * float32(sum d2)) clipped to n-1 for
 * l < n_draws (u: device doubles, the host RandomState's uniforms); pot_out (device double, may be NULL) = sum d2.
 * ws: scd_kpp_draw_ws_bytes(n). */
int scd_kpp_searchsorted(scd_handle h, const float* d2, int64_t n, const double* u, int n_draws, int64_t* idx_out,
                         double* pot_out, void* ws, size_t ws_bytes, void* stream);
/* The same greedy seeding for the R = n_init starts of a fit in lock-step, the rounds in C (the starts share X; each owns a fixed
 * slice of the host RandomState's stream: its first centre, then L = 2 + int(ln k) uniforms per added centre - `_k_init` of the
 * scikit-learn the reference vendors, local_utils/k_means_constrained/sklearn_import/cluster/k_means_.py:33-132, = `_kmeans_plusplus`
 * of the pinned 1.0.2).  first: device int64 [R] rows of the first centres; u: device double [k-1][R][L]; C_buf float [R][k][d] and
 * picks_out int64 [k][R] receive the centres and their row indices.  X16: the exact fp16 copy of X (scd_f16_exact) or NULL: with it
 * the R * L candidates of a round are measured through the MFMA lower-bound filter of scd_kpp_seed_lockstep, without it densely -
 * the same potentials (float64 sums of float32(float64-exact) distances), the same picks. */
size_t scd_kpp_greedy_ws_bytes(int64_t n, int d, int R, int L);
int scd_kpp_greedy_lockstep(scd_handle h, const float* X, const void* X16, int64_t n, int d, int R, int L, int k, const int64_t* first,
                            const double* u, float* C_buf, int64_t* picks_out, void* ws, size_t ws_bytes, void* stream);
/* sklearn's `_kmeans_single_lloyd` behind one call, for rows with an exact fp16 copy (the Lloyd loop of `KMeans.fit`, main_unsup.py:362):
 * iterations of scd_kmeans_lloyd_step_delta with sklearn's centre shift (sum_k ||dc_k||^2) from C_start until no label changes
 * (never at the first iteration) or the shift is <= tol or max_iter is reached, then the E-step of the final centres.  The host stays
 * one iteration behind the device as in scd_kmeans_lloyd_run (same rings: lab_ring int32 [3][n], C_ring float [3][k,d], stats_ring
 * double [2][5]; labels_prev int32 [n]).  final_labels int32 [n], final_C [k,d] (device, valid in stream order).  result_host (HOST
 * double [4]) = {status, n_iter, iterations with the incremental M-step, iterations launched}; status 1: an iteration left a cluster
 * empty - sklearn re-seeds it with a far point (`_relocate_empty_clusters_dense`), the caller runs that start itself. */
int scd_kmeans_lloyd_run_sk(scd_handle h, const float* X, const void* prep, int64_t n, const void* X16, int d, int k, int32_t* lab_ring,
                            int32_t* labels_prev, const float* C_start, float* C_ring, double* sums, int64_t* counts,
                            const double* sumsq4, double* stats_ring, int max_iter, double tol, int32_t* final_labels, float* final_C,
                            double* result_host, void* ws_e, size_t ws_e_bytes, void* ws_m, size_t ws_m_bytes, void* stream);
/* incremental k-means++ (kpp, sskm_constrained.py:28-44): d2 = min(d2, ||x - c_new||^2) */
int scd_kmeans_min_update(scd_handle h, const float* X, const float* c_new, int64_t n, int d, float* d2_inout,
                          void* stream);
/* one draw: prob = d2/float32(total); first i with float32(prefix + cumsum_f64(prob))[i] >= r; idx_out device int64
 * (-1: none on this shard).  total / prefix (device doubles, may be NULL = local sum / 0) make the draw shard-aware for
 * multi-GPU k-means++; probsum_out (device double, may be NULL) receives this shard's sum of prob. */
size_t scd_kpp_draw_ws_bytes(int64_t n);
int scd_kpp_draw(scd_handle h, const float* d2, int64_t n, float r, const double* total, const double* prefix,
                 int64_t* idx_out, double* probsum_out, void* ws, size_t ws_bytes, void* stream);
/* The same for R restarts in lock-step (the n_init restarts of one fit share X and a fixed random stream): d2 [R][ld] (ld >= n),
 * c_new [R][d], r_dev device float [R], total / prefix / idx_out / probsum_out device arrays of R (or NULL as above).  X is read
 * once per round instead of R times; ws: R * scd_kpp_draw_ws_bytes(n).  scd_sum_f32_multi: out[r] = float64 sum of row r. */
int scd_kmeans_min_update_multi(scd_handle h, const float* X, const float* c_new, int64_t n, int d, int R, float* d2_inout,
                                int64_t ld, void* stream);
int scd_kpp_draw_multi(scd_handle h, const float* d2, int64_t n, int64_t ld, int R, const float* r_dev, const double* total,
                       const double* prefix, int64_t* idx_out, double* probsum_out, void* ws, size_t ws_bytes, void* stream);
int scd_sum_f32_multi(scd_handle h, const float* x, int64_t n, int64_t ld, int R, double* out, void* stream);
/* The rounds of the lock-step seeding behind one call (kpp of sskm_constrained.py:28-44 for R restarts at once): for t < T: draw
 * one row per restart from d2 with the uniforms r_dev[t][R] (scd_kpp_draw_multi), store it as centre m0 + t of C_buf [R][k][d],
 * d2[r] = min(d2[r], ||x - that row||^2).  On entry d2 [R][ld] holds the distances to the m0 centres chosen so far.  picks_out
 * int64 [T][R] on the device (-1: no row drawn; the reference raises there).  X16: the exact fp16 copy of X (scd_f16_exact) or
 * NULL: with it the distance update reads 2 bytes per value through a filter (16x16x32 MFMA lower bounds rule out the rows a new
 * centre cannot improve, the rest get the float64 value) - the same float32 results as scd_kmeans_min_update_multi. */
size_t scd_kpp_seed_ws_bytes(int64_t n, int d, int R);
int scd_kpp_seed_lockstep(scd_handle h, const float* X, const void* X16, int64_t n, int d, int R, float* d2, int64_t ld,
                          const float* r_dev, int T, float* C_buf, int k, int m0, int64_t* picks_out, void* ws, size_t ws_bytes,
                          void* stream);
/* One round's distance update of the lock-step seeding through that filter, as a call of its own: d2[r] = min(d2[r], ||x - c_new[r]||^2),
 * r < R <= 16, c_new [R][d] float32 (rows of the global X), X16 = the exact fp16 copy of this rank's rows.  Same float32 results as
 * scd_kmeans_min_update_multi.  For callers whose rounds cannot run behind scd_kpp_seed_lockstep: under a process group three
 * all-gathers sit between a round's draw and its update.  ws keeps the rows' norm table between calls:
 * first_call != 0 (re)builds it - pass it on the first update of a seeding. */
size_t scd_kpp_update_ws_bytes(int64_t n, int d);
int scd_kpp_update_filter(scd_handle h, const void* X16, int64_t n, int d, int R, const float* c_new, float* d2, int64_t ld,
                          int first_call, void* ws, size_t ws_bytes, void* stream);
/* deterministic float64 sum of a float32 vector (inertia, d2.sum()) */
int scd_sum_f32(scd_handle h, const float* x, int64_t n, double* out, void* stream);

/* ---- vote histogram: Counter(...).most_common(m) per cluster, main_unsup.py:573-586, main_ptsup.py:636-648.
 * name_idx int64 [n, ld] (first top_k columns used); preds int64 [n]; clusters int64 [n_clusters] (ids to vote for);
 * known int64 [n_known] vocabulary ids to drop (may be NULL).  Output per cluster c: keys_out[c, 0..m) and
 * counts_out[c, 0..m) in most_common order (count desc, first-seen asc), padded with -1 / 0.
 * Limits, from the 64-bit sort keys (cluster slot 16 bits | name 24 bits | position 24 bits, then slot | count 24 bits | position):
 * n_clusters <= 65,536 and cluster ids in [0, 65,536) - an id of `clusters` outside it gets an all-padding row, a prediction outside
 * it votes for nothing (the Python wrapper refuses such ids in `clusters`); names in [0, 2^24) - a name outside it is dropped like a
 * `known` one; n * top_k < 2^24 (refused otherwise), which also bounds every count. */
size_t scd_vote_hist_ws_bytes(int64_t n, int top_k);
int scd_vote_hist(scd_handle h, const int64_t* name_idx, int64_t n, int ld, int top_k, const int64_t* preds,
                  const int64_t* clusters, int n_clusters, const int64_t* known, int n_known, int m,
                  int64_t* keys_out, int32_t* counts_out, void* ws, size_t ws_bytes, void* stream);
/* The histogram over row SHARDS (one process per GPU).  scd_vote_table: this rank's dense tables counts int32 [C, V]
 * (occurrences of a name among the first top_k columns of the rows predicted as cluster c) and first int64 [C, V] (smallest
 * (row_offset + row) * top_k + column at which it occurs; 0x7f7f7f7f7f7f7f7f = never) - slot_of int32 [n_slots] maps a prediction to its
 * table row (-1: not voted on).  The caller all-reduces counts with SUM and first with MIN over the ranks;
 * scd_vote_table_topm then reads most_common(m) of every cluster off the reduced tables, (count desc, first asc) - the order of
 * Counter.most_common on the concatenated rows (main_unsup.py:573-586).  Limits: scd_vote_table skips names outside [0, v) and
 * predictions outside [0, n_slots) or with slot -1, and refuses top_k > ld and (row_offset + n) * top_k >= 2^40; scd_vote_table_topm
 * compares the whole int32 count (up to 2^31 - 1; cells <= 0 are empty) and the whole 64-bit first.  SIDE EFFECT: scd_vote_table_topm
 * zeroes the counts it takes (the cells it reports) and leaves every other cell and `first` as they are. */
int scd_vote_table(scd_handle h, const int64_t* name_idx, int64_t n, int ld, int top_k, const int64_t* preds, const int32_t* slot_of,
                   int n_slots, int64_t row_offset, int64_t v, int n_clusters, int32_t* counts, int64_t* first, void* stream);
int scd_vote_table_topm(scd_handle h, int32_t* counts, const int64_t* first, int n_clusters, int64_t v, int m, int64_t* keys_out,
                        int32_t* counts_out, void* stream);

/* ---- clustering scores: the contingency table of a clustering against targets and the statistics ACC / NMI / ARI / purity are
 * computed from.  scd_contingency replaces the counting loop of cluster_acc (gcd/project_utils/cluster_utils.py:39-62:
 * `w[y_pred[i], y_true[i]] += 1`) and the `contingency_matrix` sklearn builds inside nmi_score / ari_score / purity_score
 * (cluster_utils.py:65-69); with `subset` it builds the tables of the labelled and of the unlabelled rows, which one evaluation of
 * GCD's estimator scores separately (gcd/methods/estimate_k/estimate_k.py:87-94: `[mask]` / `[~mask]`), in one pass.
 * pred, truth int32 [n]; subset uint8 [n] or NULL; table_out int32 [S, kp, kt] with S = 1 (subset NULL) or 2: row i adds one to
 * table (subset[i] != 0 ? 0 : 1), cell (pred[i], truth[i]).  A row with pred outside [0, kp) or truth outside [0, kt) is counted in
 * n_bad_out (int64 [1]) and in no table.  Both outputs are zeroed by the call.  Integer counts: exact, whatever the arrival order.
 * Two kernels: up to scd_contingency_private_cells() cells (S * kp * kt; the table as uint32 in one block's LDS) every block counts a
 * contiguous row range in LDS and adds its non-zero cells to the table; above that, one global integer add per row.
 * scd_contingency_last_path: which of them the handle's last scd_contingency launched (-1 before the first call). */
enum { SCD_CONTINGENCY_PRIVATE = 0, SCD_CONTINGENCY_GLOBAL = 1 };
size_t scd_contingency_private_cells(void);
int scd_contingency(scd_handle h, const int32_t* pred, const int32_t* truth, const uint8_t* subset, int64_t n, int kp, int kt,
                    int32_t* table_out, int64_t* n_bad_out, void* stream);
int scd_contingency_last_path(scd_handle h);
/* The statistics of S tables int32 [S, kp, kt] (non-negative cells, fewer than 2^31 rows per table), a kernel of its own so that
 * ranks can add their tables first.  ints_out int64 [S, 6]: n, sum n_ij^2, sum a_i^2 (a: row sums, the predictions), sum b_j^2
 * (b: column sums, the targets), sum_i max_j n_ij (the purity numerator, cluster_utils.py:65-69), the number of non-zero cells - all
 * exact.  info_out float64 [S, 3]: H(pred), H(truth) and the mutual information in nats, term by term as sklearn's `entropy` and
 * `mutual_info_score` form them (terms below 2^-52 in magnitude count as 0), summed over a fixed strided partition and a fixed tree:
 * bit-identical from call to call.  An empty table gives zeros. */
size_t scd_contingency_stats_ws_bytes(int s, int kp, int kt);
int scd_contingency_stats(scd_handle h, const int32_t* table, int s, int kp, int kt, int64_t* ints_out, double* info_out, void* ws,
                          size_t ws_bytes, void* stream);

/* ---- silhouette coefficients: sklearn.metrics.silhouette_samples(X, labels, metric='euclidean') and their mean, the label-free
 * criterion of the search for the number of categories (docs/design/estimate_k.md).  X [n, d] (SCD_F32 or SCD_F16), labels int32 [n].
 * Row i: a = the mean distance to the OTHER rows of its cluster (the sum runs over the cluster, the pair i = i contributes exactly 0,
 * divided by cnt - 1), b = the smallest mean distance to the rows of another non-empty cluster, s = (b - a) / max(a, b); s = 0 in a
 * singleton cluster and when max(a, b) = 0.  Label ids without rows are skipped.  samples_out float [n] in the caller's row order,
 * mean_out double [1] = their mean, info_out int64 [2] = {rows with a label outside [0, k) - they take part in nothing and get s = 0;
 * the number of non-empty clusters}.  With fewer than two non-empty clusters the outputs are zeros and the call returns SCD_OK.
 * Arithmetic: rows as fp16 (fp32 input rounded to nearest even), dots accumulated in fp32 by MFMA, dist^2 = max(0, |x_i|^2 + |x_j|^2 -
 * 2 dot) with the fp32 norms of the fp16 rows, the pair i = j excluded by index, per-cluster sums in fp32, the mean in float64 over a
 * fixed partition and tree.  No floating-point atomics: two calls on one input return the same bits.
 * Limits: 2 <= n <= 2^30, 1 <= d <= 1024, 2 <= k <= n; scd_silhouette_ws_bytes returns 0 outside them.  The workspace holds the
 * label-sorted fp16 copy of X: about 2 n (d rounded up to 64) bytes.
 * scd_silhouette_ranges: the number of cluster ranges (grid.y, 1 ... 32) scd_silhouette launches with for n rows and k ids on this
 * handle's device: min(k, 32, ceil(4 CUs / ceil(n / 128))).  Read-only; the samples do not depend on it.  0 for a null handle or
 * n, k outside the limits. */
size_t scd_silhouette_ws_bytes(int64_t n, int d, int k);
int scd_silhouette_ranges(scd_handle h, int64_t n, int k);
int scd_silhouette(scd_handle h, const void* X, int x_dtype, const int32_t* labels, int64_t n, int d, int k, float* samples_out,
                   double* mean_out, int64_t* info_out, void* ws, size_t ws_bytes, void* stream);

/* ---- FINCH first-neighbour clustering, cosine distance (local_utils/finch.py; docs/design/finch.md) ---- */
/* clust_rank's first neighbours (finch.py:24-27) without the n x n matrix: nn_out[i] = argmax over j != i of dot(U_i, U_j), the dot
 * taken in float64 on the fp32 rows U [n, d], ties to the lowest j (fill_diagonal + argmin); d1_out[i] = 1 - that dot (float64).  U need
 * not be unit.  An fp16 MFMA pass with an error bound computed from the rows filters the columns, float64 decides; a row whose
 * certificate fails takes an exact pass over all columns.  info_out int32 [2] = {rows that took the exact full-row pass, 1 if a value did
 * not fit fp16 (then every row takes it)}.  The result never depends on the filter; two calls return the same bits.
 * Limits: 2 <= n < 2^31 (n = 1: SCD_EINVAL), 1 <= d with d rounded up to 32 <= 1024; scd_first_neighbor_ws_bytes returns 0 outside
 * them.  The workspace holds the fp16 copy of U: about 2 n (d rounded up to 64) bytes, plus 132 bytes per row and column range. */
size_t scd_first_neighbor_ws_bytes(int64_t n, int d);
int scd_first_neighbor(scd_handle h, const float* U, int64_t n, int d, int32_t* nn_out, double* d1_out, int32_t* info_out, void* ws,
                       size_t ws_bytes, void* stream);
/* out[p] = 1 - float64 dot of rows a[p] and b[p] of U [n, d] (the same dot as scd_first_neighbor's): the distances between rows that share
 * a first neighbour (min_sim, finch.py:138-139) and across a cut mutual pair (:49-50).  A pair with an index outside [0, n) gives NaN. */
int scd_pair_dist_f64(scd_handle h, const float* U, int64_t n, int d, const int32_t* a, const int32_t* b, int64_t m, double* out,
                      void* stream);
/* get_clust's connected_components (finch.py:52) on an undirected edge list (ea[e], eb[e]), e < m: labels_out int32 [n] numbered by the
 * rank of each component's lowest member (scipy's order), ncomp_out int32 [1].  Hooking onto the smaller index and pointer jumping until
 * a device-side change flag stays clear; integers only, the result does not depend on the order of the steps.  Synchronises the stream
 * (it reads the flag).  An edge end outside [0, n) is SCD_EINVAL.  m = 0 gives n singletons. */
size_t scd_link_components_ws_bytes(int64_t n);
int scd_link_components(scd_handle h, int64_t n, const int32_t* ea, const int32_t* eb, int64_t m, int32_t* labels_out, int32_t* ncomp_out,
                        void* ws, size_t ws_bytes, void* stream);
/* cool_mean (finch.py:56-69) for k segments: segment c holds the rows order[offsets[c] .. offsets[c + 1]) of X [n, d] (order: the stable
 * sort of the rows by label).  mean_out[c] = the float64 sum of those rows in that order, divided by the count, rounded to fp32;
 * unit_out[c] = the mean divided by its norm (taken in float64), the next level's rows; a zero mean stays zero. */
int scd_segment_mean_unit(scd_handle h, const float* X, int64_t n, const int32_t* order, const int64_t* offsets, int k, int d,
                          float* mean_out, float* unit_out, void* stream);

/* ---- exact k nearest neighbours under the inner product, and the k-NN vote (no counterpart in the reference; the weighted k-NN protocol
 * of DINO, Caron et al., ICCV 2021, section 4.1, and scikit-learn's NearestNeighbors(metric='cosine', algorithm='brute') /
 * KNeighborsClassifier on unit rows; docs/design/knn.md) ---- */
/* Queries Q [m, d] and base rows X [n, d], float32.  For query i: the k admissible columns j with the largest dot(Q_i, X_j), the dot taken
 * in float64 on the fp32 rows (scd_first_neighbor's and scd_pair_dist_f64's dot: a pair has one value everywhere), ordered by (value
 * descending, column ascending); a tie at the k-th place goes to the lower column.  self_base: -1, or the row of X that query 0 is
 * (0 <= self_base, self_base + m <= n); query i then never returns column self_base + i.  Q = X with self_base = 0 is the k-NN graph,
 * Q = X + a * d with self_base = a a row shard of it.  idx_out int32 [m, k], dot_out double [m, k], info_out int32 [4] = {rows that took
 * the exact full-row pass, 1 if a value did not fit fp16 (then every row takes it), rows whose candidate slots overflowed, the largest
 * candidate count of a row}.  Two fp16 MFMA passes with an error bound computed from the rows propose candidates, float64 decides; the
 * result never depends on them; two calls return the same bits.  Inputs must be finite.  Cosine k-NN is this call on unit rows.
 * Limits: 1 <= m < 2^31, 2 <= n < 2^31, d rounded up to 32 <= 1024, 1 <= k <= 64 and k <= the admissible columns (n, or n - 1 with
 * self_base >= 0); scd_knn_ws_bytes returns 0 outside them.  The workspace holds the fp16 copies of X and Q and scd_knn_slots() int32
 * candidate slots per query: 0.69 GB at m = n = 126,976, d = 768, k = 20. */
size_t scd_knn_ws_bytes(int64_t m, int64_t n, int d, int k);
int scd_knn_slots(void);
int scd_knn(scd_handle h, const float* Q, int64_t m, const float* X, int64_t n, int d, int k, int64_t self_base, int32_t* idx_out,
            double* dot_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream);
/* The vote of the first k_use neighbours of each query (idx int32 [m, k_stride] and dot double [m, k_stride] as scd_knn returns them)
 * with the labels base_labels int32 [n] of the base rows.  mode 0, uniform: the class with the most neighbours, ties to the lowest class
 * (KNeighborsClassifier(weights='uniform')); score_out = the count.  mode 1, softmax: class score = the sum over its neighbours, in
 * neighbour order, of exp((dot_j - dot_0) / temperature) in float64, the largest wins, ties to the lowest class.  A neighbour with a
 * negative label or an index outside [0, n) does not vote; a query without a voting neighbour gets pred_out = -1 and score_out = 0.
 * Any label range: no per-class table, O(k_use^2) work per query. */
int scd_knn_vote(scd_handle h, const int32_t* idx, const double* dot, int64_t m, int k_stride, int k_use, const int32_t* base_labels,
                 int64_t n, int mode, double temperature, int32_t* pred_out, double* score_out, void* stream);

/* ---- HDBSCAN on unit rows (no counterpart in the reference; scikit-learn 1.7.2's sklearn.cluster.HDBSCAN(metric='euclidean',
 *      algorithm='brute'); docs/design/hdbscan.md) ---- */
/* One Boruvka round of the minimum spanning tree of the mutual-reachability graph, without the n x n matrix that
 * sklearn/cluster/_hdbscan/_reachability.pyx (mutual_reachability_graph) and hdbscan.py:_brute_mst build.  U float32 [n, d], core double
 * [n] (the core dot of each row: the float64 dot with its (min_samples - 1)-th nearest other row, or +inf), comp int32 [n] (any values:
 * the component of each row).  With v_ij the float64 dot of rows i and j (scd_knn's) and r_ij = min(core_i, core_j, v_ij):
 * nn_out[i] = the column j with comp[j] != comp[i] of the largest r_ij, ties to the lowest j; r_out[i] = that r_ij (double); a row without
 * a foreign column gets -1 and -inf.  info_out int32 [4] as scd_knn's.  Two fp16 MFMA passes with an error bound computed from the rows
 * propose candidates, float64 decides; the result never depends on them; two calls return the same bits.
 * prepared: 0 makes the fp16 copy of U and its row statistics in the workspace; 1 says the workspace still holds them from an earlier
 * call with this U, n and d (the rounds of one fit).  Limits: 2 <= n < 2^31, d rounded up to 32 <= 1024; scd_mr_nearest_ws_bytes returns 0
 * outside them.  The workspace holds the fp16 copy of U and scd_knn_slots() int32 slots per row: 0.47 GB at n = 126,976, d = 768. */
size_t scd_mr_nearest_ws_bytes(int64_t n, int d);
int scd_mr_nearest(scd_handle h, const float* U, int64_t n, int d, const double* core, const int32_t* comp, int prepared, int32_t* nn_out,
                   double* r_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream);
/* HOST.  _linkage.pyx:make_single_linkage and _tree.pyx:tree_to_labels (_condense_tree, _compute_stability, _get_clusters, _do_labelling,
 * get_probabilities; cluster_selection_epsilon = 0, max_cluster_size = None) on the n - 1 edges (lo[e], hi[e], weight[e]) of a spanning
 * tree in the order given (sorted by weight ascending; edge e joins as current_node = lo, next_node = hi): lambda = 1 / weight, +inf at
 * weight 0.  method 0 = 'eom', 1 = 'leaf'.  labels_out int32 [n] (noise = -1, clusters numbered as scikit-learn numbers them), prob_out
 * double [n], n_clusters_out int32 [1].  SCD_EINVAL: n < 2, min_cluster_size < 2, an index outside [0, n), edges that form no spanning
 * tree, a NaN weight.  No recursion: a path-shaped tree costs no stack. */
int scd_hdbscan_tree(const int32_t* lo, const int32_t* hi, const double* weight, int64_t n, int min_cluster_size, int method,
                     int allow_single_cluster, int32_t* labels_out, double* prob_out, int32_t* n_clusters_out);

/* ---- Ward agglomerative clustering (no counterpart in the reference; scipy's linkage(x, 'ward') and scikit-learn's
 *      AgglomerativeClustering(linkage='ward'); docs/design/ward.md) ---- */
/* The nearest-neighbour search of one round of the reciprocal-pair procedure, without the n x n matrix.  The table is X float32 [m, d]
 * (centroids) with xcnt int32 [m] (sizes); a position of size 0 is dead.  Query p is the row Q_p of Q float32 [q, d] with size qcnt[p]
 * >= 1 and qself[p], the column that is the query itself, or -1.  With qn = the float64 dot of a row with itself and v_pj the float64
 * dot of Q_p and X_j (scd_knn's), D = max(0, (qn_p + qn_j) - 2 v_pj), w = ((double)a * (double)b) / (double)(a + b) for a = qcnt[p],
 * b = xcnt[j], cost_pj = w * D, every operation in double and rounded once:
 * nn_out[p] = the live column j != qself[p] of the least cost_pj, ties to the lowest j; cost_out[p] = that cost (double; the height of
 * the merge is sqrt(2 cost)); a query without a live foreign column gets -1 and +inf.  info_out int32 [4] as scd_knn's.  Two fp16 MFMA
 * passes with an error bound computed from the rows propose candidates, float64 decides; the result never depends on them; two calls
 * return the same bits.
 * prepared: the workspace still holds the fp16 copy, row statistics and norms of positions 0 .. prepared - 1 of this X (same m and d)
 * from earlier calls, kept up to date by scd_ward_merge; 0 prepares everything, m nothing.  Limits: 1 <= q < 2^29, 2 <= m < 2^29, d
 * rounded up to 32 <= 1024; scd_ward_nearest_ws_bytes returns 0 outside them.  The workspace holds the fp16 copies of X and Q and
 * scd_knn_slots() int32 slots per query: 0.68 GB at q = m = 126,976, d = 768. */
size_t scd_ward_nearest_ws_bytes(int64_t q, int64_t m, int d);
int scd_ward_nearest(scd_handle h, const float* Q, const int32_t* qcnt, const int32_t* qself, const float* X, const int32_t* xcnt, int64_t q,
                     int64_t m, int d, int64_t prepared, int32_t* nn_out, double* cost_out, int32_t* info_out, void* ws, size_t ws_bytes,
                     void* stream);
/* The merges of one round, in place: for each of the `pairs` pairs (lo[e], hi[e]), lo < hi, both live, no position in two pairs:
 * X_lo <- fl32(((double)a X_lo + (double)b X_hi) / (double)(a + b)) per coordinate with a = xcnt[lo], b = xcnt[hi] (the products are
 * exact below 2^29 rows), xcnt[lo] = a + b, xcnt[hi] = 0, and the prepared data of position lo in the workspace of scd_ward_nearest
 * (any q; the table's part depends on m and d alone) is made again.  A pair that breaks the conditions is left alone.  With the two
 * entries a C host drives a whole fit: search the stale clusters, merge the reciprocal pairs, repeat. */
int scd_ward_merge(scd_handle h, float* X, int32_t* xcnt, const int32_t* lo, const int32_t* hi, int64_t pairs, int64_t m, int d, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- the linear probe: multinomial logistic regression on frozen features (the linear evaluation of DINO / DINOv2; scikit-learn's
 *      LogisticRegression(C) written as a sum; the reference trains the same head in gcd/methods/cluster_and_classifier/
 *      train_supervised.py; docs/design/probe.md) ---- */
/* Bytes of workspace of scd_probe_loss_grad for X [n, d] and c classes: the packed W, the residuals r float32 [n, c up to 32], the row
 * losses float32 [n] and the float64 partial sums of the row ranges; 0.65 GB at n = 126,976, d = 768, c = 1000.  0 outside the limits
 * 1 <= n < 2^31, 1 <= d <= 1024, 2 <= c <= 1024.  scd_probe_predict needs scd_probe_ws_bytes(1, d, c) whatever its n. */
size_t scd_probe_ws_bytes(int64_t n, int d, int c);
/* Rows of X a block of the forward kernel owns (with all c classes). */
int scd_probe_row_tile(void);
/* The longest float32 accumulation chain over rows in the gradient (<= 1024): a chain's 32 x 32 tile is added into float64, so the
 * gradient's rounding error is gamma_T sum_i |r_ic x_id| with T this value, whatever n. */
int scd_probe_chain_rows(void);
/* The data term of the objective and its gradient at (W, b):
 *   loss = sum_i s_i [lse_c(z_ic) - z_{i,y_i}],  gW = r^T X,  gb = column sums of r,  z_ic = W_c . x_i + b_c,
 *   r_ic = s_i (softmax(z_i)_c - [c == y_i]),  s_i = sample_weight[i], or 1 when sample_weight is NULL.
 * X float32 [n, d], y int32 [n], W float32 [c, d], b float32 [c] or NULL (then b = 0); loss_out double [1], gW_out double [c, d], gb_out
 * double [c] or NULL, pred_out int32 [n] or NULL: argmax_c z_ic, ties to the lowest class.  info_out int32 [2] = {rows whose label is
 * outside [0, c): such a row contributes nothing, as if its weight were 0; rows with a non-finite logit: the outputs are then not
 * meaningful}.  The logits are float32 fma chains over k ascending from zero (the float32-input MFMA), b added last; the softmax uses
 * expf / logf and a correctly rounded division on z - max, the maximum over the real classes; the gradient accumulates float32 over
 * chains of scd_probe_chain_rows() rows and float64 across them.  No [n, c] logits reach memory, only r.  The L2 term of the objective
 * is the caller's.  Two calls return the same bits: no floating-point atomics, and every partition of the work depends on (n, d, c)
 * alone. */
int scd_probe_loss_grad(scd_handle h, const float* X, const int32_t* y, const float* sample_weight, int64_t n, int d, int c, const float* W,
                        const float* b, double* loss_out, double* gW_out, double* gb_out, int32_t* pred_out, int32_t* info_out, void* ws,
                        size_t ws_bytes, void* stream);
/* The forward pass alone: pred_out int32 [n] = argmax_c z_ic (ties to the lowest class), the same logits as scd_probe_loss_grad's, and
 * top_logit_out float32 [n, 2] or NULL: the largest and the second largest logit of the row (equal when two classes tie). */
int scd_probe_predict(scd_handle h, const float* X, int64_t n, int d, int c, const float* W, const float* b, int32_t* pred_out,
                      float* top_logit_out, void* ws, size_t ws_bytes, void* stream);

/* ---- Gaussian mixtures with diagonal covariances: scikit-learn 1.7's GaussianMixture(covariance_type='diag' | 'spherical'), with
 *      labelled rows clamped to their class (the semi-supervised mixture of GPC, "Learning semi-supervised Gaussian mixture models for
 *      generalized category discovery"; docs/design/gmm.md) ---- */
/* Bytes of workspace of scd_gmm_em_step for X [n, d] and k components: the packed B and C, the responsibilities r float32 [n, k up to
 * 32], the row log-likelihoods float64 [n] and the float64 partial sums of the row ranges; 0.66 GB at n = 126,976, d = 768, k = 1000.
 * 0 outside the limits 1 <= n < 2^31, 1 <= d <= 1024, 1 <= k <= 1024.  scd_gmm_predict needs scd_gmm_ws_bytes(1, d, k) whatever its n. */
size_t scd_gmm_ws_bytes(int64_t n, int d, int k);
/* Rows of X a block of the forward kernel owns (with all k components). */
int scd_gmm_row_tile(void);
/* The longest float32 accumulation chain over rows in the moments (<= 1024): a chain's 32 x 32 tile is added into float64, so a
 * moment's rounding error is gamma_T sum_i |r_ik x_id| with T this value, whatever n. */
int scd_gmm_chain_rows(void);
/* One E-step and the sufficient statistics of the M-step at the weighted log-densities
 *   z_ik = a_k + sum_d x_id B_kd + sum_d x_id^2 C_kd,   B = mu / v,  C = -1 / (2 v),
 *   a_k = log w_k - 0.5 sum_d mu_kd^2 / v_kd - 0.5 sum_d log v_kd - (d / 2) log 2 pi
 * (the caller forms them in float64 and rounds to float32; a constant may be taken out of a and added back to ll, the softmax does not
 * see it).  X float32 [n, d]; y int32 [n] or NULL; a float32 [k]; B, C float32 [k, d]; s_i = sample_weight[i], or 1 when it is NULL.
 *   an unlabelled row (y NULL, or y_i < 0):  r_ik = s_i softmax_k(z_i),  row log-likelihood s_i lse_k(z_ik)
 *   a labelled row (0 <= y_i < k):           r_ik = s_i [k == y_i],      row log-likelihood s_i z_{i,y_i}   (the clamped E-step)
 *   y_i >= k:                                the row is unlabelled, and info[0] counts it
 * ll_out double [1] = the sum of the row log-likelihoods, nk_out double [k] = sum_i r_ik, s1_out double [k, d] = r^T X, s2_out double
 * [k, d] = r^T (X o X); pred_out int32 [n] or NULL: argmax_k z_ik of every row whatever its label, ties to the lowest component.
 * info_out int32 [2] = {rows with y_i >= k; rows with a non-finite logit: the outputs are then not meaningful}.
 * a == B == C == NULL is the hard M-step (y is then required): no density pass runs, every row with a label in range contributes its
 * one-hot times s_i, every other row nothing, ll_out is 0 and pred_out is not written.
 * The logits are float32 fma chains from a zero accumulator (the float32-input MFMA): octets of d ascending, within an octet the eight
 * x B products, then the eight x^2 C products (x^2 one float32 multiply), a_k added last; the softmax uses expf / logf and a correctly
 * rounded division on z - max, the maximum over the real components; the moments accumulate float32 over chains of
 * scd_gmm_chain_rows() rows and float64 across them.  No [n, k] logits reach memory, only r.  Two calls return the same bits: no
 * floating-point atomics, and every partition of the work depends on (n, d, k) alone. */
int scd_gmm_em_step(scd_handle h, const float* X, const int32_t* y, const float* sample_weight, int64_t n, int d, int k, const float* a,
                    const float* B, const float* C, double* ll_out, double* nk_out, double* s1_out, double* s2_out, int32_t* pred_out,
                    int32_t* info_out, void* ws, size_t ws_bytes, void* stream);
/* The forward pass alone, the same logits as scd_gmm_em_step's: pred_out int32 [n] or NULL = argmax_k z_ik (ties to the lowest
 * component), row_ll_out float32 [n] or NULL = lse_k z_ik, resp_out float32 [n, k] or NULL = softmax_k(z_i), dense. */
int scd_gmm_predict(scd_handle h, const float* X, int64_t n, int d, int k, const float* a, const float* B, const float* C,
                    int32_t* pred_out, float* row_ll_out, float* resp_out, void* ws, size_t ws_bytes, void* stream);

/* ---- Gaussian mixtures with a full covariance matrix per component, on rows of at most 64 dimensions (what scd_pca_transform gives):
 *      scikit-learn 1.7's GaussianMixture(covariance_type='full'; 'tied' is the same call with one factor replicated k times), labelled
 *      rows clamped as in scd_gmm_em_step (docs/design/gmm_full.md) ---- */
/* Bytes of workspace of scd_gmm_full_em_step for X [n, d] and k components: the packed Ut and mu, the responsibilities r float32 [n, k
 * up to 32], the row log-likelihoods float64 [n] and the float64 partial sums of the row ranges (32 MB a range for S at k = 1000,
 * d = 64); 0.69 GB at n = 126,976, d = 64, k = 1000.  0 outside the limits 1 <= n < 2^31, 1 <= d <= 64, 1 <= k <= 1024.
 * scd_gmm_full_predict needs scd_gmm_full_ws_bytes(1, d, k) whatever its n. */
size_t scd_gmm_full_ws_bytes(int64_t n, int d, int k);
/* Rows of X a block of the forward kernel owns (with all k components). */
int scd_gmm_full_row_tile(void);
/* The longest float32 accumulation chain over rows in S (<= 1024): a chain's 32 x 32 tile is added into float64. */
int scd_gmm_full_chain_rows(void);
/* One E-step and the sufficient statistics of the M-step, taken about the current means, at the weighted log-densities
 *   c_ikl = fl32(x_il - mu_kl),   y_ikj = sum_l c_ikl U_k[l][j],   q_ik = sum_j y_ikj^2,   z_ik = a_k - 0.5 q_ik,
 *   a_k = log w_k + sum_j log U_k[j][j]      (the constant -(d / 2) log 2 pi is the caller's to add to ll)
 * with U_k scikit-learn's precisions_cholesky_ (upper triangular, U_k U_k^T = Sigma_k^-1).  The caller forms a, mu and U in float64 and
 * rounds them to float32.  X float32 [n, d]; y int32 [n] or NULL; a float32 [k]; mu float32 [k, d]; Ut float32 [k, d, d] with
 * Ut[k][j][l] = U_k[l][j], its entries with l > j exact zeros (the kernel skips those beyond a 32-column tile; a zero product adds an
 * exact zero, so the bits do not depend on that); s_i = sample_weight[i], or 1 when it is NULL.
 * Rows, labels, y_i >= k (info[0]), non-finite logits (info[1]), the softmax (maximum over the real components, expf, a correctly
 * rounded division), ll_out, pred_out (ties to the lowest component) and the determinism are scd_gmm_em_step's, word for word.
 * nk_out double [k] = sum_i r_ik, s1c_out double [k, d] = sum_i r_ik c_ik, S_out double [k, d, d] = sum_i r_ik c_ik c_ik^T with
 * S[k][j][l] and S[k][l][j] written from the same sum (bit-symmetric).
 * a == Ut == NULL is the hard M-step (y and mu, the centres the moments are taken about, are still required): every row with a label
 * in range contributes its one-hot times s_i, ll_out is 0 and pred_out is not written.
 * The order: y is a float32 fma chain with l ascending from a zero accumulator (the float32-input MFMA), c one IEEE subtraction in a
 * register; q a fmaf chain of the squares in an order fixed by d alone (docs/design/gmm_full.md), z = fmaf(-0.5, q, a_k); S
 * accumulates r_ik c_ij (one float32 product) times c_il in float32 over chains of scd_gmm_full_chain_rows() rows and float64 across
 * them, s1c and nk in float64 throughout.  No [n, k] logits reach memory, only r. */
int scd_gmm_full_em_step(scd_handle h, const float* X, const int32_t* y, const float* sample_weight, int64_t n, int d, int k,
                         const float* a, const float* mu, const float* Ut, double* ll_out, double* nk_out, double* s1c_out, double* S_out,
                         int32_t* pred_out, int32_t* info_out, void* ws, size_t ws_bytes, void* stream);
/* The forward pass alone, the same logits: pred_out int32 [n] or NULL, row_ll_out float32 [n] or NULL = lse_k z_ik, resp_out float32
 * [n, k] or NULL = softmax_k(z_i), dense. */
int scd_gmm_full_predict(scd_handle h, const float* X, int64_t n, int d, int k, const float* a, const float* mu, const float* Ut,
                         int32_t* pred_out, float* row_ll_out, float* resp_out, void* ws, size_t ws_bytes, void* stream);

/* ---- principal component analysis: scikit-learn 1.7's PCA(svd_solver='covariance_eigh') without a centred or float64 copy of the rows
 *      (docs/design/pca.md).  Every call sees the rows as c_ij = fl32(x_ij - shift_j), one IEEE float32 subtraction in a register;
 *      shift float32 [d], or NULL for 0.  The eigensolver of the d x d matrix is the caller's. ---- */
/* Bytes of workspace for X [n, d] and m components: the float64 partial sums of the row ranges, a flag per row and the packed W; 0.15 GB
 * at n = 126,976, d = 768, m = 1024.  0 outside the limits 1 <= n < 2^31, 1 <= d <= 1024, 1 <= m <= 1024.  scd_pca_colsum and
 * scd_pca_gram need scd_pca_ws_bytes(n, d, 1), scd_pca_transform needs scd_pca_ws_bytes(1, d, m) whatever its n. */
size_t scd_pca_ws_bytes(int64_t n, int d, int m);
/* Rows of X a block of the projection kernel owns (with all m columns). */
int scd_pca_row_tile(void);
/* The longest float32 accumulation chain over rows in the Gram matrix: a chain's 32 x 32 tile is added into float64, so an element's
 * rounding error is gamma_T sum_i |c_ij c_il| with T this value, whatever n. */
int scd_pca_chain_rows(void);
/* csum_out double [d] = sum_i c_ij in float64 (the subtraction alone is float32): row ranges of a fixed size, added in ascending order.
 * With shift NULL it is n times the mean; with the rounded mean as shift it is the exact residual, which is not zero. */
int scd_pca_colsum(scd_handle h, const float* X, const float* shift, int64_t n, int d, double* csum_out, void* ws, size_t ws_bytes,
                   void* stream);
/* G_out double [d, d] = c^T c.  128 x 128 tiles of the upper triangle times R row ranges; the float32-input MFMA over chains of
 * scd_pca_chain_rows() rows, float64 across chains and ranges (ascending); G[j][l] and G[l][j] are written from the same sum, so G is
 * bit-symmetric.  info_out int32 [2] = {rows that hold a non-finite c: G is then not meaningful; 0}.  Two calls return the same bits:
 * no floating-point atomics, and every partition of the work depends on (n, d) alone. */
int scd_pca_gram(scd_handle h, const float* X, const float* shift, int64_t n, int d, double* G_out, int32_t* info_out, void* ws,
                 size_t ws_bytes, void* stream);
/* Y_out float32 [n, m]: y_ik = sum_j c_ij W_kj, W float32 [m, d] (the components, any whitening scale folded in by the caller), a float32
 * fma chain from a zero accumulator with j ascending.  unit != 0: each row is divided by its float32 L2 norm over the m columns (sqrtf
 * and the division correctly rounded); a row of norm 0 is written as zeros.  info_out int32 [2] = {rows with a non-finite y; rows of
 * norm 0 (unit only)}. */
int scd_pca_transform(scd_handle h, const float* X, const float* shift, const float* W, int64_t n, int d, int m, int unit, float* Y_out,
                      int32_t* info_out, void* ws, size_t ws_bytes, void* stream);

/* ---- exact t-SNE: scikit-learn 1.7's TSNE(n_components=2) as the reference's save_tsne / save_tsne_wcolor call it
 *      (local_utils/util.py:178-216), with the exact all-pairs gradient instead of Barnes-Hut's (docs/design/tsne.md) ---- */
/* The conditional affinities of a k-NN graph: dist2 double [n, k] (squared distances, finite and >= 0), row i ->
 * p_out[i, j] = exp(-b_i (d_ij - d_i,min)) / sum, b_i (beta_out double [n]) the root of H_i(b) = log(perplexity), natural logarithms,
 * all in float64.  The search is sklearn/manifold/_utils.pyx's: from b = 1, doubling or halving until the root is bracketed, then
 * bisection - but with a fixed count of 200 steps and no exit on a tolerance, so the row is a function of the root alone.
 * info_out int32 [2] = {rows whose entropy cannot reach the target (for example all k distances equal): they end at the last bracket
 * value and still sum to 1; rows with a negative or non-finite distance: they get 1 / k and beta NaN}.
 * Limits: 1 <= n < 2^31, 2 <= k <= 64, 1 < perplexity < k (SCD_EINVAL outside).  Two calls return the same bits. */
int scd_tsne_calibrate(scd_handle h, const double* dist2, int64_t n, int k, double perplexity, double* p_out, double* beta_out,
                       int32_t* info_out, void* stream);
/* The gradient of KL(P || Q) at Y float [n, 2] (8-byte aligned) for the symmetric joint affinities P in CSR form (indptr int64 [n + 1],
 * indices int32 [nnz], values double [nnz]):  q_ij = 1 / (1 + |y_i - y_j|^2),  Z = sum over i != j of q_ij,
 *   grad_i = 4 [ exaggeration * sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_{j != i} q_ij^2 (y_i - y_j) ]          (grad_out double [n, 2])
 *   KL = sum over P_ij > 0 of P_ij log(P_ij Z / q_ij), always at exaggeration 1                                   (kl_out double [1], or NULL)
 * and z_out double [1] = Z.  The all-pairs sums take each pair in fp32 (v_rcp_f32 for q) and fold runs of 64 columns into float64:
 * per row |error| <= 80 * 2^-24 * the sum of the terms' magnitudes (docs/design/tsne.md); the pair i = i and the padding are excluded
 * by index, coincident points count 1 in Z.  flags = SCD_TSNE_EXACT_PAIRS takes the pairs in float64 with a division instead (the
 * same kernel at the float64 rate): the KL a fit reports is computed so.  The CSR sums and KL are float64 throughout.  No floating-point atomics: column ranges
 * are combined in a fixed order, and two calls return the same bits.
 * info_out int32 [2] = {rows with an indptr pair outside 0 <= lo <= hi <= nnz or a column outside [0, n): such entries are skipped and
 * never dereferenced; rows of Y that are not finite with |y| < 2^60}.  A call with info_out != {0, 0} has no meaning beyond that.
 * Limits: 2 <= n < 2^31, 0 <= nnz < 2^40; scd_tsne_gradient_ws_bytes returns 0 outside them.  The workspace holds the per-range
 * partial sums: 24 n bytes per column range (at most 32 ranges) + 56 n.  scd_tsne_row_tile / scd_tsne_col_chunk: the rows of a
 * block and the columns staged at a time (the tests place their sizes around them). */
size_t scd_tsne_gradient_ws_bytes(int64_t n, int64_t nnz);
int scd_tsne_row_tile(void);
int scd_tsne_col_chunk(void);
#define SCD_TSNE_EXACT_PAIRS 1
int scd_tsne_gradient(scd_handle h, const float* Y, const int64_t* indptr, const int32_t* indices, const double* values, int64_t n,
                      int64_t nnz, double exaggeration, int flags, double* grad_out, double* z_out, double* kl_out, int32_t* info_out,
                      void* ws, size_t ws_bytes, void* stream);
/* One step of _gradient_descent (sklearn/manifold/_t_sne.py) on the 2 n elements of the float64 state, in place:
 *   gains += 0.2 where vel * grad < 0, else gains *= 0.8; gains = max(gains, min_gain); vel = momentum * vel - learning_rate * (gains * grad);
 *   Y64 += vel; Y32_out = Y64 rounded to nearest.  gg_out double [n, 2] (or NULL) = gains * grad, the vector whose norm the optimiser's
 * min_grad_norm test reads.  Every operation is the IEEE float64 one (no contraction): the step equals numpy's bit for bit. */
int scd_tsne_update(scd_handle h, const double* grad, double* Y64, double* vel, double* gains, float* Y32_out, int64_t n, double momentum,
                    double learning_rate, double min_gain, double* gg_out, void* stream);

/* ---- host solvers (CPU, synchronous) ---- */
/* linear_assignment (gcd/project_utils/cluster_utils.py:234-493), same tie-breaking; pairs_out [min(n,m),2] sorted */
int scd_munkres(const int64_t* cost, int n, int m, int64_t* pairs_out, int* n_pairs_out);
/* assign_name's solve (local_utils/clip_lang_util.py:167-178): linear_assignment(w.max() - w) for the d x d vote matrix w
 * given by its nnz non-zero entries (rows/cols int32, vals int64; duplicates add up as `w[i, col] += v` does) - the same
 * decisions as scd_munkres on the dense matrix, in O(d) per covered row instead of O(d^2): d reaches 10,000-20,000 at
 * K = 1000 clusters (BASELINE configs[3]).  pairs_out [d,2] sorted by row. */
int scd_munkres_sparse(int d, int64_t nnz, const int32_t* rows, const int32_t* cols, const int64_t* vals,
                       int64_t* pairs_out, int* n_pairs_out);
/* solve_min_cost_flow_graph (sskm_constrained.py:331-356) on the transportation form: cost int32 [n,k] */
int scd_transport_solve(const int32_t* cost, int64_t n, int k, int size_min, int size_max, int32_t* labels_out,
                        int64_t* total_cost_out);
/* `batch` problems of one shape - the E-steps of a fit's restarts (sskm_constrained.py:165-176, independent once seeded) - on up to
 * `threads` host threads: cost int32 [batch,n,k], labels_out int32 [batch,n], totals_out int64 [batch] (or NULL).  Every problem's
 * result is scd_transport_solve's for it, whatever the thread count; the status is that of the first problem that failed. */
int scd_transport_solve_batch(const int32_t* cost, int64_t n, int k, int batch, int size_min, int size_max, int32_t* labels_out,
                              int64_t* totals_out, int threads);

/* ---- multi-GPU exchanges over RCCL (one process per GPU, one communicator per handle).  The reference is a
 * single process; these are the two collectives the sharded hot path needs.  librccl is dlopen'ed by the first call.
 *   rank 0: scd_comm_unique_id(id) -> ship the scd_comm_unique_id_bytes() bytes to every rank (file, socket, MPI ...)
 *   all   : scd_comm_init(h, rank, world, id) ... scd_comm_destroy(h)
 * scd_allreduce_centroids: in-place float64 sum of the packed M-step partials [sums k*d | counts k | inertia 2] (what
 *   scd_kmeans_mstep produces, counts converted to float64) - ONE collective per Lloyd iteration;
 * scd_allgather_text: w_full [world * shard_elems] fp16 <- every rank's w_shard (name-major classifier rows, equal shards). */
size_t scd_comm_unique_id_bytes(void);
int scd_comm_unique_id(void* id_out);
int scd_comm_init(scd_handle h, int rank, int world, const void* unique_id);
int scd_comm_destroy(scd_handle h);
int scd_allreduce_centroids(scd_handle h, double* packed, int64_t count, void* stream);
int scd_allgather_text(scd_handle h, const void* w_shard, int64_t shard_elems, void* w_full, void* stream);

/* ---- spectral clustering on the exact k-NN graph: scikit-learn 1.7's SpectralClustering(affinity='nearest_neighbors')
 *      (sklearn/cluster/_spectral.py:_fit; no counterpart in the reference; docs/design/spectral.md) ---- */
/* The symmetric normalised affinity of k-NN lists, in CSR form.  idx int32 [n][k] (scd_knn's idx_out: a row does not list itself; k =
 * scikit-learn's n_neighbors - 1).  Replaces sklearn.neighbors.kneighbors_graph(include_self=True) + `0.5 * (C + C.T)`
 * (sklearn/cluster/_spectral.py) and scipy.sparse.csgraph.laplacian(normed=True)'s `w = sqrt(degree); m /= w; m /= w[:, None]`
 * (scipy/sparse/csgraph/_laplacian.py) with the diagonal removed first (sklearn/manifold/_spectral_embedding.py):
 *   A[i][j] = 1 when i and j list each other, 0.5 when one lists the other;  d_i = sum_j A[i][j] (a multiple of 0.5, exact);
 *   S[i][j] = A[i][j] / (sqrt(d_i) * sqrt(d_j)) in float64, these operations in this order: S is symmetric bit for bit.
 * A negative entry and idx[i][j] == i are ignored, a neighbour listed twice in a row counts once, an index >= n is SCD_EINVAL.
 * rowptr int64 [n + 1], col int32 [cap] and val double [cap] with cap >= 2 n k; columns ascend inside a row, so the result is one fixed
 * array; *nnz_out (host) = rowptr[n].  inv_sqrt_deg double [n] = 1 / sqrt(d_i), and 1 for a row without an edge (scipy's isolated
 * nodes).  A row's length is its list plus its one-way in-degree: nothing is sized by 2 k.  The call waits for the stream (the index
 * check and nnz come back to the host).  Limits: 2 <= n < 2^31, 1 <= k <= 64; scd_knn_affinity_ws_bytes returns 0 outside them. */
size_t scd_knn_affinity_ws_bytes(int64_t n, int k);
int scd_knn_affinity(scd_handle h, const int32_t* idx, int64_t n, int k, int64_t* rowptr, int32_t* col, double* val, double* inv_sqrt_deg,
                     int64_t cap, int64_t* nnz_out, void* ws, size_t ws_bytes, void* stream);
/* Y = alpha (S X) + beta X + gamma Z for S in CSR form (n rows and columns) and blocks X [n][ldx], Z [n][ldz] (or NULL: no third term),
 * Y [n][ldy] of m columns, float64: the sparse product of scipy.sparse's `S @ X` under sklearn's eigensolver, and one step of the
 * Chebyshev three-term recurrence in one launch.  The summation order is part of the contract: a row of at most 512 entries is summed
 * left to right in CSR order from 0, a multiply and an add per term, no fused multiply-add; a longer row is cut into chunks of 512
 * entries, each summed that way, and the chunk sums are added in chunk order from 0; then (alpha * sum + beta * x) + gamma * z.  No
 * floating-point atomics: two calls return the same bits, and numpy can restate them.  A column outside [0, n) reads nothing and
 * counts as a row of zeros; a row pointer pair outside 0 <= lo <= hi <= rowptr[n] makes an empty row.
 * Limits: m % 8 == 0, leading dimensions multiples of 8 and >= m, blocks 16-byte aligned, Y's span overlaps neither X's nor Z's. */
int scd_spmm_f64(scd_handle h, const int64_t* rowptr, const int32_t* col, const double* val, int64_t n, const double* X, int64_t ldx, int m,
                 double alpha, double beta, double gamma, const double* Z, int64_t ldz, double* Y, int64_t ldy, void* stream);

/* ---- encoders: CLIP ViT-B/16 visual / text (third-party `clip`, call sites main_unsup.py:127,
 *      clip_lang_util.py:101-102), DINO ViT-B/16 (gcd/models/vision_transformer.py:135-219) and DINOv2 ViT-B/14 / ViT-L/14 with or
 *      without register tokens (kind 2 with patch 14; LayerScale, the position table at 16 x 16 and the input normalisation are
 *      folded into the weights by the loader, docs/design/dinov2.md) ---- */
typedef struct scd_encoder_desc {
    int kind;          /* 0 CLIP visual, 1 CLIP text, 2 DINO/GCD/DINOv2 ViT */
    int width, layers, heads, mlp_dim;
    int tokens;        /* visual: (image/patch)^2 + 1 + registers = 197 (ViT-B/16), 257 (patch 14) or 257 + registers <= 288; text: 77 */
    int patch, image;  /* 16 or 14, 224 (visual) */
    int vocab;         /* 49408 (text) */
    int out_dim;       /* 512 (CLIP ViT-B/16), 768 (CLIP ViT-L/14) or 0 = no projection (DINO) */
    int act;           /* 0 QuickGELU, 1 erf GELU */
    float ln_eps;
    int registers;     /* kind 2 only: register tokens between the class token and the patches (DINOv2 `_reg`: 4), rows that get no
                        * position embedding; 0 for every other tower.  registers > 0 adds ONE weight pointer behind the last layer's:
                        * fp32 [registers][width] */
} scd_encoder_desc;
/* weights: array of device pointers in the order documented in DESIGN.md (fp16 matrices, fp32 vectors); n_weights is checked exactly:
 * 9 + 12 * layers, + 1 when registers > 0. */
int scd_encoder_create(scd_handle h, const scd_encoder_desc* desc, const void* const* weights, int n_weights,
                       scd_encoder** out);
int scd_encoder_destroy(scd_encoder* e);
size_t scd_encoder_ws_bytes(const scd_encoder* e, int batch);
/* Measurement aid: while enabled, every fc1 GEMM launch of the encoder (its dominant kernel) is bracketed by HIP events on
 * the launch stream.  Each call returns and clears what was collected so far: total milliseconds, launches, algorithmic
 * FLOPs (2*M*N*K per launch); it synchronises on the recorded events. */
int scd_encoder_timing(scd_encoder* e, int enable, double* ms_out, int* launches_out, double* flop_out);
/* pixels [B,3,H,W] (dtype f32/f16) -> out fp16 [B,out] (L2-normalised when normalize != 0) */
int scd_vit_encode_image(scd_handle h, const scd_encoder* e, const void* pixels, int dtype, int batch, void* out,
                         int normalize, void* ws, size_t ws_bytes, void* stream);
/* tokens int32 [B,77] -> out fp16 [B,out] */
int scd_clip_encode_text(scd_handle h, const scd_encoder* e, const int32_t* tokens, int batch, void* out,
                         int normalize, void* ws, size_t ws_bytes, void* stream);
/* The same with only the first ctx_len positions of every prompt computed (tokens stays [B,77]).  Precondition: ctx_len >
 * the EOT position (argmax over the 77 ids) of every row - then the outputs are bit-identical to scd_clip_encode_text (the tower is
 * causal and only the EOT position is read, reference clip model.py encode_text), at ctx_len/77 of the work. */
int scd_clip_encode_text_len(scd_handle h, const scd_encoder* e, const int32_t* tokens, int batch, int ctx_len, void* out,
                             int normalize, void* ws, size_t ws_bytes, void* stream);
/* building block exposed for tests: the encoder blocks' attention, softmax(Q K^T / 8) V per (sequence, head), head_dim 64, width =
 * heads * 64 <= 1024.  qkv fp16 [batch*T][3*width] (Q | K | V, as the QKV GEMM writes them) -> out fp16 [batch*T][width]; causal: query
 * t sees keys 0..t.  Served: T <= 96, T = 197, non-causal 192 < T <= 224 and non-causal 256 < T <= 288 (SCD_EINVAL otherwise); the
 * kernel is the one the towers run at that T. */
int scd_attention_f16(scd_handle h, const void* qkv, int batch, int T, int width, int heads, int causal, void* out, void* stream);
/* building block exposed for tests: the visual towers' token assembly, through the launcher the towers call.  patch fp16
 * [batch * np][width] (np = T - 1 - nreg, the patch GEMM's rows), patch_bias fp32 [width] or NULL, cls fp32 [width], pos fp32 [1 + np][width],
 * registers fp32 [nreg][width] (NULL when nreg == 0) -> out fp16 [rows_pad][width], rows_pad = batch * T rounded up to 256:
 *   out[b*T + 0] = cls + pos[0];  out[b*T + t] = registers[t - 1] for 1 <= t <= nreg (no position row);
 *   out[b*T + t] = (patch[b*np + t - 1 - nreg] + patch_bias) + pos[t - nreg] for t > nreg;  rows >= batch * T are zeros.
 * stats int64 [rows_pad][2] or NULL: the rows' LayerNorm statistics in scd_gemm_ln's fixed point.  width % 256 == 0, width <= 1024. */
int scd_vit_assemble_f16(scd_handle h, const void* patch, const float* patch_bias, const float* cls, const float* pos,
                         const float* registers, int nreg, int batch, int T, int width, void* out, int64_t* stats, void* stream);
/* building block exposed for tests: the last block's one-query attention (the CLS / EOT row). kv fp16 [batch*T][2*width] (K | V),
 * q and out fp16 [batch][width], T <= 256; qrow int32 [batch] on the device = b*T + the query's position (causal: the last key it
 * sees; may be NULL when causal == 0, then every key is seen). */
int scd_attention_single_query_f16(scd_handle h, const void* kv, const void* q, const int* qrow, int batch, int T, int width,
                                   int heads, int causal, void* out, void* stream);
/* building block exposed for tests: C[m,n] = A[m,k] @ W[n,k]^T (+bias)(act)(+residual), fp16 in/out, fp32 accumulate */
int scd_gemm_f16(scd_handle h, const void* A, const void* W, const float* bias, const void* residual, void* C,
                 int64_t m, int n, int k, int act, void* stream);
/* building blocks exposed for tests: the rest of the GEMM family the encoder blocks run, each through the launcher the towers call.
 * scd_gemm_ln_apply_f16: C = act(LayerNorm(A) W^T + b) in the folded form (QKV / fc1): Wf, biasf, colsum as scd_fold_ln_f16 makes them,
 *   stats_in int64 [m][2] = {sum * 2^24, sum of squares * 2^20} of A's rows; rs float [m][2] is scratch ({rstd, -mean * rstd} on return),
 *   zero_out (or NULL) a second [m][2] statistics buffer that is cleared.  m % 256 = n % 256 = k % 64 = 0.
 * scd_gemm_res_stats_f16: C = A W^T + bias + residual (proj / fc2; C may be the residual buffer) and stats_out[m] += the same fixed-point
 *   sums of the stored rows of C (the caller clears stats_out).  bias and residual are required, act must be 0.
 * scd_fold_ln_f16: Wf[n][k] = fp16(W[n][k] gamma[k]), colsum[n] = sum_k Wf[n][k], biasf[n] = bias[n] + sum_k beta[k] W[n][k].
 * scd_gemm_img_f16: the patch-16 embedding GEMM fed from the fp16 image batch [batch][3][image][image]: row b * (image/16)^2 + p of C
 *   [m][n] = patch (b, p) (k = c * 256 + i * 16 + j) times W[n][768]^T; m % 256 = 0, m >= batch * (image/16)^2 (rows beyond: scratch).
 * scd_layernorm_f16: out[r] = fp16(LayerNorm(x[row_index ? row_index[r] : r]) gamma + beta), width a multiple of 256, at most 1024. */
int scd_gemm_ln_apply_f16(scd_handle h, const void* A, const void* Wf, const float* biasf, const float* colsum, const int64_t* stats_in,
                          float* rs, int64_t* zero_out, void* C, int64_t m, int n, int k, float eps, int act, void* stream);
int scd_gemm_res_stats_f16(scd_handle h, const void* A, const void* W, const float* bias, const void* residual, void* C,
                           int64_t* stats_out, int64_t m, int n, int k, int act, void* stream);
int scd_fold_ln_f16(scd_handle h, const void* W, const float* gamma, const float* beta, const float* bias, int n, int k, void* Wf,
                    float* colsum, float* biasf, void* stream);
int scd_gemm_img_f16(scd_handle h, const void* pixels, const void* W, void* C, int64_t m, int n, int batch, int image, void* stream);
int scd_layernorm_f16(scd_handle h, const void* x, const int* row_index, int64_t rows, int width, float eps, const float* gamma,
                      const float* beta, void* out, void* stream);

/* ---- image preprocessing: CLIP's `preprocess` (main_unsup.py:237,271, applied by the DataLoader at :271-289) on decoded images -
 *      torchvision Resize(size, BICUBIC) on a PIL RGB image (Pillow Resample.c, uint8, separable, int32 taps with 22 fraction bits),
 *      CenterCrop(crop), ToTensor + Normalize through a lookup table - bit for bit (docs/design/ingest.md).
 * Plans (per image size, cached by the library; host only):
 *   scd_image_geometry: out6 = {resized w, resized h, crop left, crop top, first source row read, source rows read};
 *   scd_image_plan_axis: Pillow's taps of outputs off .. off + n - 1 of an in_size -> out_size bicubic resize: first[n] input index,
 *     ntaps[n], taps = the int32 weights of every output in order; taps == NULL only reports the total (n_taps_out);
 *   scd_image_batch_plan: descs[batch] and the packed plan (int32 [plan_len]) of a batch of images of sizes wh = {w0, h0, w1, h1, ...}
 *     whose packed uint8 RGB HWC pixels lie back to back (pixel_bytes in all); ws_bytes: workspace of scd_image_preprocess.  With
 *     plan == NULL (descs may be NULL too) only the three sizes are reported.
 * scd_image_preprocess: descs / plan (device copies of scd_image_batch_plan's), lut fp16 [3][256] = ((v / 255 - mean) / std).half()
 *   per channel, out fp16 [batch, 3, crop, crop] (NCHW), crop <= 256.  Descriptors and taps are checked against pixel_bytes, plan_len
 *   and ws_bytes on the device by both passes: nothing is read outside them, and an image whose descriptor would (or a column whose
 *   taps would) gets NaN pixels there.  size and crop of the planners: 1 <= crop <= size <= 65536; image edges 1 .. 65536. */
typedef struct scd_image_desc {
    int64_t src_off;   /* byte offset of the image's pixels in `pixels` */
    int64_t tmp_off;   /* byte offset of its horizontal-pass band in the workspace */
    int32_t w, h;      /* source size */
    int32_t plan_x;    /* int32 offset of the horizontal plan block in `plan` */
    int32_t plan_y;    /* ... of the vertical one */
    int32_t row0, rows;/* source rows the horizontal pass covers */
} scd_image_desc;
int scd_image_geometry(int w, int h, int size, int crop, int32_t* out6);
int scd_image_plan_axis(int in_size, int out_size, int off, int n, int32_t* first, int32_t* ntaps, int32_t* taps, int64_t taps_cap,
                        int64_t* n_taps_out);
int scd_image_batch_plan(const int32_t* wh, int batch, int size, int crop, scd_image_desc* descs, int32_t* plan, int64_t plan_cap,
                         int64_t* plan_len, int64_t* pixel_bytes, int64_t* ws_bytes);
int scd_image_preprocess(scd_handle h, const uint8_t* pixels, int64_t pixel_bytes, const scd_image_desc* descs, const int32_t* plan,
                         int64_t plan_len, int batch, int crop, const void* lut, void* out, void* ws, size_t ws_bytes, void* stream);

/* ---- baseline JPEG decoding, bit-equal to Pillow's Image.open(f).convert('RGB') (torchvision's pil_loader, main_unsup.py:271-289), so that
 *      only the compressed bytes cross to the device (docs/design/ingest.md, "Device JPEG decode").
 * Scope: one SOF0 / SOF1 frame of 8-bit samples, 1 component or 3 (YCbCr by libjpeg's rule; chroma 1x1, luma 1x1, 2x1 or 2x2), one scan
 *   with all components and every table it names present, downsampled chroma wider than 2 samples.  scd_jpeg_parse reports anything
 *   else as info->reason != 0 (SCD_JPEG_*); such a file is the caller's to decode with Pillow.
 * scd_jpeg_parse (host): info of one file; rst_offsets (may be NULL with rst_cap 0) receives the file offsets of the first rst_cap RSTn
 *   markers of the scan, info->n_restarts counts all of them.  Returns SCD_OK whatever the reason.
 * scd_jpeg_batch_plan (host): descs[n] and the batch's distinct derived Huffman / quantisation tables for files whose infos have reason 0.
 *   The caller lays the files out back to back at descs[i].data_off (16-byte aligned, data_bytes in all); out_offs[i] is the byte offset of
 *   image i's w x h x 3 uint8 RGB (HWC) in the pixel section (scd_image_desc.src_off).  With descs == NULL and tables == NULL only the
 *   three sizes are reported (ws_bytes: workspace of scd_jpeg_decode).
 * scd_jpeg_decode (device): data / descs / tables are device copies; writes the RGB of every image whose status comes out 0 and
 *   status[n] (device int32): SCD_JPEG_E* for a stream the decoder cannot follow, for the range guard (a dequantised coefficient
 *   above 4096 or a column-pass output above 8192 in magnitude: beyond them libjpeg-turbo's 16-bit lanes could differ; a row-pass
 *   output outside [-512, 511]: beyond it libjpeg-turbo's C code wraps where its SIMD code saturates) and for a
 *   descriptor that reaches outside data_bytes / tables_bytes / ws_bytes / pixel_bytes.  Such an image's pixels are not written.
 *   data, tables and ws 16-byte aligned.  The kernels end on any input.
 * scd_jpeg_decode_host (host): the same functions on the CPU for one file; SCD_EINVAL when the parser rejects it, else *status_out as
 *   above and, for status 0, rgb[h][w][3]. */
enum { SCD_JPEG_OK = 0, SCD_JPEG_NOT_JPEG = 1, SCD_JPEG_TRUNCATED = 2, SCD_JPEG_BAD_MARKER = 3, SCD_JPEG_PROGRESSIVE = 4, SCD_JPEG_ARITHMETIC = 5,
       SCD_JPEG_SOF = 6, SCD_JPEG_PRECISION = 7, SCD_JPEG_COMPONENTS = 8, SCD_JPEG_SAMPLING = 9, SCD_JPEG_COLOURSPACE = 10,
       SCD_JPEG_MULTISCAN = 11, SCD_JPEG_MISSING_TABLE = 12, SCD_JPEG_BAD_TABLE = 13, SCD_JPEG_CHROMA_WIDTH = 14, SCD_JPEG_DNL = 15 };
enum { SCD_JPEG_EHUFF = 1, SCD_JPEG_EINDEX = 2, SCD_JPEG_EEOF = 3, SCD_JPEG_EMARKER = 4, SCD_JPEG_ERANGE = 5, SCD_JPEG_EDESC = 6 };
typedef struct scd_jpeg_info {
    int32_t reason;            /* 0: device-decodable; else SCD_JPEG_* (the fields below are then as far as the parser got) */
    int32_t w, h, ncomp;
    int32_t hs, vs;            /* luma sampling factors (1, 1 for one component) */
    int32_t restart_interval;  /* MCUs between RSTn markers, 0: none */
    int32_t file_len;
    int32_t scan_off, scan_end;/* the scan's bytes: [scan_off, scan_end), scan_end = the marker that ends it or file_len */
    int32_t has_eoi;           /* that marker is EOI */
    int32_t n_restarts;        /* RSTn markers inside the scan */
    int32_t qt_off[3], qt_prec[3]; /* per component: file offset of its quantisation table's 64 entries, 0 = 8-bit / 1 = 16-bit entries */
    int32_t dc_off[3], ac_off[3];  /* ... of its DC / AC Huffman table (16 counts, then the symbols) */
} scd_jpeg_info;
typedef struct scd_jpeg_desc {
    int64_t data_off;          /* byte offset of the file in `data` */
    int64_t out_off;           /* byte offset of its RGB in `pixels` */
    int64_t plane_off;         /* byte offset of its component planes in the workspace */
    int32_t data_len, scan_off, scan_end, has_eoi;
    int32_t w, h, ncomp, hs, vs, restart_interval;
    int32_t qt[3], dc[3], ac[3];   /* byte offsets of the component's tables in `tables` */
    int32_t pad_;
} scd_jpeg_desc;
int scd_jpeg_parse(const uint8_t* data, int64_t len, scd_jpeg_info* info, int32_t* rst_offsets, int64_t rst_cap);
int scd_jpeg_batch_plan(const uint8_t* const* files, const scd_jpeg_info* infos, const int64_t* out_offs, int n, scd_jpeg_desc* descs,
                        uint8_t* tables, int64_t tables_cap, int64_t* tables_bytes, int64_t* data_bytes, int64_t* ws_bytes);
int scd_jpeg_decode(scd_handle h, const uint8_t* data, int64_t data_bytes, const scd_jpeg_desc* descs, const uint8_t* tables,
                    int64_t tables_bytes, int n, uint8_t* pixels, int64_t pixel_bytes, int32_t* status, void* ws, size_t ws_bytes,
                    void* stream);
int scd_jpeg_decode_host(const uint8_t* data, int64_t len, uint8_t* rgb, int64_t rgb_cap, int32_t* status_out);

#ifdef __cplusplus
}
#endif
#endif /* SCD_HIP_H */
