/*
 * kmeans_amd.h - C-ABI of the MI355X-native Lloyd-iteration hot path.
 *
 * Drop-in boundary for the reference's per-iteration worker closures and the
 * Spark collectives around them (ersanjay16/Assignment--2-Group7-distributed-K-means,
 * kmeans_spark.py).  The reference has no FFI of its own: its interface for
 * this path is the PySpark RDD calls inside class KMeans, and each entry point
 * below names the reference call it replaces.  The Python host layer
 * (assignment--2-group7-distributed-k-means_amd/kmeans.py) binds these with
 * ctypes and re-exposes the reference's KMeans(...)/fit(rdd, sc)/predict(rdd, sc)
 * surface.
 *
 * Conventions
 *   - every function returns int: 0 = OK (KM_OK), KM_EMPTY (>0) where noted,
 *     < 0 = error; km_last_error() returns a thread-local message.
 *   - plain C types only: host pointers are caller-owned and may be released
 *     when the call returns; device pointers are marked "device".
 *   - all matrices are row-major; centroids are float64 [k][d]; data rows are
 *     float32 [n][d] (stored padded to a multiple of 16 features in HBM).
 *   - one context = one GPU = one rank; a context is not thread-safe.
 *   - work is enqueued on the context stream (km_set_stream, default: own
 *     non-blocking stream); calls that return host data synchronise it.
 */
#ifndef KMEANS_AMD_H
#define KMEANS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KM_ABI_VERSION 6

#define KM_OK 0
#define KM_EMPTY 1          /* informational: the update found empty clusters */
#define KM_ERR_ARG (-1)
#define KM_ERR_HIP (-2)
#define KM_ERR_STATE (-3)
#define KM_ERR_UNSUPPORTED (-4)

typedef struct km_ctx km_ctx;

/* Per-iteration result of km_update (quantities of kmeans_spark.py:176-313). */
typedef struct km_status {
  double sse;        /* SSE of this assignment w.r.t. the pre-update centroids
                        (replaces _compute_sse, kmeans_spark.py:208-237)        */
  double max_shift;  /* max_c ||new_c - old_c||, empties counted as 0
                        (kmeans_spark.py:293-294)                                */
  int32_t n_empty;   /* clusters absent from the reduce (kmeans_spark.py:186-188) */
  int32_t nonfinite; /* NaN/Inf in a new centroid (kmeans_spark.py:289)         */
  int32_t q_rerank;  /* points whose top-2 were re-ranked in float64             */
  int32_t q_full;    /* points that needed a full float64 scan                   */
  int32_t ran;       /* 1: the iteration ran (0: a no-op of a stopped batch)     */
  int32_t stop_reason; /* KM_STOP_* this iteration raised (batches), else 0     */
  int32_t repaired;  /* its empty clusters were replaced on the device
                        (max_shift includes them, kmeans_spark.py:191-204)      */
  int32_t reserved;
} km_status;

/* Why a batch stopped (km_status.stop_reason). */
#define KM_STOP_CONVERGED 1 /* max_shift < tolerance (kmeans_spark.py:310)       */
#define KM_STOP_EMPTY 2     /* empty clusters: host repair (kmeans_spark.py:191)  */
#define KM_STOP_NONFINITE 3 /* NaN/Inf centroid (kmeans_spark.py:289)            */
/* Iterations per batch (km_batch_begin .. km_batch_end). */
#define KM_MAX_BATCH 32

/* Static facts about a context (for logging / benchmarks). */
typedef struct km_info {
  int64_t n;         /* local rows                                    */
  int32_t d, dp;     /* features, padded row stride                   */
  int32_t k, kp;     /* clusters, padded to a multiple of 64          */
  int32_t path;      /* 1 = small direct-form path, 2 = MFMA fp16x3 screen
                        (k_fused / k_assign_mfma; k_assign_wide for dp > 256) */
  int32_t n_cu;      /* compute units of the device                   */
  int32_t device;
  int32_t fused_stats;
  int32_t delta_stats; /* ABI 6: the last km_assign_stats left changes since the
                          previous assignment in the stats buffer (delta
                          statistics, see km_assign_stats), not full sums */
} km_info;

/* Kernel kinds for km_prof_read. */
#define KM_K_ASSIGN 0
#define KM_K_RESOLVE 1
#define KM_K_STATS 2
#define KM_K_UPDATE 3
#define KM_K_PREP 4
#define KM_K_SEED 5 /* k_seed_fold of km_seed_update (added within ABI 6) */
#define KM_K_COUNT 6

int km_abi_version(void);
const char* km_last_error(void);
int km_device_count(int* out);

/* Context lifetime.  Replaces the SparkContext / executor set-up
 * (kmeans_spark.py:626) for one GPU. */
int km_create(int device, km_ctx** out);
int km_destroy(km_ctx* ctx);
/* Enqueue on an external stream (e.g. torch.cuda.current_stream()); NULL =
 * the context's own stream. */
int km_set_stream(km_ctx* ctx, void* hip_stream);
int km_sync(km_ctx* ctx);
int km_info_get(km_ctx* ctx, km_info* out);
/* Row gate of the delta statistics (fused k_s1 geometries, compute_sse off):
 * a row whose stored margin proves that its label cannot have changed since
 * the previous assignment is not screened at all.  *out = the rows the last
 * km_assign_stats did screen (n on the first gated pass and after anything
 * that invalidates the margins: new centroids or rows, a predict, a full
 * statistics pass, an empty-cluster repair), or -1 when that pass was not
 * gated.  Synchronises the stream.  (Added within ABI 6: a new entry point,
 * no existing layout changes.) */
int km_gated_rows(km_ctx* ctx, int64_t* out);
/* Which statistics pass the next km_assign_stats with FULL statistics runs
 * for the current geometry and weight mode (read-only; needs centroids):
 *   *route = 0  inside the assign kernel (small path, fused path);
 *            1  the range-tiled LDS table (k_stats, weighted or not);
 *            2  the counting sort and segment sums (k_segsum, weighted or not).
 * For routes 1 and 2 the split of the table: *fr features and *kr clusters
 * per workgroup, *feature_ranges = dp / fr and *cluster_ranges =
 * ceil(k / kr) of them (route 2 sorts because the table would need that
 * many cluster ranges); all four are 0 for route 0.  A delta-statistics pass
 * (km_info.delta_stats) folds its change list instead and is not described.
 * The values are the ones the dispatch itself reads, not a second
 * computation.  (Added within ABI 6: a new entry point, no layout changes.) */
int km_stats_route(km_ctx* ctx, int32_t* route, int32_t* cluster_ranges, int32_t* kr, int32_t* feature_ranges,
                   int32_t* fr);

/* Materialise this rank's rows in HBM once: replaces sc.parallelize(X) +
 * rdd.cache() (kmeans_spark.py:256, 369, 418, 471, 518, 568).  km_load_begin
 * allocates n rows of d features; km_load_rows copies host float32 rows
 * [row0, row0 + nrows) (pinned staging, chunked). */
int km_load_begin(km_ctx* ctx, int64_t n, int32_t d);
int km_load_rows(km_ctx* ctx, int64_t row0, const float* rows, int64_t nrows);
/* The device-source twin of km_load_rows (a torch tensor already in HBM):
 * dev_rows is a row-major [nrows][d] array of dtype elements in device memory
 * of the context's GPU, row stride src_stride_elems >= d elements, unit column
 * stride; any base alignment (an aligned base and row stride select the
 * vector-load instance of the kernel).  One kernel (k_ingest, km_ingest.hip)
 * converts the rows into the row store: fp16 and bf16 widen exactly, fp64
 * rounds to nearest-even as the host route's conversion to float32 does (out
 * of range -> +-inf, NaN stays NaN, the sign of zero is kept, subnormals are
 * rounded, not flushed), so the stored rows, and the data maximum and row
 * norms computed from them, hold the bits a km_load_rows of the same float32
 * values leaves.  Like km_load_rows it flushes a deferred assign, invalidates
 * delta statistics and the row gate, runs on the context's stream and
 * synchronises it before returning: the caller may then free or overwrite the
 * source, and must itself have finished the work that produced it (the
 * context's stream is not ordered after any other).
 * KM_ERR_STATE before km_load_begin; KM_ERR_ARG for rows out of range, an
 * unknown dtype, src_stride_elems < d, a null pointer with nrows > 0, a
 * pointer that hipPointerGetAttributes does not report as device memory of
 * the context's GPU (the message names both devices), and a source, from its
 * first byte to the last one of the last row, that does not lie inside the
 * one device allocation holding the pointer (hipMemGetAddressRange; where the
 * runtime reports no single range, the last byte is looked up like the
 * first): a wrong pointer, stride or row count is an error code, not a GPU
 * fault.  What the check cannot see is memory freed by the caller while the
 * call runs.  nrows == 0 returns KM_OK and does nothing.
 * (Added within ABI 6: new entry points, no existing layout changes.) */
#define KM_DT_F32 0
#define KM_DT_F64 1
#define KM_DT_F16 2
#define KM_DT_BF16 3
int km_load_device(km_ctx* ctx, int64_t row0, const void* dev_rows, int64_t nrows, int64_t src_stride_elems,
                   int32_t dtype);
/* Synthetic Gaussian blobs generated in HBM, keyed by global row (benchmarks). */
int km_generate_blobs(km_ctx* ctx, int64_t n, int32_t d, int64_t global_row0, int32_t n_centers, float box,
                      float stddev, uint64_t seed);
/* Row weights (fit(..., sample_weight=w); MLlib's weightCol): float64, one
 * per local row, kept in HBM as float64 (8 bytes per row).  km_set_weights
 * copies host weights of rows [row0, row0 + nrows) (chunked like
 * km_load_rows; rows never set weigh 1) and puts the context in weighted
 * mode; KM_ERR_STATE before km_load_begin and inside a batch.  The caller
 * guarantees finite, strictly positive weights: with w > 0 a cluster is empty
 * exactly when it holds no row, so the empty-cluster policy, the device
 * repair and the reported cluster sizes (row counts) are unchanged.
 * In weighted mode km_assign_stats computes the same labels (the labels-only
 * assignment of km_predict, exact on every path) and then runs one weighted
 * statistics pass over the rows (X is read twice per iteration); delta
 * statistics, the row gate, the small path's folded update and the k_s1 SSE
 * correction are off (km_info.delta_stats = 0).  The stats buffer becomes
 * float64 [k][d+1]: per-cluster sum of w x, then the ROW count; the SSE slot
 * (sum of w ||x - c_label||^2 with km_set_sse); then k more doubles, the
 * clusters' sums of weights W.  km_stats_buffer reports the length
 * k (d+1) + 1 + k and a buffer bound with km_bind_stats_buffer must hold as
 * many: one sum all-reduce per iteration still suffices.  km_update /
 * km_update_async divide by W where the row count is positive and keep the
 * old centroid elsewhere; status, counts, batches and repairs are as without
 * weights.  km_predict is unaffected.
 * km_clear_weights returns to unweighted mode (a no-op without weights).
 * Entering or leaving weighted mode changes the buffer's length: an external
 * stats buffer is unbound (the context's own is current; bind again).
 * km_load_begin, km_generate_blobs and km_destroy release the weights.
 * (Added within ABI 6: new entry points, no existing layout changes.) */
int km_set_weights(km_ctx* ctx, int64_t row0, const double* w, int64_t nrows);
int km_clear_weights(km_ctx* ctx);
/* Local sum_p x_p of the resident rows (float64 [d]; integrity checks). */
int km_sum_x(km_ctx* ctx, double* out_d);
/* compute_sse (kmeans_spark.py:38, 278-286): when enabled, km_assign_stats
 * also adds every row's float64 residual ||x - c_label||^2 to the SSE slot of
 * the stats buffer, in the same pass over the rows that assigns them
 * (replaces _compute_sse's second pass, :208-237). */
int km_set_sse(km_ctx* ctx, int32_t enable);

/* Set the current centroids: replaces sc.broadcast(self.centroids)
 * (kmeans_spark.py:268, 340). */
int km_set_centroids(km_ctx* ctx, const double* C, int32_t k, int32_t d);
/* Read centroids: which = 0 current, 1 the update's new centroids. */
int km_get_centroids(km_ctx* ctx, int32_t which, double* out);

/* Assignment + partial statistics of one iteration: replaces
 * rdd.mapPartitions(assign_partition) + the map-side combine of
 * reduceByKey (kmeans_spark.py:147-171).  Output = the stats buffer
 * (float64 [k][d+1]: per-cluster sum of x, then count; then one SSE slot,
 * 0 unless km_set_sse is on).
 * Delta statistics (ABI 5, the k_s1 screen's geometries, compute_sse off):
 * from the second iteration after new centroids / rows / a predict, the
 * buffer holds only the CHANGES since the previous assignment (rows that
 * moved: -x, -1 on the old cluster, +x, +1 on the new one), and the context
 * keeps the full sums itself; the update folds the (all-reduced) changes
 * into them.  Summing the buffer over ranks is valid either way (every rank
 * takes the same path: the choice depends on the call sequence and the
 * geometry only).  After a batch update the buffer is zero.  A caller that
 * reads the sums themselves takes the buffer with km_stats_buffer, which
 * turns delta statistics off for the context (full sums every iteration). */
int km_assign_stats(km_ctx* ctx);
/* The stats buffer (device) and its length in doubles, k (d+1) + 1; a caller
 * may bind an external device buffer instead (e.g. a torch tensor it
 * all-reduces): this is the reduceByKey shuffle + collect
 * (kmeans_spark.py:169-173) and the partition-SSE .sum() (:237).
 * km_stats_buffer: the buffer then always holds full sums after
 * km_assign_stats (delta statistics off).  km_bind_stats_buffer keeps delta
 * statistics on: the bound buffer carries the sums or the changes as
 * described at km_assign_stats, which is what a sum all-reduce needs. */
int km_stats_buffer(km_ctx* ctx, void** dev_ptr, int64_t* len);
int km_bind_stats_buffer(km_ctx* ctx, void* dev_ptr);

/* Centroid update from the (all-reduced) stats: replaces _update_centroids
 * (kmeans_spark.py:176-206), reads the SSE slot (:208-237) and computes the
 * shifts (:293-294).  Synchronises; fills *st and counts[k].
 * Returns KM_EMPTY when clusters are empty (their new centroid is the old
 * one until km_replace_rows). */
int km_update(km_ctx* ctx, km_status* st, int64_t* counts);
/* The dataset's partition layout for rdd.takeSample (sizes[nparts] in row
 * order; this context's rows start at global row row0).  device_repair = 1
 * (one context holding every row) moves the empty-cluster repair of
 * kmeans_spark.py:191-204 onto the device inside batches: after an update
 * with empty clusters, takeSample(False, n_empty, empty_seed) runs there
 * (PySpark's fraction, per-partition Bernoulli passes with CPython's MT19937,
 * shuffle; one pass, no retry), its rows replace the empty clusters and their shifts enter
 * max_shift, without stopping the batch (km_status.repaired = 1).  Otherwise
 * (or if a pass overflows its slots or comes back short: the device does not
 * retry PySpark's resampling loop) empty clusters stop the batch and the
 * caller repairs them on the host with the same policy.
 * The layout belongs to the loaded rows: km_load_begin (and with it
 * km_generate_blobs) ends it, with the device repair and its buffers, as a
 * new km_set_layout does; set it again after every load. */
int km_set_layout(km_ctx* ctx, const int64_t* sizes, int32_t nparts, int64_t row0, int32_t device_repair);
/* device_repair = 2 (ABI 4): the rows are spread over ranks, this context
 * holding global rows [row0, row0 + n).  Every rank runs the same takeSample
 * passes over all partitions (index level), so all pick the same rows; then,
 * for an iteration whose km_update_async left the repair waiting
 * (km_repair_state: waiting = 1), the caller sum-all-reduces the repair
 * buffer (km_repair_buffer: k*d doubles, each rank contributing the picked
 * rows it holds and zeros) on the context's stream, and km_repair_apply_async
 * puts the rows in place and finishes the iteration -- no host round trip.
 * Replaces the driver-side takeSample + broadcast of kmeans_spark.py:191-204
 * when the rows sit on several GPUs.  The seed passed to km_update_async must
 * be the same on every rank. */
int km_repair_state(km_ctx* ctx, int32_t* armed, int32_t* waiting);
int km_repair_buffer(km_ctx* ctx, void** buffer, int64_t* len);
/* use an external device buffer of k*d doubles (e.g. a torch tensor that the
 * process group all-reduces); NULL restores the context's own */
int km_bind_repair_buffer(km_ctx* ctx, void* buffer);
int km_repair_apply_async(km_ctx* ctx);
/* Batches of Lloyd iterations without host synchronisation (replaces the
 * per-iteration driver round trip of kmeans_spark.py:266-313).  Between
 * km_batch_begin and km_batch_end the caller enqueues up to KM_MAX_BATCH
 * iterations, each km_assign_stats [+ its all-reduce of the stats buffer] +
 * km_update_async(tol, empty_seed) (empty_seed: int(time.time()), the seed
 * of kmeans_spark.py:196 for an on-device repair); km_update_async also
 * commits speculatively.  The
 * device records every iteration (status, counts) and, on convergence
 * (max_shift < tol), empty clusters or non-finite centroids, raises a gate
 * that turns the rest of the batch into no-ops.  km_batch_end synchronises
 * once, returns the records of the iterations that ran (*n_ran of them:
 * st[i], counts[i*k .. i*k+k)) and leaves the context as km_update would
 * after the last of them: km_replace_rows / km_commit apply to it. */
int km_batch_begin(km_ctx* ctx);
int km_update_async(km_ctx* ctx, double tol, int64_t empty_seed);
int km_batch_end(km_ctx* ctx, km_status* st, int64_t* counts, int32_t* n_ran);
/* Empty-cluster repair (kmeans_spark.py:196-204): overwrite new centroids
 * of the given clusters with the given rows (float64 [n][d]). */
int km_replace_rows(km_ctx* ctx, const int32_t* cluster_ids, const double* rows, int32_t n);
/* Commit the new centroids (kmeans_spark.py:307). */
int km_commit(km_ctx* ctx);

/* Rows by local index (float64 [n][d]): the rows behind rdd.takeSample
 * (kmeans_spark.py:72, 196). */
int km_gather_rows(km_ctx* ctx, const int64_t* local_idx, int32_t n, double* out);

/* Bernoulli pass of rdd.takeSample(False, num, seed) (kmeans_spark.py:72,
 * 196; PySpark RDD.takeSample + RDDSampler): for each of the nparts given
 * partitions, row i is kept when the i-th double of Python's
 * random.Random(seeds[p]) (seeds[p] = takeSample seed ^ partition index,
 * after ten randint(0, 1) warm-up draws) is < fraction.  One wave per
 * partition on this context's GPU.  out[0..*n_out): global row indices
 * bases[p] + i, partitions in the given order, rows ascending.  KM_ERR_ARG
 * when a partition yields more picks than the device pass holds (4x the
 * expectation + 64) or *n_out would exceed cap: the caller then samples on
 * the host. */
int km_bernoulli_sample(km_ctx* ctx, const uint64_t* seeds, const int64_t* sizes, const int64_t* bases,
                        int32_t nparts, double fraction, int64_t* out, int64_t cap, int64_t* n_out);

/* Labels of every local row for the current centroids: replaces predict's
 * assign_partition (kmeans_spark.py:343-350). */
int km_predict(km_ctx* ctx, int32_t* labels_out);
/* Labels of the last km_assign_stats (device -> host). */
int km_labels(km_ctx* ctx, int32_t* labels_out);
/* km_labels with a device destination: n int32 copied device to device on the
 * context's stream, then synchronised (km_predict(ctx, NULL) followed by this
 * call leaves predictions in HBM with no host copy).  KM_ERR_STATE without
 * data; KM_ERR_ARG for a null pointer with n > 0 and for a destination that is
 * not device memory of the context's GPU (checked as in km_load_device).
 * (Added within ABI 6.) */
int km_labels_device(km_ctx* ctx, int32_t* dev_out);

/* k-means|| seeding (Bahmani et al. 2012): an initialisation the reference
 * does not have (its only one is takeSample, kmeans_spark.py:58-82); the
 * algorithm is stated in seeding.py.  The passes over the local rows run
 * here, the round loop and the weighted recluster of the candidates on the
 * host.  (Added within ABI 6: new entry points, no existing layout changes.)
 * Every call returns KM_ERR_STATE before km_load_begin, and every call but
 * km_seed_begin before km_seed_begin.  A context with 0 rows is valid (phi 0,
 * no picks, zero counts).  The state is independent of the Lloyd state: it
 * survives km_set_centroids and is released by km_seed_end, km_load_begin,
 * km_generate_blobs and km_destroy.
 *
 * km_seed_begin: per local row, D2 (float64, the squared distance to the
 * nearest candidate so far; starts at +inf) and near (int32, that candidate's
 * id; starts at -1): 12 bytes per row. */
int km_seed_begin(km_ctx* ctx);
/* Fold a batch of m new candidates, the current centroids (km_set_centroids
 * with k = m), ids first_id .. first_id + m - 1, into the state.  Per row:
 * j = np.argmin(np.linalg.norm(C - x, axis=1)) by the labels-only assignment
 * of km_predict (the context is left as after km_predict(ctx, NULL); delta
 * statistics are invalidated); t = np.add.reduce((C[j] - x) * (C[j] - x)) in
 * float64, NumPy's pairwise order, no fused multiply-add; if t < D2 then
 * D2 = t, near = first_id + j (the earliest candidate keeps ties, a NaN never
 * replaces a value).  *phi_local = the sum of D2 over the local rows, in a
 * fixed order (bit-identical between identical calls).  Synchronises. */
int km_seed_update(km_ctx* ctx, int32_t first_id, double* phi_local);
/* The pick rule of one round over the local rows: row i (global index
 * g = global_row0 + i) is picked iff u * phi < ell * D2[i], both products
 * rounded in float64, u = (h >> 11) * 2^-53,
 * h = splitmix64(splitmix64(seed ^ (round * 0xD1B54A32D192ED03 mod 2^64)) ^ g).
 * out[0..*n_out): local indices, ascending.  KM_ERR_ARG when the picks exceed
 * cap (*n_out = their number; out is not written): the caller then applies
 * the rule itself to km_seed_read's D2. */
int km_seed_sample(km_ctx* ctx, uint64_t seed, int32_t round, int64_t global_row0, double ell, double phi,
                   int64_t* out, int64_t cap, int64_t* n_out);
/* counts_out[j] = local rows with near == j, j < m_total. */
int km_seed_weights(km_ctx* ctx, int32_t m_total, int64_t* counts_out);
/* The state to the host (d2_out[n], near_out[n]); either may be NULL. */
int km_seed_read(km_ctx* ctx, double* d2_out, int32_t* near_out);
/* Release the state. */
int km_seed_end(km_ctx* ctx);

/* Screening kernel.  A cost choice: labels, sums and SSE are exact in every
 * mode.  -1 (default): the one-MFMA screen k_s1 (mode 4) wherever the
 * geometry has an instance, else mode 5 on the unfused path (dp a multiple
 * of 32), else per batch from the last iteration's queue fraction; 0: fp16x3
 * screen, global bound; 1: fp16x3 with per-key bounds (0 and 1 keep
 * k_fused16 with full statistics on every iteration, and the fp16x3
 * k_assign_mfma16 on the unfused path); 4 (ABI 5): k_s1, one fp16 MFMA per
 * product, candidates re-scored exactly in fp32 inside the kernel, delta
 * statistics on the fused geometries (the first iteration after new data,
 * centroids or a predict still runs the fp16x3 screen with full statistics;
 * with compute_sse every iteration does), labels then the statistics pass on
 * the unfused ones; 5 (ABI 5): one fp16 MFMA per product in the unfused
 * k_assign_mfma16 with the one-part bound, the rows it cannot settle going
 * to the float64 resolvers (candidate lists).  Modes 2 and 3 (fast screen:
 * one fp16 MFMA per product, pairwise bound; 3 with the row split hi + lo)
 * exist in the diagnostic library only (libkmeans_amd_diag.so, make diag);
 * the product library returns KM_ERR_UNSUPPORTED for them. */
#define KM_SCREEN_AUTO (-1)
#define KM_SCREEN_S1 4
#define KM_SCREEN_ONE 5
int km_set_screen(km_ctx* ctx, int32_t mode);
/* The screen the next assign with statistics uses (0..5). */
int km_get_screen(km_ctx* ctx, int32_t* mode);

/* Kernel timing with HIP events on the context stream.  `enable` is a
 * bitmask of (1 << KM_K_*) phases to time (-1: all, 0: off). */
int km_profile(km_ctx* ctx, int32_t enable);
/* Time one launch in `period` (>= 1, default 1) of each profiled phase: each
 * timed launch costs ~6 us of stream time, which a 0.16 ms c2 step notices. */
int km_profile_every(km_ctx* ctx, int32_t period);
int km_prof_read(km_ctx* ctx, int32_t kind, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* KMEANS_AMD_H */
