/*
 * icp_mi355x.h -- C ABI of the MI355X (gfx950) ICP registration core.
 *
 * Drop-in boundary for the hot path of tier4/icp_rust: the reference has no FFI of its
 * own; its boundary is the crate's public Rust API (src/lib.rs:12-26).  Each entry
 * point below names the Rust item (file:line under /root/reference) it stands in for.
 * INTEGRATION.md shows the `extern "C"` block + safe wrappers a maintainer adds to the
 * crate so that `Icp2d`, `Icp3d`, `Transform`, `estimate_transform`, ... keep their
 * signatures.  Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * Conventions
 *  - points are dense AoS doubles exactly as `&[Vector2]` / `&[Vector3]` lie in memory
 *    (nalgebra ArrayStorage<f64, D, 1>: stride 16 B / 24 B), src/types.rs:4-12;
 *  - `icp_pose` is `Transform { rot: Rotation2, t: Vector2 }` (src/transform.rs:6-10),
 *    rotation column-major as nalgebra stores it;
 *  - every function returns an icp_status; the reference's `None` is ICP_NONE, its two
 *    panics (empty dst: src/lib.rs:122,165; NaN residual: src/stats.rs:12) are
 *    ICP_EMPTY_DST / ICP_NAN_INPUT;
 *  - one in-flight call per handle (it owns scratch + a HIP stream); handles are
 *    independent.  Entry points that take DEVICE pointers run on the handle's private,
 *    non-blocking streams unless icp_set_stream was called: the buffers they read must be
 *    complete when the call is made (synchronise the stream that produced them, or put the
 *    handle on that stream with icp_set_stream -- then everything is ordered there).  When a
 *    call returns, whatever its status, none of its work is still in flight on the caller's
 *    buffers.  All compute runs on the GPU: without a usable HIP device every
 *    compute entry point returns ICP_NO_DEVICE -- there is no CPU fallback.
 */
#ifndef ICP_MI355X_H
#define ICP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: additions only (sharded stage calls, icp_multi, single-launch switch, point-to-plane extension, icp_f64_sin/cos);
 * everything of version 1 is unchanged */
/* 3: additions only (icp_last_fold_order; icp_sort_source_device).  Behavioural note: icp_estimate[_device] on the grid
 * engine now folds its sums over the source cloud in FOLD ORDER (a deterministic sort by target-grid cell, section 9a)
 * instead of the caller's order -- same correspondences, pose equal within the rounding of a re-ordered sum (~1e-12) */
/* 4: the sharded evaluation has TWO exchanges: icp_shard_eval_accumulate_device is gone, icp_shard_eval_compact_device
 * hands out one block per rank (candidates + block sums, icp_shard_exchange_bytes) and icp_shard_eval_finish_device
 * takes the gathered blocks.  Additions: icp_shard_exchange_bytes, icp_nn_cert_counters, icp_multi_append_targets,
 * icp_grid_append_counters.  Behavioural note: the sums of the weighted normal equations are kept per dimension and
 * scaled by 1 / sigma after the fold (g_x S_x + g_y S_y) instead of per term -- pose equal within rounding (~1e-13) */
/* 5: additions only (section 5b: the one-launch sharded inner loop -- icp_loop_inbox*, icp_loop_ipc_*,
 * icp_shard_loop_*; icp_multi_compute/update_target_normals, icp_multi_estimate_point_to_plane).  The counters and
 * icp_profile_* moved to icp_mi355x_debug.h (same symbols, same library).  Behavioural note: clouds of at most 2^20
 * points run their inner loop inside one launch; results are the same bits as the stepped loop's */
/* 6: icp_loop_inbox takes the KIND of memory (ICP_INBOX_*: 0 and 1 are what `fine_grained` 0 / 1 meant); additions:
 * ICP_INBOX_HOST and icp_loop_inbox_shm_name / _shm_unlink / icp_loop_shm_open / _shm_close (inboxes in pinned host
 * memory shared between processes), icp_loop_transport_probe, icp_reset_window_predictions.  Behavioural notes: a
 * sharded one-launch inner loop that gives up raises the abort word in every rank's inbox, so all ranks report
 * ICP_HIP_ERROR for that launch; the evaluations of icp_estimate[_device] file their candidates in the first pass over
 * the pairs and finish in one workgroup (same bits: the order statistics are exact either way) */
/* 7: additions only (section 5c: icp_shard_pipe_run_device, the pipelined sharded registration; icp_pipe_counters,
 * icp_multi_pipe_iterations in icp_mi355x_debug.h).  Behavioural note: icp_multi_estimate and the sharded drivers serve
 * the steady state of a registration through it (same bits) */
/* 8: additions only (section 8: icp_batch_*, many small registrations in one launch; icp_batch_counters in
 * icp_mi355x_debug.h).  Everything of version 7 is unchanged.  Section 9 (icp_quality, icp_evaluate*,
 * icp_batch_evaluate*; icp_batch_evaluate_counters in icp_mi355x_debug.h) was added later without a bump: an addition
 * detectable by symbol; so was section 10 (icp_estimate_gated*, icp_gate_pairs_device); so was section 11
 * (icp_crop_targets, icp_multi_crop_targets; icp_grid_crop_counters in icp_mi355x_debug.h); so was section 12
 * (icp_estimate_point_to_plane_gated*, icp_gate_plane_pairs_device, icp_multi_estimate_point_to_plane_gated); so was
 * section 13 (icp_plane_quality, icp_evaluate_point_to_plane*); so was section 14 (icp_*_target_line_normals,
 * icp_estimate_point_to_line*); so was section 15 (icp_batch_estimate_point_to_line*; icp_batch_line_counters in
 * icp_mi355x_debug.h); so was section 16 (icp_line_quality, icp_evaluate_point_to_line*,
 * icp_batch_evaluate_point_to_line*; icp_batch_line_quality_counters in icp_mi355x_debug.h); so was section 17
 * (icp_batch_estimate_point_to_line_gated*; icp_batch_line_gated_counters in icp_mi355x_debug.h); so was section 18
 * (icp_batch_estimate_point_to_plane*; icp_batch_plane_counters in icp_mi355x_debug.h); so was section 19
 * (icp_batch_estimate_point_to_plane_gated*; icp_batch_plane_gated_counters in icp_mi355x_debug.h); so was section 20
 * (icp_batch_evaluate_point_to_plane*; icp_batch_plane_quality_counters in icp_mi355x_debug.h); so was section 21
 * (icp_batch_estimate_gated*; icp_batch_gated_counters in icp_mi355x_debug.h); so was section 22
 * (icp_voxel_downsample*, icp_thin_targets, icp_multi_thin_targets; icp_grid_thin_counters in icp_mi355x_debug.h) */
#define ICP_ABI_VERSION 8

typedef enum icp_status {
  ICP_OK = 0,
  ICP_NONE = 1,        /* Option::None (src/lib.rs:67-69, 186-189, 257-260)           */
  ICP_EMPTY_DST = 2,   /* reference panics: index.unwrap(), src/lib.rs:122,165        */
  ICP_NAN_INPUT = 3,   /* reference panics: partial_cmp().unwrap(), src/stats.rs:12   */
  ICP_BAD_ARGUMENT = 4,
  ICP_NO_DEVICE = 5,   /* HIP runtime/device unavailable -- no CPU fallback exists    */
  ICP_HIP_ERROR = 6,
  ICP_OUT_OF_MEMORY = 7,
  ICP_RETRY_REPLICATED = 8, /* sharded evaluation (section 5): evaluate this one on the gathered pairs */
  ICP_RETRY_SHARDED = 9     /* sharded evaluation: the window missed; hist again with refined = 1      */
} icp_status;

/* Transform (src/transform.rs:6-10) */
typedef struct icp_pose {
  double r00, r10, r01, r11; /* Rotation2, column-major */
  double tx, ty;             /* Vector2                 */
} icp_pose;

/* constants of the path (read-only; src/lib.rs:32,60,61, src/stats.rs:42) */
#define ICP_HUBER_K 1.345
#define ICP_DELTA_NORM_THRESHOLD 1e-6
#define ICP_INNER_MAX_ITER 200
#define ICP_PPF34 1.482602218505602

/* nearest-neighbour engines: identical results (exact NN, d^2 = ((dx^2+dy^2)+dz^2)
 * without FMA, ties -> lowest index), different cost. */
typedef enum icp_nn_mode {
  ICP_NN_AUTO = 0,
  ICP_NN_BRUTE = 1, /* LDS-tiled brute force, O(N*M) f64                              */
  ICP_NN_GRID = 2   /* exact uniform-grid search built on device at icp_create        */
} icp_nn_mode;

const char *icp_status_string(int status);
int icp_abi_version(void);
/* number of usable HIP devices (0 on a CPU-only host; never initialises a context) */
int icp_device_count(void);
/* the PCI bus id of a device ("0000:c1:00.0"): what tells two devices of one node apart whatever ordinal a process sees
 * them under (the sharded drivers pick the transport of their inboxes by it) */
int icp_device_pci_bus_id(int device, char out[64]);

/* ================================================================================
 * 1. Host-side pose algebra: Transform / se2 / so2 (tiny, runs on the host exactly as
 *    in the reference; exported so the host mirror and the tests share one definition)
 * ============================================================================== */
void icp_transform_new(const double param[3], icp_pose *out);      /* Transform::new, transform.rs:13-16 -> se2::calc_rt se2.rs:21-41 */
void icp_transform_from_rt(const double rot_colmajor[4], const double t[2], icp_pose *out); /* transform.rs:18-20 */
void icp_transform_identity(icp_pose *out);                        /* transform.rs:34-39 */
void icp_transform_apply(const icp_pose *T, const double p[2], double out[2]);   /* Transform::transform, transform.rs:22-24 */
void icp_transform_inverse(const icp_pose *T, icp_pose *out);      /* transform.rs:26-32 */
void icp_transform_mul(const icp_pose *lhs, const icp_pose *rhs, icp_pose *out); /* impl Mul, transform.rs:42-51 */
void icp_se2_exp(const double param[3], double m3_rowmajor[9]);    /* se2::exp, se2.rs:43-52 */
void icp_se2_log(const double m3_rowmajor[9], double param[3]);    /* se2::log, se2.rs:54-77 */
void icp_se2_get_rt(const double m3_rowmajor[9], double rot_rowmajor[4], double t[2]); /* se2::get_rt, se2.rs:11-19 */
void icp_so2_exp(double theta, double m2_colmajor[4]);             /* so2::exp / new_rotation2, so2.rs:8-31 */
double icp_so2_log(const double m2_colmajor[4]);                   /* so2::log, so2.rs:19-21 */
double icp_norm(const double *m_colmajor, size_t nrows, size_t ncols); /* icp::norm, norm.rs:19-21 */
int icp_inverse3x3(const double m_rowmajor[9], double out_rowmajor[9]); /* linalg::inverse3x3, linalg.rs:3-29 (ICP_NONE iff det == 0) */
/* f64::sin / f64::cos as the reference's no_std build evaluates them (num-traits `libm` feature,
 * Cargo.toml:17-20 -> the libm crate, a port of musl's kernels; restated in icp_trig.h).  Host and
 * device share the definition: the inner loop's pose updates (Transform::new, src/lib.rs:81) run
 * on the GPU and must give the bits the host API gives. */
double icp_f64_sin(double x);
double icp_f64_cos(double x);
/* Transform::new on the DEVICE for n parameter vectors (host buffers in and out; test / observability
 * entry: proves that device and host evaluate se2::calc_rt to the same bits) */
int icp_transform_new_device(const double *params_xyz, size_t n, icp_pose *out, int device);

/* ================================================================================
 * 2. The registration handle: Icp2d / Icp3d
 * ============================================================================== */
typedef struct icp_handle icp_handle;

/* Icp2d::new (src/lib.rs:97-102) / Icp3d::new (src/lib.rs:139-144).  dim = 2 | 3.
 * Copies `dst` (m points, AoS) to the device and builds the search structure there, so
 * `dst` may be freed afterwards (stricter than the reference's borrow `'a`, never
 * weaker).  device < 0 selects the current HIP device. */
int icp_create(icp_handle **out, int dim, const double *dst, size_t m, int device);
/* same, but `d_dst` already lives in device memory (m x dim doubles, AoS); it is
 * borrowed for the lifetime of the handle, like the reference's `&'a [Vector]`. */
int icp_create_device(icp_handle **out, int dim, const double *d_dst, size_t m, int device);
void icp_destroy(icp_handle *h);

/* Clouds of the reference's own size (scans/2d: ~650 points; here: up to 1024 source points against up
 * to 2048 targets) are registered by icp_estimate[_device] in ONE launch of one workgroup -- search,
 * inner loop, 3x3 solve, break tests and pose updates all on the device, same bits as the general
 * path.  icp_set_single_launch(h, 0) switches that off for a handle (tests, A/B); the counters:
 * out[0] calls served, out[1] Gauss-Newton evaluations in them, out[2] of which needed the sorting path. */
int icp_set_single_launch(icp_handle *h, int enable);
int icp_set_nn_mode(icp_handle *h, int mode);   /* icp_nn_mode; default ICP_NN_AUTO */
int icp_get_nn_mode(const icp_handle *h);       /* the engine AUTO resolved to      */
/* run the handle's kernels on a caller-chosen HIP stream (hipStream_t) instead of the handle's
 * own non-blocking stream.  NULL is the HIP default (null) stream -- what torch.cuda's default
 * stream is -- not "reset".  Used by hosts that interleave their own device work (e.g. RCCL
 * collectives, torch ops) with the stage-level calls of section 4: everything is then ordered
 * on that one stream.  icp_use_own_stream goes back to the private stream. */
int icp_set_stream(icp_handle *h, void *hip_stream);
int icp_use_own_stream(icp_handle *h);

/* Icp2d::estimate (src/lib.rs:105-130) / Icp3d::estimate (src/lib.rs:148-173):
 * the result of exactly `max_iter` outer iterations of transform -> exact NN -> estimate_transform
 * -> compose.  (An iteration that applies no update and returns the pose it was given, bit for bit, is a fixed point:
 * the iterations after it would repeat it and are not run, except the last, which reports the correspondences; their
 * inner counts are 0, as they would be.  icp_fixed_point_skips, icp_mi355x_debug.h, counts them.)
 * src: n points AoS (host).  Optional outputs (NULL to skip):
 *   last_idx[n]          correspondence indices of the last outer iteration,
 *   inner_iters[max_iter] inner Gauss-Newton updates applied per outer iteration. */
int icp_estimate(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                 size_t max_iter, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters);
/* same with `d_src` (and optional d_last_idx) resident in device memory */
int icp_estimate_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                        size_t max_iter, icp_pose *out, uint32_t *d_last_idx,
                        uint32_t *inner_iters);

/* ================================================================================
 * 3. The robust pose estimator as free functions (host buffers; a, b are n x 2 AoS)
 * ============================================================================== */
/* icp::estimate_transform, src/lib.rs:59-84.  inner_iters (nullable) = updates applied */
int icp_estimate_transform(const double *a_xy, const double *b_xy, size_t n, icp_pose *out,
                           uint32_t *inner_iters);
/* icp::weighted_gauss_newton_update, src/lib.rs:218-261 (ICP_NONE where it returns None) */
int icp_weighted_gauss_newton_update(const icp_pose *T, const double *a_xy, const double *b_xy,
                                     size_t n, double delta[3]);
/* icp::gauss_newton_update, src/lib.rs:191-216 */
int icp_gauss_newton_update(const icp_pose *T, const double *a_xy, const double *b_xy, size_t n,
                            double delta[3]);
/* icp::error, src/lib.rs:38-43 and icp::huber_error, src/lib.rs:45-50 */
int icp_error(const icp_pose *T, const double *a_xy, const double *b_xy, size_t n, double *out);
int icp_huber_error(const icp_pose *T, const double *a_xy, const double *b_xy, size_t n, double *out);
/* stats::calc_stddevs over the residuals T*a - b (src/stats.rs:49-60, called at
 * src/lib.rs:236): sigma[2] = 1.4826 * MAD per dimension.  Exposed for parity tests. */
int icp_residual_stddevs(const icp_pose *T, const double *a_xy, const double *b_xy, size_t n,
                         double sigma[2]);

/* ================================================================================
 * 4. Stage-level calls on device memory (what a multi-GPU host composes: shard the
 *    source cloud over ranks, all-gather the matched pairs, replicate the tiny solve)
 * ============================================================================== */
/* stage (i) of one outer iteration, src/lib.rs:113-124 / 156-167 (+ get_xy :86-89):
 * s' = T (.) src; idx = NN(s'); a = xy(s'); b = xy(dst[idx]).  d_src: n x dim AoS;
 * d_a, d_b: n x 2 AoS out; d_idx: n out (nullable).  Asynchronous on the handle's
 * stream. */
int icp_correspond_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                          double *d_a_xy, double *d_b_xy, uint32_t *d_idx);
/* a = xy(T (.) src), b = xy(dst[idx]) for n points from given correspondence indices -- the
 * second half of icp_correspond_device on its own.  A multi-GPU host that replicates the source
 * cloud all-gathers only the 4-byte indices of each rank's shard (instead of 32 bytes of pairs
 * per point) and rebuilds the pairs locally with this call; same arithmetic, same bits. */
int icp_materialize_pairs_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                 const uint32_t *d_idx, double *d_a_xy, double *d_b_xy);
/* Optional, before a run of icp_correspond_device calls on the same source buffer: takes a
 * cell-sorted snapshot of (d_src, n) under pose T so that neighbouring GPU lanes search
 * neighbouring cells (results are unchanged, bit for bit; only memory locality changes).
 * The snapshot is used by later icp_correspond_device calls with the same (d_src, n) and
 * must be retaken if the buffer's contents change.  icp_estimate* do this themselves. */
int icp_prepare_source_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T);
/* stage (ii)+(iii): the whole inner loop of src/lib.rs:59-84 on device-resident pairs;
 * synchronises the stream (the 3x3 solve and the break tests run on the host). */
int icp_estimate_transform_device(icp_handle *h, const double *d_a_xy, const double *d_b_xy,
                                  size_t n, icp_pose *out, uint32_t *inner_iters);
/* brute-force / grid NN alone (parity tests): d_q n x dim AoS -> d_idx[n] */
int icp_nn_search_device(icp_handle *h, const double *d_q, size_t n, uint32_t *d_idx);
int icp_synchronize(icp_handle *h);

/* One evaluation of weighted_gauss_newton_update (src/lib.rs:218-261) plus the Huber error of the same
 * pose (:75) on device pairs -- the body of one inner iteration of icp_estimate_transform_device, for
 * hosts that drive the inner loop themselves.  kind: 0 = first evaluation on new correspondences,
 * 1 = the evaluation after the first update, 2 = later ones (only selects which earlier evaluation
 * predicts this one's statistics; results never depend on it).  ICP_NONE where the reference returns
 * None. */
int icp_weighted_gn_step_device(icp_handle *h, const double *d_a_xy, const double *d_b_xy, size_t n,
                                const icp_pose *T, int kind, double delta[3], double *huber_err);

/* ================================================================================
 * 5. Sharded evaluation: the inner loop's sums across the GPUs of a node, bit-identical to one GPU
 * ==============================================================================
 * SURVEY.md 8(e).  The N-term sums are folded in a fixed tree of `blocks x 512` threads
 * (icp_reduce_geometry).  Rank r of `world` owns the blocks [blocks r / world, blocks (r+1) / world):
 * the points those blocks fold (icp_shard_geometry: n_local of them; icp_shard_take_device compacts
 * them out of a full array in fold order, icp_shard_put_device is the inverse).  It searches their
 * nearest neighbours (icp_correspond_device on its compact source cloud) and evaluates them with
 *   icp_shard_eval_hist_device        residuals + window histograms of its points   -> *d_hist
 *                                     (+ the running sums of its blocks, kept in the handle: since ABI 4 they
 *                                     carry no 1 / sigma and so need not wait for the statistics)
 *      [host: SUM the icp_shard_histogram_words() u32 at *d_hist over all ranks, in place -- EVERY rank, whatever
 *       its hist call answered (short of ICP_BAD_ARGUMENT): the last four words are status counters, one-hot per
 *       rank {OK, RETRY_REPLICATED, NONE, other}; after the sum every rank reads the same four counts
 *       (icp_shard_eval_status) and takes the same branch, also when a rank-local condition made one rank answer
 *       differently from its peers -- the ranks must never enter different collectives]
 *   icp_shard_eval_compact_device     its candidates around the median / the MAD
 *                                     and its block sums                             -> d_exchange_out
 *      [host: ALL-GATHER icp_shard_exchange_bytes(world) bytes per rank, rank order]
 *   icp_shard_eval_finish_device      exact statistics from all candidates, second stage over all block
 *                                     sums, 3x3 solve                                -> delta, Huber error
 * Two exchanges per evaluation (ABI 3 had a third: icp_shard_eval_accumulate_device between compact and finish).
 * What crosses ranks is integer counts, order statistics candidates and per-block sums placed in block
 * order, so every rank ends with the bits one GPU computes.  The exchange is the host's: RCCL
 * (icp_rust_amd/dist.py drives these calls through torch.distributed), or the peer copies of
 * icp_multi_* below.  ICP_RETRY_REPLICATED (from hist: no prediction of this evaluation's statistics
 * yet / fewer blocks than ranks; from finish: the predicted window missed) means: gather the pairs of
 * all ranks in global order and call icp_weighted_gn_step_device on them instead -- same result, and
 * it provides the prediction.  ICP_RETRY_SHARDED from finish: the window missed, but its (exact,
 * global) counts place a narrower one that will not -- run the three stages again with refined = 1.
 * All calls are asynchronous on the handle's stream except finish. */
int icp_shard_geometry(size_t n_total, int rank, int world, int *block_first, int *block_end, int *blocks,
                       size_t *n_local);
size_t icp_shard_histogram_words(void);
size_t icp_shard_candidates_bytes(void);     /* layout of the exchanged block: the candidates ... */
size_t icp_shard_partials_bytes(int world);  /* ... then the block sums */
size_t icp_shard_exchange_bytes(int world);  /* = the two together */
int icp_shard_take_device(icp_handle *h, const void *d_full, void *d_local, size_t n_total, int rank, int world,
                          size_t elem_bytes);
/* icp_sort_source_device + icp_shard_take_device in one: the fold order of the WHOLE cloud under pose T and this rank's
 * points gathered through it, without a sorted copy of the whole cloud.  d_perm: nullable (n_total words). */
int icp_shard_sort_take_device(icp_handle *h, const double *d_src_full, size_t n_total, const icp_pose *T, int rank, int world,
                               double *d_local, uint32_t *d_perm);
/* icp_prepare_source_device for a rank's points as icp_shard_take_device compacts them out of the fold order: runs of
 * the cell-sorted cloud, whose order the search snapshot keeps (no second sort) */
int icp_shard_prepare_source_device(icp_handle *h, const double *d_src_local, size_t n_local, const icp_pose *T);
int icp_shard_put_device(icp_handle *h, const void *d_local, void *d_full, size_t n_total, int rank, int world,
                         size_t elem_bytes);
int icp_shard_eval_hist_device(icp_handle *h, const double *d_a_xy_local, const double *d_b_xy_local, size_t n_total,
                               int rank, int world, const icp_pose *T, int kind, int refined, uint32_t **d_hist);
int icp_shard_eval_compact_device(icp_handle *h, void *d_exchange_out);
int icp_shard_eval_finish_device(icp_handle *h, const void *d_exchange_all, double delta[3], double *huber_err);
/* the four status counts of the evaluation in flight.  from_device = 0: as finish left them in host memory (valid once
 * finish has returned, no wait); 1: read from the summed buffer behind the stream (a rank whose own hist call was not
 * ICP_OK and which ran no finish).  icp_shard_eval_abort_device: after an evaluation the ranks did not ALL answer with
 * ICP_OK, back to the rest state the next evaluation expects (a rank without a histogram of its own holds its peers'
 * counts after the sum). */
int icp_shard_eval_status(icp_handle *h, uint32_t out[4], int from_device);
int icp_shard_eval_abort_device(icp_handle *h);

/* ---- 5b. The inner loop of a sharded registration in ONE launch per rank (estimate_transform, src/lib.rs:59-84) ----
 * Round 4.  The stage calls above cost ten enqueues and a host wait per evaluation and rank.  Here a rank launches its
 * tree blocks' workgroups ONCE per outer iteration; they keep the rank's pairs on chip, run evaluation after evaluation
 * and exchange the window histograms, the candidates and the block sums with the other ranks THROUGH MEMORY while they
 * run: every rank owns an INBOX (icp_loop_inbox, icp_loop_inbox_bytes() of device memory) that every peer has mapped --
 * plain pointers between ranks of one process (peer access between devices), hipIpc handles between processes
 * (icp_loop_inbox_ipc_handle / icp_loop_ipc_open) -- a producer writes its bytes into every inbox and then a flag word,
 * a consumer polls and reads only its own.  3 x 3 solve, break tests and Transform::new run on the device (every rank
 * computes the same bits); the host sees one result per launch.  Results: the bits of one handle, as with the stage calls.
 *   icp_shard_loop_connect: every rank's inbox as mapped in this process (inboxes[rank] = this handle's own); empties
 *     the own inbox, so the ranks must meet (any barrier of the driver) between connecting and the first launch.
 *   icp_shard_loop_launch_device: from evaluation it0 with the loop's state (inner pose, previous Huber error, updates
 *     applied: src/lib.rs:62-82); launch_no = 1, 2, ... the same on every rank for the same launch; eval_base = the
 *     evaluations earlier launches of this connection served.  ICP_RETRY_SHARDED: nothing launched (no window
 *     prediction for it0 yet, more than 2^23 pairs in total, fewer tree blocks than ranks) -- every rank answers alike, and the
 *     stage calls of section 5 serve that evaluation.
 *   icp_shard_loop_wait: the state after the launch; *evals = the evaluation ROUNDS it ran (an evaluation whose
 *     window missed is repeated once inside the launch with the widest windows and counts twice): what eval_base
 *     advances by; *finished, or *it = the evaluation the stage calls must serve
 *     next (its window missed, or the rotation left the range of the restated sin / cos).  ICP_HIP_ERROR: the launch
 *     gave up waiting for a peer (3 s) -- on EVERY rank: the rank whose wait ran out raises the abort word in all
 *     inboxes, so its peers leave at once and every host takes the same way out (nothing of the launch is used: the
 *     loop's state is the one it was started with; icp_reset_window_predictions, then the stage calls).
 * Ranks that share a device must launch on streams that really run side by side (they wait for each other): more
 * than four of them need GPU_MAX_HW_QUEUES raised before the HIP runtime starts. */
/* What an inbox is made of.  Memory that a PEER DEVICE writes while this device's kernels are polling it has to be
 * coherent between the two at every access, not only at kernel boundaries:
 *   ICP_INBOX_DEVICE  ordinary device memory (hipMalloc).  Right for ranks that share ONE device (virtual ranks of a
 *                     process; processes sharing a GPU through hipIpc): they share its L2.
 *   ICP_INBOX_FINE    fine-grained device memory (hipExtMallocWithFlags): peer access inside a process, hipIpc between
 *                     processes where the runtime exports such an allocation (icp_loop_inbox_ipc_handle fails otherwise).
 *   ICP_INBOX_HOST    pinned host memory in a POSIX shared-memory object: every process of the node maps it
 *                     (icp_loop_inbox_shm_name -> icp_loop_shm_open), registers it with its own device and gets a device
 *                     pointer.  Coherent by construction; the exchange crosses the host link instead of xGMI (a few
 *                     KB per evaluation).  The owner unlinks the name once every peer has opened it (_shm_unlink).
 * Which of them carries the loop between distinct devices is decided AT RUN TIME: icp_loop_transport_probe plays
 * ping-pong over the connected inboxes (every rank at once, bounded waits) and reports whether every token arrived; the
 * driver takes the first transport whose probe passes on every rank (icp_rust_amd/dist.py: connect_loop), else the
 * stage calls of section 5. */
#define ICP_INBOX_DEVICE 0
#define ICP_INBOX_FINE 1
#define ICP_INBOX_HOST 2
size_t icp_loop_inbox_bytes(void);
int icp_loop_inbox(icp_handle *h, int kind, void **d_inbox);
int icp_loop_inbox_ipc_handle(icp_handle *h, unsigned char out[64]);
int icp_loop_ipc_open(int device, const unsigned char handle[64], void **d_ptr);
int icp_loop_ipc_close(void *d_ptr);
int icp_loop_inbox_shm_name(icp_handle *h, char out[64]);
int icp_loop_inbox_shm_unlink(icp_handle *h);
int icp_loop_shm_open(int device, const char *name, void **d_ptr);
int icp_loop_shm_close(void *d_ptr);
int icp_shard_loop_connect(icp_handle *h, int rank, int world, void *const *inboxes);
int icp_loop_transport_probe(icp_handle *h, int rounds, int *ok);
/* every window prediction of the handle forgotten (what a rank does after a one-launch loop gave up: the stage calls
 * that serve from there on must see the same windows on every rank) */
int icp_reset_window_predictions(icp_handle *h);
int icp_shard_loop_launch_device(icp_handle *h, const double *d_a_xy_local, const double *d_b_xy_local, size_t n_total,
                                 unsigned launch_no, unsigned eval_base, int it0, uint32_t applied0, const icp_pose *Ti,
                                 double prev_error, int first_kind, int second_kind);
int icp_shard_loop_wait(icp_handle *h, icp_pose *Ti, double *prev_error, uint32_t *applied, int *it, int *finished,
                        uint32_t *evals);

/* ---- 5c. The PIPELINED sharded registration (round 6; csrc/pipe.hip, csrc/gn_win.hip: k_win_pick_shard) -------------
 * Replaces, for a rank of a sharded registration, the body of the reference's outer loop (src/lib.rs:113-127 / 156-170)
 * in the steady state of a registration -- the inner loop (src/lib.rs:59-84) applies exactly one update -- by the one-GPU
 * pipeline: search -> the two evaluations' first launches over the rank's own points -> their finishing workgroups, which
 * meet the other ranks' through the connected inboxes (section 5b: two exchanges per evaluation, no host, no collective)
 * and leave the next pose on the device for the search already enqueued behind them.  Three launches and one host wait
 * per outer iteration and rank.
 * icp_shard_pipe_run_device: collective -- every rank of the connection calls it at the same outer iteration *it_io with
 * the same pose *T_io (replicated state); it serves nothing until the stage calls or the loop launches have seeded the
 * window predictions of both kinds of evaluation (one outer iteration; a later call on the same handle starts from the
 * previous call's).  d_src_local: the rank's points (icp_shard_take_device out of the fold order,
 * icp_shard_prepare_source_device called on them).  On return *it_io / *T_io
 * are the iteration and pose the caller continues from; inner_iters[k] = 1 for every iteration k served (nullable);
 * d_idx_local receives the correspondences if the call's last iteration (max_iter - 1) was served.  *why = 0: served
 * through max_iter; 1: handed back (a window missed, an inner loop of no or several updates, a NaN: the caller's loop
 * serves iteration *it_io and may call again); 5: a wait for a peer ran out -- every rank reports it, the inboxes carry a
 * raised abort word, and the caller serves the rest through the stage calls.  The bits are those of the other two ways
 * to run a sharded evaluation, and of one GPU.  A rank may own up to 256 tree blocks (world x 2^20 points in total). */
int icp_shard_pipe_run_device(icp_handle *h, const double *d_src_local, size_t n_local, size_t n_total, int rank, int world,
                              icp_pose *T_io, size_t *it_io, size_t max_iter, uint32_t *inner_iters, uint32_t *d_idx_local,
                              int *why);

/* (STATUS: with every rank on ONE device -- "virtual ranks" -- this path runs in the test-suite; between DISTINCT
 * devices it has never run on hardware (no multi-GPU box was available to the build): experimental there.  Mixed lists
 * that repeat only some devices, e.g. {0, 0, 1, 1}, are refused.)
 * The same from ONE host process over the GPUs of a node (SURVEY.md 8(b) sketch: device_ids /
 * n_devices): rank r is a handle on device_ids[r], the target cloud is replicated, the source cloud
 * sharded by reduction-tree block, and the two exchanges are peer reads over xGMI behind flags (no
 * collective library: there is no ICP_RCCL_ERROR).  The result equals icp_estimate's on one GPU bit
 * for bit.  device_ids may repeat a device ("virtual ranks": how the N-rank path is tested on a
 * one-GPU box; ranks on one device share a stream).  icp_multi_counters: out[0] evaluations that ran
 * sharded, out[1] evaluations that fell back to gathered pairs. */
typedef struct icp_multi icp_multi;
int icp_create_multi(icp_multi **out, int dim, const double *dst, size_t m, const int *device_ids, int n_devices);
int icp_multi_estimate(icp_multi *M, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                       icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters);
/* EXTENSION (section 6 across the ranks; BASELINE configs[4] on several GPUs): every rank appends the same k points,
 * moved by T (NULL: as they are), to its replica of the target cloud and rebuilds its search grid; afterwards the
 * object answers like a fresh icp_create_multi on the concatenated cloud, in the sense of section 6 (correspondences
 * always; pose bits for source clouds that keep the caller's fold order). */
int icp_multi_append_targets(icp_multi *M, const double *pts, size_t k, const icp_pose *T);
size_t icp_multi_target_count(const icp_multi *M);
void icp_destroy_multi(icp_multi *M);


/* The N-term sums (jtj, jtr, Huber error) are added in a fixed, run-to-run
 * deterministic tree; this reports its geometry for n points so a checker can
 * reproduce the exact association order (DESIGN.md "GN reduction order"). */
void icp_reduce_geometry(size_t n, int *blocks, int *threads);
/* ... over the source points in FOLD ORDER.  The reference folds over the caller's order
 * (src/lib.rs:240-255, a left fold); the sum is the same up to rounding, so any fixed order meets the
 * 1e-5 pose bar.  When icp_estimate[_device] takes a cell-sorted snapshot of the source cloud (grid
 * engine, MORE THAN 65 536 source points -- the largest cloud searched with four lanes per query; the threshold is a
 * constant of the library) the fold order IS the snapshot order -- ascending
 * (target-grid cell of init * src[i], i), a stable sort, hence a pure function of the inputs AND OF THE HANDLE'S GRID
 * (box and cell size: what icp_create chose for the target cloud, kept by incremental appends, section 6) -- so that
 * the search can store its pairs with full-line writes and nothing is ever scattered back; otherwise (smaller clouds,
 * the sweep engine, the stage calls) it is the caller's order.
 * icp_last_fold_order reports it for the last estimate call on `h` (host buffers of n words, either may be
 * NULL): perm[k] = caller's index of the k-th folded point, cell[k] = its sort key (all 0 for the identity).
 * A checker reproduces the device sums by folding the pairs of src[perm[0]], src[perm[1]], ... in the
 * tree of icp_reduce_geometry. */
int icp_last_fold_order(icp_handle *h, size_t n, uint32_t *perm, uint32_t *cell);
/* The fold order of an estimate call that starts at pose T, applied (device buffers): d_sorted[k] = d_src[perm[k]],
 * d_perm nullable.  For hosts that drive the stage calls of sections 4 and 5 themselves and want the bits of
 * icp_estimate_device: sort first, then treat the sorted cloud as the source (sorting it again is the identity). */
int icp_sort_source_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, double *d_sorted,
                           uint32_t *d_perm);




/* The reference builds a new Icp per frame (examples/scan2d.rs:87, scan3d.rs:130), so icp_destroy
 * keeps the device buffers, streams and pinned memory of up to two handles per process for the
 * next icp_create on the same device (a create then costs its kernels, not its allocations).
 * icp_trim_pool releases them. */
void icp_trim_pool(void);

/* ================================================================================
 * 6. EXTENSION (not in the reference): a target cloud that grows -- scan-to-map
 * ==============================================================================
 * BASELINE.json configs[4] registers each scan against a map that the
 * registered scans are appended to.  The reference has no such thing: its Icp borrows a fixed
 * `dst` (src/lib.rs:97-102, 139-144).  What the reference does define is the registration of a
 * scan against ANY target cloud, so a map handle is an ordinary handle whose target cloud can
 * be extended; after an append every CORRESPONDENCE is that of a fresh icp_create on the
 * concatenated cloud (target indices = position in the concatenation), and so is every pose, bit for bit, as long as
 * the source cloud keeps the caller's fold order (up to 65 536 points, section 9a).  Larger source clouds fold
 * their sums in the order of the handle's grid cells; an incrementally appended handle keeps the grid of its last full
 * build where a fresh handle derives a new one, so their poses agree to the rounding of a re-ordered sum (~1e-12
 * relative; the bar is 1e-5) -- each equals the oracle evaluated in ITS fold order (icp_last_fold_order) bit for bit.  Point-to-plane
 * residuals, also named by configs[4], have no definition in the reference (no normals
 * anywhere in src/): section 7 builds them as a second labelled extension.
 *
 * icp_append_targets[_device]: append k points (AoS, the handle's dim) to the target cloud;
 * with T != NULL the points are first moved by T exactly as Transform::transform does
 * (transform.rs:22-24: x' = (r00 x + r01 y) + tx, y' = (r10 x + r11 y) + ty, z kept; no FMA),
 * i.e. "append the scan at its registered pose".  A handle made by icp_create_device stops
 * borrowing the caller's buffer at its first append (the cloud moves into storage the handle
 * owns, grown geometrically).  The search structures are rebuilt on the device.
 * icp_reserve_targets sizes that storage ahead of time; icp_target_count reports m. */
int icp_append_targets(icp_handle *h, const double *pts, size_t k, const icp_pose *T);
int icp_append_targets_device(icp_handle *h, const double *d_pts, size_t k, const icp_pose *T);
int icp_reserve_targets(icp_handle *h, size_t capacity);
size_t icp_target_count(const icp_handle *h);
/* copy target points [first, first + k) back to the host (AoS), e.g. to save the map */
int icp_read_targets(icp_handle *h, size_t first, size_t k, double *out);

/* ================================================================================
 * 7. EXTENSION (not in the reference): point-to-plane residuals
 * ==============================================================================
 * The second thing BASELINE.json configs[4] names.  tier4/icp_rust is point-to-point only (no normal
 * anywhere in src/; src/lib.rs:218-261), so there is no reference behaviour to match and no parity
 * claim: the definition lives in icp_rust_amd/csrc/p2plane.hip, its CPU restatement (the checker of
 * tests/test_p2plane.py) in oracle/icp_oracle.c (orc_p2pl_*).  Kept from the reference: the exact 3-D
 * nearest neighbour, the SE(2) pose on xy with z carried through, the Huber / MAD Gauss-Newton loop
 * with its constants and break tests, the 3x3 solve, Transform::new.  3-D handles only.
 *
 * icp_compute_target_normals: unit normal of every target = smallest-eigenvalue eigenvector of the
 * covariance of its k nearest targets (3 <= k <= 16, itself included), searched through the handle's
 * grid; after an append call it again, or icp_update_target_normals: only the appended targets get a
 * normal (from the cloud as it is now), the older ones keep theirs ("normals at insertion time": what a
 * map that grows frame by frame uses; same k as before).  icp_estimate_point_to_plane*: Icp3d::estimate
 * with the scalar residual n_q . (T p - q) in place of the two-row point-to-point residual.  The pairs are
 * folded in the caller's order (no snapshot order) in the tree of icp_reduce_geometry(n); the pose is bit-equal
 * to the CPU restatement folded that way (tests/test_gpu_plane_parity.py).  An empty source cloud (n == 0)
 * returns *init with every inner count 0, as Icp3d::estimate does on an empty scan. */
int icp_compute_target_normals(icp_handle *h, int k);
int icp_update_target_normals(icp_handle *h, int k);
int icp_read_target_normals(icp_handle *h, size_t first, size_t count, double *out_xyz);
int icp_estimate_point_to_plane(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                                size_t max_iter, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters);
int icp_estimate_point_to_plane_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                       size_t max_iter, icp_pose *out, uint32_t *d_last_idx,
                                       uint32_t *inner_iters);
/* ... across the ranks of an icp_multi (round 4; BASELINE configs[4] on several GPUs): the normals belong to the replicated
 * target cloud, so every rank computes / updates the same ones; a registration shards the SEARCH (contiguous slices of
 * the source cloud), every rank receives every slice's indices and runs the same inner loop on the whole cloud
 * (SURVEY.md 8(e) option 1).  Result: one handle's icp_estimate_point_to_plane, bit for bit. */
int icp_multi_compute_target_normals(icp_multi *M, int k);
int icp_multi_update_target_normals(icp_multi *M, int k);
int icp_multi_estimate_point_to_plane(icp_multi *M, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                                      icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters);

/* ================================================================================
 * 8. EXTENSION (not in the reference): many small registrations in one call
 * ==============================================================================
 * Loop-closure candidates, K initial poses of one scan against one map, a recorded sequence against fixed keyframes:
 * independent registrations of small clouds.  One call runs every item whose clouds fit one workgroup (n <= 1024
 * source points, 1 <= m <= 2048 targets, 1 <= max_iter <= 1024) as one workgroup of ONE launch per workgroup size
 * (at most three launches), the other items -- and those a workgroup hands back -- through icp_create_device +
 * icp_estimate_device on the item's ranges, one after another.  Item i's out[i], status[i], indices and inner counts
 * are what icp_create(dim, dst + dst_first, m) + icp_estimate(src + src_first, n, &init, max_iter) return on a fresh
 * handle, bit for bit.  out[i] is meaningful when status[i] == ICP_OK; per-item statuses are ICP_OK, ICP_EMPTY_DST and
 * ICP_NAN_INPUT.  The call's own return value is ICP_OK or a whole-call failure: ICP_BAD_ARGUMENT (a bad dim, an item
 * range outside its array, NULL where a pointer is required -- all checked before the device is touched),
 * ICP_NO_DEVICE, ICP_HIP_ERROR, ICP_OUT_OF_MEMORY.  count == 0 is a successful no-op.
 * Ranges may overlap (K hypotheses of one scan against one map share one src range and one dst range: no copies).
 * last_idx (nullable): each item's final correspondences (indices into its own dst range), concatenated in item
 * order, sum(n) entries; inner_iters (nullable): count x max_iter, item-major.
 * An icp_batch keeps a stream, pinned result buffers and the device item lists between calls; one call in flight per
 * icp_batch (as for handles).  icp_batch_create does not touch the device (device < 0: the current one, resolved by
 * the first call that computes); every argument of a call is checked before the device is.  The _device entry reads src / dst from device memory that must be complete when the
 * call is made, and writes d_last_idx on the device; out / status / inner_iters are host memory in both entries. */
typedef struct icp_batch icp_batch;
typedef struct icp_batch_item {
  uint64_t src_first, n; /* source points [src_first, src_first + n) of the call's src array */
  uint64_t dst_first, m; /* target points [dst_first, dst_first + m) of the call's dst array */
  icp_pose init;
} icp_batch_item;
int icp_batch_create(icp_batch **out, int dim, int device);
void icp_batch_destroy(icp_batch *b);
int icp_batch_estimate(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                       const icp_batch_item *items, size_t count, size_t max_iter, icp_pose *out, int *status,
                       uint32_t *last_idx, uint32_t *inner_iters);
int icp_batch_estimate_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                              size_t dst_points, const icp_batch_item *items, size_t count, size_t max_iter,
                              icp_pose *out, int *status, uint32_t *d_last_idx, uint32_t *inner_iters);

/* ================================================================================
 * 9. EXTENSION (not in the reference): the quality of a pose
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  What a caller bases an accept / reject or a
 * best-hypothesis decision on, and the information matrix a pose-graph edge needs: scored on the device at the pose
 * given, with the handle's own exact correspondence search.  DESIGN.md section 9d restates the definition.
 *
 * For a handle with targets dst (m points), a source cloud src (n points, caller order), a pose T and max_dist r
 * (r >= 0, or +inf), for every source point i:
 *   qx = (r00 px + r01 py) + tx, qy = (r10 px + r11 py) + ty, qz = pz     (transform_xy, no FMA)
 *   j  = the handle's exact nearest neighbour of q (d2 = ((dx dx + dy dy) + dz dz), ties -> lowest index), b = dst[j]
 *   ex = qx - bx, ey = qy - by, e2 = ex ex + ey ey, h = rho(e2)          (huber.rs, k = ICP_HUBER_K)
 *   inlier = d2 <= r * r (r * r in f64; d2 in the handle's dimension; a NaN d2 is never an inlier)
 *   inlier terms: 1, d2, qx, qy, qx qx + qy qy; a point that is not an inlier adds +0.0 to each sum.
 * fold(v), over the n values in caller order: n == 0 -> +0.0; n == 1 -> v[0]; otherwise, while more than one value is
 * left: pad with +0.0 to a multiple of 256, run g[i] += g[i + s] for s = 128, 64, ..., 1 in each group of 256, and keep
 * each group's g[0].  The order is fixed: it does not depend on how the work is launched.
 *   inliers        the count (exact)                  fitness      inliers / n (0 when n == 0)
 *   inlier_sum_d2  fold(d2 terms)                     inlier_rmse  sqrt(inlier_sum_d2 / inliers) (0 without inliers)
 *   error          fold(e2)                           huber_error  fold(h)  (icp::error / huber_error, src/lib.rs:38-50,
 *                                                                           of the pairs (xy(T src), xy(dst[idx])))
 *   information    row-major [[c, 0, -Sy], [0, c, Sx], [-Sy, Sx, Srr]], c = (double)inliers, Sx / Sy / Srr the folds
 *                  of the qx / qy / qx qx + qy qy terms: the jtj that gauss_newton_update (src/lib.rs:191-216) forms at
 *                  identity on the inlier pairs -- the SE(2) Hessian in (x, y, theta).
 * Statuses: ICP_BAD_ARGUMENT (r NaN or negative, a required pointer NULL; checked before any device use); n == 0 ->
 * ICP_OK and zeros; ICP_EMPTY_DST (no targets); ICP_NAN_INPUT (some e2 is NaN, the estimator's rule).  *out is the
 * result when the call returns ICP_OK; otherwise it holds n and zeros.
 *
 * icp_evaluate[_device]: any handle (a map handle after appends, either search engine); idx / d_idx (nullable): the n
 * correspondences at T, caller order.  The handle's registration state is not touched: an estimate after an evaluate
 * gives the bits it gives without one.
 * icp_batch_evaluate[_device]: item i (its `init` is the pose to evaluate) gets the status and quality of
 * icp_create(dst range) + icp_evaluate(src range, init), bit for bit; items of 1 <= n <= 1024 and 1 <= m <= 2048 run as
 * one workgroup each of one launch, the others one by one.  Argument checks and whole-call errors as
 * icp_batch_estimate's, plus r; ranges may overlap; out and status are host memory in both entries. */
typedef struct icp_quality {
  uint64_t n;              /* source points                                   */
  uint64_t inliers;        /* points with d2 <= max_dist^2                     */
  double fitness;          /* inliers / n                                      */
  double inlier_rmse;      /* sqrt(inlier_sum_d2 / inliers)                    */
  double inlier_sum_d2;    /* fold of the inliers' squared distances           */
  double error;            /* fold of e2 over all points                       */
  double huber_error;      /* fold of rho(e2) over all points                  */
  double information[9];   /* row-major SE(2) information of the inlier pairs  */
} icp_quality;
int icp_evaluate(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist, icp_quality *out,
                 uint32_t *idx);
int icp_evaluate_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, double max_dist,
                        icp_quality *out, uint32_t *d_idx);
int icp_batch_evaluate(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                       const icp_batch_item *items, size_t count, double max_dist, icp_quality *out, int *status);
int icp_batch_evaluate_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                              size_t dst_points, const icp_batch_item *items, size_t count, double max_dist,
                              icp_quality *out, int *status);

/* ================================================================================
 * 10. EXTENSION (not in the reference): registration with a maximum correspondence distance
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  icp_estimate lets every source point pull on
 * the pose; only the Huber / MAD weights stand between an object the target does not hold and the result.  Here the
 * estimator sees the INLIERS of each outer iteration only -- section 9's inlier rule, so a caller registers on the
 * pairs it scores a pose by.  The reference has no gate: no parity claim; DESIGN.md section 9e restates the definition.
 *
 * icp_estimate_gated[_device] runs the outer loop of Icp2d / Icp3d::estimate (src/lib.rs:105-130, 148-173).  For
 * outer iteration `it` at pose T, for every source point i:
 *   q, j, b = dst[j] and d2 exactly as section 9 defines them (transform_xy without FMA, the handle's exact nearest
 *   neighbour, d2 = ((dx dx + dy dy) + dz dz) in the handle's dimension);
 *   inlier = d2 <= r * r (r = max_dist, r * r in f64; a NaN d2 is never an inlier).
 * The pairs (xy(q), xy(b)) of the inliers, IN FOLD ORDER WITH THE OTHERS REMOVED AND THE ORDER KEPT, go to
 * estimate_transform (src/lib.rs:59-84); the update is composed as src/lib.rs:127, 170 do.  The fold order over all n
 * points is the one icp_estimate_device would use (the caller's order up to 65 536 points and on the sweep engine, the
 * snapshot order above that); icp_last_fold_order reports it for a gated call too.  The sums of an evaluation are
 * folded in the tree of icp_reduce_geometry(number of inliers).
 *   fewer than two inliers: the iteration applies no update (check_input_size, src/lib.rs:186-189), inner_iters[it] = 0;
 *   inliers[it] (nullable, max_iter words): the number of inliers of that iteration;
 *   last_idx / d_last_idx (nullable): the correspondences of ALL n points at the last iteration, caller order, as
 *   icp_estimate returns them;
 *   the fixed-point exit of icp_estimate applies unchanged: the iterations it skips report inner_iters = 0 and the
 *   inlier count of the iteration that found the fixed point (same pose, hence the same count).
 * Statuses: ICP_BAD_ARGUMENT (max_dist NaN or negative, a required pointer NULL: checked before any device use; +inf
 * and 0.0 are valid bounds); ICP_EMPTY_DST (no targets); ICP_NAN_INPUT (an inlier pair with a NaN residual); n == 0
 * and max_iter == 0 behave as in icp_estimate.
 * Consequence: for inputs without a NaN d2, max_dist = +inf returns the pose, the indices and the inner counts of
 * icp_estimate[_device], bit for bit, at every size and on both engines (every evaluation pipeline returns the same
 * bits for the same pairs in the same order).  With a finite bound a source point with a NaN coordinate is dropped
 * like any other outlier.  A call takes the general path at every size: clouds of the one-launch registration
 * (section 2) are served by several launches per iteration here.
 *
 * icp_gate_pairs_device: the gate alone, in the style of section 4 (device buffers; synchronises the stream).  From
 * the source cloud, a pose and the indices of a search at that pose (icp_correspond_device, icp_nn_search_device) it
 * writes the inliers' pairs densely, in the order of d_src: d_a_xy[k] = xy(T src[i_k]), d_b_xy[k] = xy(dst[idx[i_k]])
 * for the k-th inlier i_k; d_kept[k] = i_k (nullable); *kept = their number.  d_a_xy, d_b_xy (and d_kept) hold n
 * entries. */
int icp_estimate_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                       double max_dist, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers);
int icp_estimate_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init, size_t max_iter,
                              double max_dist, icp_pose *out, uint32_t *d_last_idx, uint32_t *inner_iters,
                              uint32_t *inliers);
int icp_gate_pairs_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                          double max_dist, double *d_a_xy, double *d_b_xy, uint32_t *d_kept, size_t *kept);

/* ================================================================================
 * 11. EXTENSION (not in the reference): a target cloud that lets go -- the sliding-window map
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  The counterpart of icp_append_targets
 * (section 6): a map that a scan-to-map loop feeds grows without bound; icp_crop_targets keeps the targets inside a disc
 * of the xy plane and removes the others, on the device, normals included.  It keeps the contract section 6 gives an
 * append: afterwards the handle answers like a fresh icp_create on the cloud it now holds.  The reference has no such
 * thing: no parity claim; DESIGN.md section 9f restates the definition.
 *
 * The keep rule.  For centre (cx, cy) = center_xy and radius r (r >= 0, or +inf), target i with coordinates (x, y[, z]):
 *   dx = x - cx, dy = y - cy, d2 = dx dx + dy dy                        (no FMA)
 *   kept = d2 <= r * r (r * r in f64; a NaN d2 is never kept)
 * The same xy disc applies to 2-D and 3-D handles (the pose is SE(2), z is never estimated: a caller crops around the
 * translation of its pose).  +inf and 0.0 are valid radii.
 * After a crop of a cloud of m_before targets:
 *   the kept targets stay in their original relative order; target index = position in the kept sequence;
 *   icp_read_targets returns them bit for bit;
 *   new_index (nullable, host, m_before words): new_index[i] = the new index of old target i, 0xffffffff if removed;
 *   *removed (nullable) = the number of targets removed;
 *   every CORRESPONDENCE is that of a fresh icp_create on the kept cloud, and so is every pose, bit for bit, for source
 *   clouds that keep the caller's fold order (up to 65 536 points); larger source clouds fall under the clause of
 *   section 6: a cropped handle may keep the grid of its last full build, and each handle equals the oracle evaluated in
 *   ITS fold order (icp_last_fold_order) bit for bit.
 * Normals (section 7): kept targets keep their normals, compacted alongside the points; the number of targets that have
 * one becomes the number of kept targets among those that had one.  A map whose normals were complete stays usable
 * for icp_estimate_point_to_plane* without recomputation; after an append without an update,
 * icp_update_target_normals still gives normals to exactly the kept targets that have none.
 * Edges.  Nothing removed: nothing about the handle changes (it keeps borrowing a caller's device buffer; no counter
 * moves).  Otherwise a handle made by icp_create_device stops borrowing, as at its first append; the caller's buffer is
 * never written.  Everything removed: the handle behaves like one created on an empty cloud (ICP_EMPTY_DST from
 * icp_estimate; a later append works).
 * Statuses: ICP_BAD_ARGUMENT (h or center_xy NULL, a NaN centre, a NaN or negative radius: checked before any device
 * use); ICP_NO_DEVICE, ICP_HIP_ERROR, ICP_OUT_OF_MEMORY as elsewhere.  On any failure the handle is what it was before
 * the call (the cloud is compacted out of place and the buffers are swapped on success).
 * icp_multi_crop_targets: every rank crops its replica, icp_multi_target_count follows; a rank that fails leaves the
 * replicas different and the object unusable, as for icp_multi_append_targets. */
int icp_crop_targets(icp_handle *h, const double center_xy[2], double radius, uint32_t *new_index, size_t *removed);
int icp_multi_crop_targets(icp_multi *M, const double center_xy[2], double radius, size_t *removed);

/* ================================================================================
 * 12. EXTENSION (not in the reference): point-to-plane registration with a maximum correspondence distance
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 10's gate for section 7's estimator:
 * the point-to-plane inner loop sees the INLIERS of each outer iteration only.  A frame registered against a growing
 * map always holds surface the map does not; without the gate every such point pulls on the pose through the plane of
 * whatever target happens to be nearest.  No parity claim; DESIGN.md section 9g restates the definition.
 *
 * icp_estimate_point_to_plane_gated[_device] runs the outer loop of icp_estimate_point_to_plane_device.  For outer
 * iteration `it` at pose T: the exact 3-D search at T; then for every source point i with match j
 *   qx = (r00 px + r01 py) + tx, qy = (r10 px + r11 py) + ty, ex = qx - dst[j].x, ey = qy - dst[j].y,
 *   dz = pz - dst[j].z, d2 = ((ex ex + ey ey) + dz dz)                  (no FMA: d2 exactly as sections 9 / 10 define it)
 *   inlier = d2 <= max_dist * max_dist (in f64; a NaN d2 is never an inlier);
 * section 7's inner loop on the pairs of the inliers, IN THE CALLER'S ORDER WITH THE OTHERS REMOVED (the point-to-plane
 * path has no snapshot order); T = dT * T.  The sums of an evaluation are folded in the tree of
 * icp_reduce_geometry(number of inliers).
 *   fewer than two inliers: the iteration applies no update (as n < 2 does in section 7), inner_iters[it] = 0;
 *   inliers[it] (nullable, max_iter words): the number of inliers of iteration `it`;
 *   last_idx / d_last_idx (nullable): the correspondences of ALL n points at the last iteration, caller order;
 *   there is no fixed-point exit, as icp_estimate_point_to_plane has none: every iteration runs.
 * Statuses, decided in this order: ICP_BAD_ARGUMENT (a required pointer NULL, max_dist NaN or negative, n >= 2^32 - 1:
 * before any device use and before the handle is read; +inf and 0.0 are valid bounds); ICP_NO_DEVICE; then the handle:
 * ICP_BAD_ARGUMENT (not a 3-D handle; normals not current), ICP_EMPTY_DST (no targets, when a search would run);
 * ICP_NAN_INPUT (an inlier pair with a NaN residual); n == 0 and max_iter == 0 behave as in section 7.
 * Consequence: for inputs without a NaN d2, max_dist = +inf returns the pose, the indices and the inner counts of
 * icp_estimate_point_to_plane[_device], bit for bit (same pairs, same order, same n: the same reduction geometry), and
 * inliers[it] == n.
 *
 * icp_gate_plane_pairs_device: the gate alone, in the style of section 4 (device buffers; synchronises the stream).
 * From the source cloud, a pose and the indices of a search at that pose it writes, for the k-th inlier i_k in the order
 * of d_src, the eight doubles the inner loop reads: d_pairs[8 k ..] = ax, ay (xy(T src[i_k])), qx, qy (xy of its match),
 * dz (src z - match z), nx, ny, nz (the match's normal); d_kept[k] = i_k (nullable); *kept = their number.  d_pairs
 * holds 8 n doubles, d_kept n words.  n == 0: ICP_OK, *kept = 0, nothing else is looked at.
 *
 * icp_multi_estimate_point_to_plane_gated: icp_multi_estimate_point_to_plane with the gate -- the search is sharded,
 * every rank gates the whole cloud and runs the inner loop on its survivors; the ranks must agree on pose, applied
 * count and kept count.  Result: one handle's icp_estimate_point_to_plane_gated, bit for bit. */
int icp_estimate_point_to_plane_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                                      double max_dist, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters,
                                      uint32_t *inliers);
int icp_estimate_point_to_plane_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                             size_t max_iter, double max_dist, icp_pose *out, uint32_t *d_last_idx,
                                             uint32_t *inner_iters, uint32_t *inliers);
int icp_gate_plane_pairs_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                                double max_dist, double *d_pairs, uint32_t *d_kept, size_t *kept);
int icp_multi_estimate_point_to_plane_gated(icp_multi *M, const double *src, size_t n, const icp_pose *init,
                                            size_t max_iter, double max_dist, icp_pose *out, uint32_t *last_idx,
                                            uint32_t *inner_iters, uint32_t *inliers);

/* ================================================================================
 * 13. EXTENSION (not in the reference): the quality of a pose under the point-to-plane residual
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 9 scores a pose by the point-to-point
 * residual: its information matrix has the translation block c * I whatever the scene looks like.  A pose registered
 * with plane residuals (sections 7, 12) is observed only along the normals of the surfaces it was matched to -- in a
 * corridor it slides freely along the axis -- and a filter or a pose graph needs the information that residual
 * actually gives.  This section scores a pose for a 3-D handle with current normals: the fitness, the plane-residual
 * RMSE and the unweighted jtj of section 7's accumulation at the pose, rank-deficient exactly where the scene is.
 * The reference has no such thing: no parity claim; DESIGN.md section 9h restates the definition.
 *
 * For a handle with targets dst (m points) and their normals nrm, a source cloud src (n points, caller order), a pose
 * T and max_dist r (r >= 0, or +inf), for every source point p (no FMA anywhere):
 *   qx = (r00 px + r01 py) + tx, qy = (r10 px + r11 py) + ty               (transform_xy)
 *   j  = the handle's exact 3-D nearest neighbour of (qx, qy, pz); b = dst[j], (nx, ny, nz) = nrm[j]
 *   ex = qx - bx, ey = qy - by, dz = pz - bz
 *   d2 = ((ex ex + ey ey) + dz dz)                                         (section 9's d2)
 *   inlier = d2 <= r * r (r * r in f64; a NaN d2 is never an inlier)
 *   rp = (nx ex + ny ey) + nz dz                (section 7's plane residual at the identity inner pose)
 *   p2 = rp rp
 *   c  = (nx * (-qy)) + (ny * qx)               (the third entry of section 7's Jacobian row (nx, ny, c) at identity)
 * Ten sums, each by section 9's fold over the n values in caller order (n == 1: the one value); a point that is not an
 * inlier adds +0.0 to the inlier-only sums:
 *   S_d2 = fold(inlier ? d2)     S_p2 = fold(inlier ? p2)     E = fold(p2)     H = fold(rho(p2))  (huber.rs)
 *   Ixx = fold(inlier ? nx nx)   Ixy = fold(inlier ? nx ny)   Iyy = fold(inlier ? ny ny)
 *   Ixt = fold(inlier ? nx c)    Iyt = fold(inlier ? ny c)    Itt = fold(inlier ? c c)
 *   inliers        the count (exact)                  fitness      inliers / n
 *   inlier_sum_d2  S_d2                               inlier_rmse  sqrt(S_d2 / inliers) (0 without inliers): the bits
 *                                                                  icp_evaluate gives at the same T and r
 *   plane_sum_r2   S_p2                               plane_rmse   sqrt(S_p2 / inliers) (0 without inliers)
 *   error          E                                  huber_error  H (what section 7's evaluation reports as its error)
 *   information    row-major [[Ixx, Ixy, Ixt], [Ixy, Iyy, Iyt], [Ixt, Iyt, Itt]]: the SE(2) Hessian in (x, y, theta) of
 *                  the plane residual on the inlier pairs, unweighted
 *   translation_eig  the eigenvalues lmin, lmax of [[Ixx, Ixy], [Ixy, Iyy]], on the host with + - * sqrt only:
 *                  h = (Ixx + Iyy) * 0.5, g = (Ixx - Iyy) * 0.5, s = sqrt(g g + Ixy Ixy), lmin = h - s, lmax = h + s.
 *                  Only the translation block gets eigenvalues: its units are consistent; the 3 x 3 matrix mixes metres
 *                  and radians and is left to the caller.
 * Statuses, decided in this order: ICP_BAD_ARGUMENT (h, T or out NULL; src NULL with n > 0; r NaN or negative;
 * n >= 2^32 - 1: before any device use and before the handle is read); n == 0 -> ICP_OK and zeros; ICP_NO_DEVICE; then
 * the handle: ICP_BAD_ARGUMENT (not a 3-D handle; normals not current), ICP_EMPTY_DST (no targets); ICP_NAN_INPUT (some
 * p2 is NaN).  *out is the result when the call returns ICP_OK; otherwise it holds n and zeros.
 * idx / d_idx (nullable): the n correspondences at T, caller order.  The handle's registration state is not touched:
 * an estimate after an evaluation gives the bits it gives without one. */
typedef struct icp_plane_quality {
  uint64_t n;                 /* source points                                          */
  uint64_t inliers;           /* points with d2 <= max_dist^2                           */
  double fitness;             /* inliers / n                                            */
  double inlier_rmse;         /* sqrt(inlier_sum_d2 / inliers): section 9's             */
  double inlier_sum_d2;       /* fold of the inliers' squared distances                 */
  double plane_rmse;          /* sqrt(plane_sum_r2 / inliers), 0 without inliers        */
  double plane_sum_r2;        /* fold of the inliers' squared plane residuals           */
  double error;               /* fold of p2 over all points                             */
  double huber_error;         /* fold of rho(p2) over all points                        */
  double information[9];      /* row-major SE(2) information of the inlier pairs        */
  double translation_eig[2];  /* lmin, lmax of the 2 x 2 translation block              */
} icp_plane_quality;
int icp_evaluate_point_to_plane(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                                icp_plane_quality *out, uint32_t *idx);
int icp_evaluate_point_to_plane_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, double max_dist,
                                       icp_plane_quality *out, uint32_t *d_idx);

/* ================================================================================
 * 14. EXTENSION (not in the reference): point-to-line registration for 2-D handles
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  The planar counterpart of sections 7 and 12
 * ("PLICP"): a 2-D scan and its target sample the same walls at different places, so nearest-neighbour pairs differ
 * ALONG the wall by up to the sample spacing; the line residual does not see that, the point residual does.  Lifting
 * a scan to z = 0 and calling section 7 does not give it: the covariance of coplanar neighbours has its smallest
 * eigenvector along z, every normal is (0, 0, 1) and every residual nz dz = 0.  Every entry is for dim == 2 handles
 * only (ICP_BAD_ARGUMENT on a 3-D handle); sections 7, 12 and 13 keep refusing a 2-D handle.  The reference has no
 * such thing: no parity claim; DESIGN.md section 9i restates the definition.
 *
 * The line normal of a target q (section 7's definition with the third coordinate removed; no FMA anywhere):
 *   neighbourhood  the k targets nearest to q in the xy plane, q itself included, ordered by (d2, index) with
 *                  d2 = dx dx + dy dy; 3 <= k <= 16, k clamped to the number of targets
 *   mean, a        mean[d] = (sum over the neighbours in that order) / count; a[r][s] += e[r] e[s] with e = p - mean, in
 *                  that order: the 2 x 2 covariance (unnormalised)
 *   eigenvector    one Jacobi rotation of the pair (0, 1) -- theta = (a11 - a00) / (2 a01),
 *                  t = sign(theta) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c; A <- A J,
 *                  A <- J^T A, V <- V J -- skipped when a01 == 0; the column of the smaller diagonal, a tie: column 0
 *   normalisation  by sqrt(n0 n0 + n1 n1); sign: the first non-zero of (n_y, n_x) is positive
 *   degenerate     fewer than 3 neighbours, or zero length: the zero vector
 * icp_compute_target_line_normals computes all of them through the target grid; icp_update_target_line_normals gives
 * one to the targets appended since (from the cloud as it is now; the older targets keep theirs bit for bit; the same
 * k as before, ICP_BAD_ARGUMENT otherwise); icp_read_target_line_normals copies count x 2 doubles out.  As in
 * section 7 an append leaves the normals stale until an update, and icp_crop_targets (section 11) carries the kept
 * targets' normals along.  Statuses: ICP_BAD_ARGUMENT (h NULL, k outside [3, 16]); ICP_NO_DEVICE; then the handle:
 * ICP_BAD_ARGUMENT (not a 2-D handle; non-finite targets; read: normals not current or the range outside the cloud),
 * ICP_EMPTY_DST (no targets).
 *
 * icp_estimate_point_to_line[_device]: Icp2d::estimate (src/lib.rs:105-130) with the residual n_q . (T p - q), ONE
 * scalar per pair, where q is the handle's exact 2-D nearest neighbour of T p and n_q its line normal.  Weights
 * (sigma = 1.4826 MAD(r), Huber 1.345), Jacobian row n^T [R | R (-a_y, a_x)^T], Huber error, the inner loop and its
 * break tests are section 7's, applied to pairs with dz = 0 and nz = 0.  inner_iters / last_idx as there.
 * icp_estimate_point_to_line_gated[_device]: section 12's gate around it -- the inner loop of outer iteration `it`
 * sees the pairs with d2 = ex ex + ey ey <= max_dist * max_dist only (ex = qx - dst[j].x, ey = qy - dst[j].y at the
 * iteration's pose; a NaN d2 is never an inlier), in the caller's order; inliers[it] (nullable) their number.
 * Statuses, decided in this order: ICP_BAD_ARGUMENT (a required pointer NULL, n >= 2^32 - 1, gated: max_dist NaN or
 * negative; +inf and 0.0 are valid bounds); ICP_NO_DEVICE; then the handle: ICP_BAD_ARGUMENT (not a 2-D handle),
 * ICP_EMPTY_DST (no targets, only when a search would run: n > 0 and max_iter > 0; otherwise *out = *init),
 * ICP_BAD_ARGUMENT (normals absent or stale); ICP_NAN_INPUT (a pair with a NaN residual).  Fewer than two pairs: the
 * iteration applies no update.  Consequence: for inputs without a NaN d2, max_dist = +inf returns the pose, the
 * indices and the inner counts of the ungated call, bit for bit, and inliers[it] == n. */
int icp_compute_target_line_normals(icp_handle *h, int k);
int icp_update_target_line_normals(icp_handle *h, int k);
int icp_read_target_line_normals(icp_handle *h, size_t first, size_t count, double *out_xy);
int icp_estimate_point_to_line(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                               icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters);
int icp_estimate_point_to_line_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init, size_t max_iter,
                                      icp_pose *out, uint32_t *d_last_idx, uint32_t *inner_iters);
int icp_estimate_point_to_line_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                                     double max_dist, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters,
                                     uint32_t *inliers);
int icp_estimate_point_to_line_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                            size_t max_iter, double max_dist, icp_pose *out, uint32_t *d_last_idx,
                                            uint32_t *inner_iters, uint32_t *inliers);

/* ================================================================================
 * 15. EXTENSION (not in the reference): many small point-to-line registrations in one call
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 8's call with section 14's residual,
 * for 2-D batches: K pose hypotheses of one scan against one map, loop-closure candidates, a log replayed offline.
 * Item i's out[i], status[i], indices and inner counts are what icp_create(2, dst + 2 dst_first, m) +
 * icp_compute_target_line_normals(k) + icp_estimate_point_to_line(src + 2 src_first, n, &init, max_iter) return on a
 * fresh handle, bit for bit (the ungated call; a first failing step's status is the item's).  Every item with
 * 1 <= n <= 1024, 1 <= m <= 2048 and 1 <= max_iter <= 1024 runs as ONE workgroup that computes the item's line normals
 * and the whole registration (one launch per workgroup size, at most two); the other items, and those a workgroup hands
 * back, go through exactly those three entries one after another.  An item is never approximated.  DESIGN.md
 * section 9j lists the hand-back reasons.
 * Arguments, ranges, last_idx, inner_iters, per-item statuses and the call's own return value are section 8's; in
 * addition ICP_BAD_ARGUMENT for a batch that is not 2-D and for k outside [3, 16] -- checked, like every argument,
 * before the device is touched.  count == 0 is a successful no-op. */
int icp_batch_estimate_point_to_line(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                     size_t dst_points, const icp_batch_item *items, size_t count, int k, size_t max_iter,
                                     icp_pose *out, int *status, uint32_t *last_idx, uint32_t *inner_iters);
int icp_batch_estimate_point_to_line_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                            size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                            size_t max_iter, icp_pose *out, int *status, uint32_t *d_last_idx,
                                            uint32_t *inner_iters);

/* ================================================================================
 * 16. EXTENSION (not in the reference): the quality of a pose under the point-to-line residual, single and batched
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 13 for 2-D handles: the score of a
 * pose under the residual sections 14 and 15 register with.  Section 9's score uses the point residual: its translation
 * information is c * I whatever the scene looks like, so it cannot see a corridor, and its RMSE measures the sample
 * spacing of the two scans along the walls rather than the fit.  This section gives the line-residual RMSE (the sensor
 * noise where the pose is right) and the unweighted jtj of section 14's accumulation at the pose, rank-deficient
 * exactly where the scene is: what ranks K registered hypotheses and what a pose graph takes as their information.
 * The reference has no such thing: no parity claim; DESIGN.md section 9k restates the definition.
 *
 * It is section 13's definition with the third coordinate removed.  For a 2-D handle with targets dst (m points) and
 * their current line normals nrm (section 14), a source cloud src (n points, caller order), a pose T and max_dist r
 * (r >= 0, or +inf), for every source point p (no FMA anywhere):
 *   qx = (r00 px + r01 py) + tx, qy = (r10 px + r11 py) + ty               (Transform::transform)
 *   j  = the handle's exact 2-D nearest neighbour of (qx, qy); b = dst[j], (nx, ny) = nrm[j]
 *   ex = qx - bx, ey = qy - by
 *   d2 = ex ex + ey ey                                                     (the 2-D icp_evaluate's d2)
 *   inlier = d2 <= r * r (r * r in f64; a NaN d2 is never an inlier)
 *   rp = nx ex + ny ey                          (section 14's line residual at the identity inner pose; the estimator's
 *                                               plane_residual adds a trailing + nz dz = + 0.0, which only turns a
 *                                               -0.0 into +0.0: the square below does not see it)
 *   p2 = rp rp
 *   c  = (nx * (-qy)) + (ny * qx)               (the third entry of section 14's Jacobian row (nx, ny, c) at identity)
 * Ten sums, each by section 9's fold over the n values in caller order (n == 1: the one value); a point that is not an
 * inlier adds +0.0 to the inlier-only sums -- section 13's sums in section 13's order:
 *   S_d2 = fold(inlier ? d2)     S_p2 = fold(inlier ? p2)     E = fold(p2)     H = fold(rho(p2))  (huber.rs)
 *   Ixx = fold(inlier ? nx nx)   Ixy = fold(inlier ? nx ny)   Iyy = fold(inlier ? ny ny)
 *   Ixt = fold(inlier ? nx c)    Iyt = fold(inlier ? ny c)    Itt = fold(inlier ? c c)
 * and the fields from them, on the host, exactly as section 13 forms icp_plane_quality's:
 *   inliers        the count (exact)                  fitness      inliers / n
 *   inlier_sum_d2  S_d2                               inlier_rmse  sqrt(S_d2 / inliers) (0 without inliers): the bits
 *                                                                  icp_evaluate gives at the same T and r
 *   line_sum_r2    S_p2                               line_rmse    sqrt(S_p2 / inliers) (0 without inliers)
 *   error          E                                  huber_error  H (what section 14's evaluation reports as its error)
 *   information    row-major [[Ixx, Ixy, Ixt], [Ixy, Iyy, Iyt], [Ixt, Iyt, Itt]]
 *   translation_eig  lmin, lmax of [[Ixx, Ixy], [Ixy, Iyy]] with + - * sqrt only: h = (Ixx + Iyy) * 0.5,
 *                  g = (Ixx - Iyy) * 0.5, s = sqrt(g g + Ixy Ixy), lmin = h - s, lmax = h + s
 * A target with fewer than three neighbours has the zero normal (section 14): its pairs add zeros, the result is valid.
 *
 * icp_evaluate_point_to_line[_device].  Statuses, decided in this order: ICP_BAD_ARGUMENT (h, T or out NULL; src NULL
 * with n > 0; r NaN or negative; n >= 2^32 - 1: before any device use and before the handle is read); n == 0 -> ICP_OK
 * and zeros; ICP_NO_DEVICE; then the handle: ICP_BAD_ARGUMENT (not a 2-D handle; line normals not current),
 * ICP_EMPTY_DST (no targets); ICP_NAN_INPUT (some p2 is NaN).  *out is the result when the call returns ICP_OK;
 * otherwise it holds n and zeros.  idx / d_idx (nullable): the n correspondences at T, caller order.  The handle's
 * registration state is not touched: an estimate after an evaluation gives the bits it gives without one.
 *
 * icp_batch_evaluate_point_to_line[_device]: section 9's batch call with this residual, for 2-D batches.  Item i's
 * out[i] and status[i] are what icp_create(2, dst + 2 dst_first, m) + icp_compute_target_line_normals(k) +
 * icp_evaluate_point_to_line(src + 2 src_first, n, &items[i].init, max_dist) give on a fresh handle, bit for bit; the
 * first failing step's status is the item's (ICP_EMPTY_DST without targets, ICP_BAD_ARGUMENT where section 14 refuses
 * the targets, ICP_NAN_INPUT), and out[i] then holds n and zeros.  Every item with 1 <= n <= 1024 and 1 <= m <= 2048 runs as ONE
 * workgroup that computes the item's line normals and the score, all of them in one launch; the other items, and those
 * a workgroup hands back, go through exactly those three entries one after another.  An item is
 * never approximated.  Arguments and ranges are section 8's and section 9's: ICP_BAD_ARGUMENT for b, items, out or
 * status NULL with count > 0, a range outside the packed arrays, max_dist NaN or negative, a batch that is not 2-D and
 * k outside [3, 16] -- all before the device is touched; count == 0 is a successful no-op. */
typedef struct icp_line_quality {
  uint64_t n;                 /* source points                                          */
  uint64_t inliers;           /* points with d2 <= max_dist^2                           */
  double fitness;             /* inliers / n                                            */
  double inlier_rmse;         /* sqrt(inlier_sum_d2 / inliers): section 9's             */
  double inlier_sum_d2;       /* fold of the inliers' squared distances                 */
  double line_rmse;           /* sqrt(line_sum_r2 / inliers), 0 without inliers         */
  double line_sum_r2;         /* fold of the inliers' squared line residuals            */
  double error;               /* fold of p2 over all points                             */
  double huber_error;         /* fold of rho(p2) over all points                        */
  double information[9];      /* row-major SE(2) information of the inlier pairs        */
  double translation_eig[2];  /* lmin, lmax of the 2 x 2 translation block              */
} icp_line_quality;
int icp_evaluate_point_to_line(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                               icp_line_quality *out, uint32_t *idx);
int icp_evaluate_point_to_line_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, double max_dist,
                                      icp_line_quality *out, uint32_t *d_idx);
int icp_batch_evaluate_point_to_line(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                     size_t dst_points, const icp_batch_item *items, size_t count, int k, double max_dist,
                                     icp_line_quality *out, int *status);
int icp_batch_evaluate_point_to_line_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                            size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                            double max_dist, icp_line_quality *out, int *status);

/* ================================================================================
 * 17. EXTENSION (not in the reference): section 15's call with a maximum correspondence distance
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Loop-closure candidates and hypotheses far
 * from the truth overlap only partly: they need section 14's gate.  Item i's out[i], status[i], indices, inner counts
 * and inlier counts are what icp_create(2, dst + 2 dst_first, m) + icp_compute_target_line_normals(k) +
 * icp_estimate_point_to_line_gated(src + 2 src_first, n, &init, max_iter, max_dist) return on a fresh handle, bit for
 * bit: per outer iteration the inner loop sees only the pairs with d2 = ex ex + ey ey <= max_dist * max_dist (no FMA;
 * max_dist * max_dist in f64; a NaN d2 is never kept, so a NaN source point is gated out), in the caller's order.
 * Every item within section 15's limits runs as ONE workgroup (one launch per workgroup size, at most two); the other
 * items, and those a workgroup hands back, go through exactly those three entries one after another.  An item is never
 * approximated.  DESIGN.md section 9l.
 * Arguments, ranges, last_idx (the search result of ALL n points in the last iteration), inner_iters, statuses and the
 * return value are section 15's.  inliers: count * max_iter words, nullable, laid out like inner_iters: the number of
 * kept pairs of each outer iteration.  In addition ICP_BAD_ARGUMENT for max_dist NaN or negative (+inf is allowed: every
 * pair with a d2 that is not NaN is kept) -- checked, like every argument, before the device is touched.  count == 0 is a
 * successful no-op. */
int icp_batch_estimate_point_to_line_gated(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                           size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                           size_t max_iter, double max_dist, icp_pose *out, int *status,
                                           uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers);
int icp_batch_estimate_point_to_line_gated_device(icp_batch *b, const double *d_src, size_t src_points,
                                                  const double *d_dst, size_t dst_points, const icp_batch_item *items,
                                                  size_t count, int k, size_t max_iter, double max_dist, icp_pose *out,
                                                  int *status, uint32_t *d_last_idx, uint32_t *inner_iters,
                                                  uint32_t *inliers);

/* ================================================================================
 * 18. EXTENSION (not in the reference): many small point-to-plane registrations in one call
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 8's call with the point-to-plane
 * residual, for 3-D batches: submap patches, object segments, voxel-thinned frames, K pose hypotheses against one small
 * cloud.  Item i's out[i], status[i], indices and inner counts are what icp_create(3, dst + 3 dst_first, m) +
 * icp_compute_target_normals(k) + icp_estimate_point_to_plane(src + 3 src_first, n, &init, max_iter) return on a fresh
 * handle, bit for bit (the ungated call; a first failing step's status is the item's: ICP_EMPTY_DST without targets,
 * ICP_BAD_ARGUMENT where icp_compute_target_normals refuses them, ICP_NAN_INPUT).  Every item with 1 <= n <= 1024,
 * 1 <= m <= 2048 and 1 <= max_iter <= 1024 runs as ONE workgroup that computes the item's plane normals and the whole
 * registration (one launch per workgroup size, at most two); the other items, and those a workgroup hands back, go
 * through exactly those three entries one after another.  An item is never approximated.  DESIGN.md section 9m lists
 * the hand-back reasons.
 * Arguments, ranges, last_idx, inner_iters, per-item statuses and the call's own return value are section 8's; in
 * addition ICP_BAD_ARGUMENT for a batch that is not 3-D and for k outside [3, 16] -- checked, like every argument,
 * before the device is touched.  count == 0 is a successful no-op. */
int icp_batch_estimate_point_to_plane(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                      size_t dst_points, const icp_batch_item *items, size_t count, int k, size_t max_iter,
                                      icp_pose *out, int *status, uint32_t *last_idx, uint32_t *inner_iters);
int icp_batch_estimate_point_to_plane_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                             size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                             size_t max_iter, icp_pose *out, int *status, uint32_t *d_last_idx,
                                             uint32_t *inner_iters);

/* ================================================================================
 * 19. EXTENSION (not in the reference): section 18's call with a maximum correspondence distance
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  A submap patch with an object the map does not
 * hold, a loop-closure candidate, a far hypothesis overlap their targets only partly: they need section 12's gate.  Item
 * i's out[i], status[i], indices, inner counts and inlier counts are what icp_create(3, dst + 3 dst_first, m) +
 * icp_compute_target_normals(k) + icp_estimate_point_to_plane_gated(src + 3 src_first, n, &init, max_iter, max_dist)
 * return on a fresh handle, bit for bit: per outer iteration the inner loop sees only the pairs with
 * d2 = (ex ex + ey ey) + dz dz <= max_dist * max_dist (no FMA; max_dist * max_dist in f64; a NaN d2 is never kept, so a
 * NaN source point is gated out), in the caller's order.  Every item within section 18's limits runs as ONE workgroup
 * (one launch per workgroup size, at most two); the other items, and those a workgroup hands back, go through exactly
 * those three entries one after another.  An item is never approximated.  DESIGN.md section 9n.
 * Arguments, ranges, last_idx (the search result of ALL n points in the last iteration), inner_iters, statuses and the
 * return value are section 18's.  inliers: count * max_iter words, nullable, laid out like inner_iters: the number of
 * kept pairs of each outer iteration.  In addition ICP_BAD_ARGUMENT for max_dist NaN or negative (+inf is allowed: every
 * pair with a d2 that is not NaN is kept) -- checked, like every argument, before the device is touched.  count == 0 is a
 * successful no-op. */
int icp_batch_estimate_point_to_plane_gated(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                            size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                            size_t max_iter, double max_dist, icp_pose *out, int *status,
                                            uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers);
int icp_batch_estimate_point_to_plane_gated_device(icp_batch *b, const double *d_src, size_t src_points,
                                                   const double *d_dst, size_t dst_points, const icp_batch_item *items,
                                                   size_t count, int k, size_t max_iter, double max_dist, icp_pose *out,
                                                   int *status, uint32_t *d_last_idx, uint32_t *inner_iters,
                                                   uint32_t *inliers);

/* ================================================================================
 * 20. EXTENSION (not in the reference): the point-to-plane quality of many poses in one call
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 16's batch call with section 13's
 * residual, for 3-D batches: K submap patches, loop-closure candidates or hypotheses registered by section 18 are ranked
 * by plane_rmse and handed to a pose graph with the information the plane residual gives (section 9's batch score has
 * c I for its translation block whatever the scene looks like).  Item i's out[i] and status[i] are what
 * icp_create(3, dst + 3 dst_first, m) + icp_compute_target_normals(k) +
 * icp_evaluate_point_to_plane(src + 3 src_first, n, &items[i].init, max_dist) give on a fresh handle, bit for bit; the
 * first failing step's status is the item's (ICP_EMPTY_DST without targets, ICP_BAD_ARGUMENT where
 * icp_compute_target_normals refuses the targets, ICP_NAN_INPUT), and out[i] then holds n and zeros.  Every item with
 * 1 <= n <= 1024 and 1 <= m <= 2048 (section 18's limits) runs as ONE workgroup that computes the item's plane normals
 * and the score, all of them in one launch; the other items, and those a workgroup hands back,
 * go through exactly those three entries one after another.  An item is never approximated.  Arguments and ranges are
 * section 8's and section 9's: ICP_BAD_ARGUMENT for b, items, out or status NULL with count > 0, a range outside the
 * packed arrays, max_dist NaN or negative, a batch that is not 3-D and k outside [3, 16] -- all before the device is
 * touched; count == 0 is a successful no-op. */
int icp_batch_evaluate_point_to_plane(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                      size_t dst_points, const icp_batch_item *items, size_t count, int k, double max_dist,
                                      icp_plane_quality *out, int *status);
int icp_batch_evaluate_point_to_plane_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                             size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                             double max_dist, icp_plane_quality *out, int *status);

/* ================================================================================
 * 21. EXTENSION (not in the reference): section 8's call with a maximum correspondence distance
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  K hypotheses of one scan, loop-closure
 * candidates, a log replayed against keyframes overlap their targets only partly: they need section 10's gate.  Item i's
 * out[i], status[i], indices, inner counts and inlier counts are what icp_create(dim, dst + dim dst_first, m) +
 * icp_estimate_gated(src + dim src_first, n, &init, max_iter, max_dist) return on a fresh handle, bit for bit, for 2-D
 * and 3-D batches: per outer iteration the inner loop sees only the pairs with d2 = (ex ex + ey ey) + ez ez <=
 * max_dist * max_dist (ez: 3-D batches only; no FMA; max_dist * max_dist in f64; a NaN d2 is never kept, so a NaN source
 * point is gated out and is not ICP_NAN_INPUT: that is reported for a kept pair with a NaN residual, as in section 10),
 * in the caller's order.  Every item within section 8's limits runs as ONE workgroup (one launch per workgroup size, at
 * most three); the other items, and those a workgroup hands back, go through exactly those two entries one after
 * another.  An item is never approximated.  DESIGN.md section 9r.
 * Arguments, ranges, last_idx (the search result of ALL n points in the last iteration), inner_iters, statuses and the
 * return value are section 8's.  inliers: count * max_iter words, nullable, laid out like inner_iters: the number of
 * kept pairs of each outer iteration.  In addition ICP_BAD_ARGUMENT for max_dist NaN or negative (+inf and 0.0 are
 * allowed: +inf keeps every pair with a d2 that is not NaN) -- checked, like every argument, before the device is
 * touched.  count == 0 is a successful no-op. */
int icp_batch_estimate_gated(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                             const icp_batch_item *items, size_t count, size_t max_iter, double max_dist, icp_pose *out,
                             int *status, uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers);
int icp_batch_estimate_gated_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                    size_t dst_points, const icp_batch_item *items, size_t count, size_t max_iter,
                                    double max_dist, icp_pose *out, int *status, uint32_t *d_last_idx,
                                    uint32_t *inner_iters, uint32_t *inliers);

/* ================================================================================
 * 22. EXTENSION (not in the reference): voxel thinning -- one point per voxel, for clouds and for a handle's targets
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  A map fed by icp_append_targets (section 6)
 * gains a layer of near-duplicates at every revisit of a place, and a lidar front end thins a frame before it registers
 * it (the "voxel-thinned frames" of section 18): both keep at most one point per voxel.  The reference has no such
 * thing: no parity claim; DESIGN.md section 9s restates the definition.
 *
 * The rule.  For a point p with dim coordinates and a voxel size v:
 *   the cell coordinate on axis a is the f64 value floor(p_a / v): ONE IEEE division, then floor; never a product with
 *   1 / v (the two differ, e.g. for 195 of the 2 000 inputs k * 0.1, k in [-1000, 1000), at v = 0.1);
 *   two points share a voxel iff their cell coordinates compare equal as doubles on every axis: -0.0 == +0.0; a quotient
 *   that overflows to +-inf is a cell coordinate like any other; cell coordinates are never narrowed to an integer type,
 *   so there is no range to exceed and no status for it;
 *   a point with a NaN or infinite coordinate belongs to no voxel and is dropped;
 *   of every voxel the point with the LOWEST INDEX is kept, the others are dropped;
 *   kept points keep their relative order and their bits (a kept -0.0 stays -0.0).
 * v must be finite and at least DBL_MIN: a NaN, zero, negative, subnormal or infinite v is ICP_BAD_ARGUMENT.
 * In numpy:  ok = isfinite(p).all(axis=1);  c = floor(p / v) + 0.0;  _, first = unique(c[ok], axis=0, return_index=True);
 *            kept_index = sort(flatnonzero(ok)[first]).
 * The result is a pure function of the input: the same bytes from every call.
 *
 * icp_voxel_downsample (host arrays) and icp_voxel_downsample_device (device arrays; everything is enqueued on
 * hip_stream, NULL: the default stream, and the entry waits for that stream to deliver *kept): dim is 2 or 3; pts holds n
 * points; out (nullable) receives the kept points and needs room for n of them; it must not overlap pts; kept_index
 * (nullable) receives their indices in pts, ascending, room for n; *kept (required) their number.  n == 0 gives
 * *kept = 0 and ICP_OK.  device: -1 = the current one.  Statuses: ICP_BAD_ARGUMENT (dim, v as above, kept NULL, pts NULL
 * with n > 0, n > 2^32 - 2, device < -1: all decided before the device is touched; a device number past the last one),
 * ICP_NO_DEVICE, ICP_HIP_ERROR, ICP_OUT_OF_MEMORY.  The workspace (a hash table of 2^ceil(log2(2 n)) words, one mark per
 * point, the tile counts; for the host entry also the staging buffers) is kept per device between calls and grown when a
 * larger cloud comes: no allocation per frame.  The calls of one process take turns.  icp_trim_pool releases it.
 *
 * icp_thin_targets: section 11's call with this keep rule in place of the disc.  Everything section 11 says of the
 * handle after a crop holds after a thin: order, bits, new_index (nullable, host, m_before words; 0xffffffff = removed),
 * *removed (nullable), correspondences and poses of a fresh icp_create on the kept cloud, normals carried over and their
 * count, the edges (nothing removed: the handle is untouched and keeps borrowing; everything else: it owns its cloud;
 * a cloud of only non-finite points: all removed), the statuses (ICP_BAD_ARGUMENT: h NULL or v as above, before any
 * device use) and the way back on failure.  Because the lowest index wins, a thin after an append keeps every target
 * that was kept by the thin before it and drops exactly the new points that fall into an occupied voxel.
 * icp_multi_thin_targets: every rank thins its replica, as icp_multi_crop_targets crops it. */
int icp_voxel_downsample(int dim, const double *pts, size_t n, double voxel, double *out, uint32_t *kept_index,
                         size_t *kept, int device);
int icp_voxel_downsample_device(int dim, const double *d_pts, size_t n, double voxel, double *d_out,
                                uint32_t *d_kept_index, size_t *kept, int device, void *hip_stream);
int icp_thin_targets(icp_handle *h, double voxel, uint32_t *new_index, size_t *removed);
int icp_multi_thin_targets(icp_multi *M, double voxel, size_t *removed);

/* ================================================================================
 * 23. EXTENSION (not in the reference): exact k-nearest target lists and neighbourhood outlier removal
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  The cloud-hygiene step beside the voxel filter
 * of section 22: dropping targets whose neighbourhood is too sparse (dust, rain, mixed pixels, ghost points), by the
 * radius rule or by the statistical rule, and the lists both rest on.  The reference has no such thing: no parity claim;
 * DESIGN.md section 9u restates the definitions, tests/test_outlier_abi.py restates them in numpy.
 *
 * Throughout, d2(i, j) = dx dx + dy dy (+ dz dz) with dx = p_i - p_j, a left fold without FMA, exactly as sections 7 and
 * 14 form it; a d2 that overflows to +inf is a distance like any other.  All three calls need the handle's grid: a
 * handle whose targets are not all finite has none and answers ICP_BAD_ARGUMENT (as icp_compute_target_normals).
 *
 * icp_target_neighbours (host out) / icp_target_neighbours_device (device out, enqueued on the handle's stream:
 * icp_synchronize before reading).  Row i - first holds, for target i in [first, first + count), its min(k, m) nearest
 * targets, ITSELF INCLUDED, ordered by (d2, index) ascending -- the tie rule of sections 7 and 14.  idx and d2 are
 * count x k, row-major; either may be NULL.  With m < k the tail of a row is idx = 0xffffffff, d2 = +inf.
 * 1 <= k <= 32.  Statuses: ICP_BAD_ARGUMENT (h NULL or k out of range: before any device use; first + count > m or no
 * grid: from the handle's state), ICP_EMPTY_DST (m == 0), ICP_OK for count == 0, ICP_NO_DEVICE, ICP_HIP_ERROR,
 * ICP_OUT_OF_MEMORY.  In numpy: order = lexsort((arange(m), d2[i])); idx = order[:k]; d2 = d2[i][order[:k]].
 *
 * icp_remove_radius_outliers.  Target i is KEPT iff  #{ j : d2(i, j) <= radius * radius } >= min_neighbours,  j over
 * ALL targets, i included (so min_neighbours <= 1 keeps everything and min_neighbours > m removes everything);
 * radius * radius is one f64 product.  radius >= 0 or +inf; a NaN or negative radius is ICP_BAD_ARGUMENT (with h NULL:
 * before any device use).  In numpy: keep = (d2 <= r * r).sum(1) >= min_neighbours.
 *
 * icp_remove_statistical_outliers.  1 <= k <= 31; std_ratio any double but a NaN (both, and h NULL: ICP_BAD_ARGUMENT
 * before any device use).  Every step is the definition of the bits:
 *   ke = min(k, m - 1); with m <= 1 nothing is removed and stats are +0.0;
 *   u_i = (sum of sqrt(d2) over the first ke entries, other than the one whose index is i, of target i's list of length
 *         ke + 1) / (double)ke: a left fold from the nearest that starts from the first term, the correctly rounded
 *         sqrt, a division (never a product with a reciprocal);
 *   mean = fold(u) / (double)m;  deviation = sqrt(fold((u - mean)^2) / (double)(m - 1)), fold = the tree of section 9
 *         (groups of 256, s = 128 ... 1, level after level);
 *   threshold = mean + std_ratio * deviation: two roundings, no FMA;
 *   target i is KEPT iff !(u_i > threshold): a NaN threshold (an infinite u; std_ratio = +-inf with deviation == 0)
 *         keeps everything.
 * stats (nullable) receives {mean, deviation, threshold}.
 *
 * After either filter everything section 11 says of a handle after a crop holds: order, bits, new_index (nullable, host,
 * m_before words; 0xffffffff = removed), *removed (nullable), the results of a fresh icp_create on the kept cloud, normals
 * carried over, the edges (nothing removed: the handle is untouched and keeps borrowing; everything removed) and the way
 * back on failure.  The scratch (8 B per target, the tree's records, three scalars; the host list entry's staging rows)
 * is kept per device between calls; icp_trim_pool releases it.  Results are pure functions of the input. */
int icp_target_neighbours(icp_handle *h, int k, size_t first, size_t count, uint32_t *idx, double *d2);
int icp_target_neighbours_device(icp_handle *h, int k, size_t first, size_t count, uint32_t *d_idx, double *d_d2);
int icp_remove_radius_outliers(icp_handle *h, double radius, size_t min_neighbours, uint32_t *new_index, size_t *removed);
int icp_remove_statistical_outliers(icp_handle *h, int k, double std_ratio, uint32_t *new_index, size_t *removed,
                                    double stats[3]);

/* ================================================================================
 * 24. EXTENSION (not in the reference): neighbour queries of arbitrary points, and target removal by the caller's mask
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  Section 23 answers only for points that are
 * targets already, and removes only by its own two rules.  These calls answer for ANY points -- cloud-to-map distance,
 * density, change detection, local fits around scan points -- and remove by a verdict the caller computed: query,
 * decide, remove.  The reference has no such thing: no parity claim; DESIGN.md section 9v restates the definitions,
 * tests/test_query_abi.py restates them in numpy.  Every step below is the definition of the bits.
 *
 * The query point.  q holds n points of dim coordinates each (AoS).  With pose == NULL the coordinates are used exactly
 * as given.  Otherwise  px = (r00 x + r01 y) + tx,  py = (r10 x + r11 y) + ty,  z kept: Transform::transform as section 7
 * forms it -- the two products, their sum, then + t, no FMA.  NULL is NOT a product with the identity: 0 * inf is NaN, so
 * a point with an infinite coordinate differs between the two.
 * The distance.  d2 = dx dx + dy dy (+ dz dz) with dx = p - t, a left fold without FMA, as sections 7, 14 and 23 form
 * it.  A d2 that overflows to +inf is a distance like any other.  A NaN d2 (a NaN coordinate of p) is no neighbour.
 * All four query calls need the handle's grid: a handle whose targets are not all finite has none and answers
 * ICP_BAD_ARGUMENT (as section 23).
 *
 * icp_query_neighbours (host in, host out) / icp_query_neighbours_device (device in and out, enqueued on the handle's
 * stream: icp_synchronize before reading).  Row i holds the min(k, m) nearest targets of query i by (d2, index)
 * ascending; idx and d2 are n x k, row-major, padded with 0xffffffff / +inf; either may be NULL.  1 <= k <= 32.  A query
 * with a NaN coordinate gets a row of padding only.  A query with an infinite coordinate (and no NaN) has d2 = +inf to
 * every target and so gets the targets 0 .. min(k, m) - 1 with d2 = +inf.
 * In numpy:  cand = flatnonzero(~isnan(d2[i]));  order = cand[lexsort((cand, d2[i][cand]))][:k].
 *
 * icp_count_within / icp_count_within_device.  counts[i] = min(cap, #{ j : d2(p_i, t_j) <= radius * radius });
 * radius * radius is one f64 product; radius >= 0 or +inf, a NaN or negative radius is ICP_BAD_ARGUMENT; cap >= 1, and
 * cap = 0xffffffff gives the full count (a count stops at cap: with a small cap a large radius stays cheap).  A NaN query
 * counts 0; an infinite one counts min(cap, m) iff radius * radius is +inf, else 0 -- both by the arithmetic above.
 * q == NULL: the queries are the handle's targets in index order; this takes pose == NULL and n == m (else
 * ICP_BAD_ARGUMENT: for the pose before any device use, for n from the handle's state).  Then  counts[i] >= min_neighbours  with cap = min_neighbours is the keep rule of
 * icp_remove_radius_outliers.
 *
 * Order of service.  Results are per query, so the order in which the device serves the queries changes no bit.  Calls
 * with at least 250 000 points sort them by target-grid cell first (the sort of icp_sort_source_device), smaller ones go
 * in the caller's order.  Such a call treats the handle's search snapshot as icp_sort_source_device does: the snapshot
 * belongs to the call and is invalid afterwards, and icp_last_fold_order reports the identity until the next estimate
 * call.  An estimate call after a query returns the bits it returns without the query.
 *
 * icp_remove_targets (keep: m bytes on the host) / icp_remove_targets_device (d_keep: m bytes on the handle's device,
 * complete when the call is made).  Target i is kept iff keep[i] != 0.  Everything section 11 says of a handle after a
 * crop holds: order, bits, new_index (nullable, host, m_before words; 0xffffffff = removed), *removed (nullable), the
 * results of a fresh icp_create on the kept cloud, normals carried over, the edges (nothing removed: the handle is
 * untouched and keeps borrowing; everything removed) and the way back on failure.  Like a crop it needs no grid.
 * m == 0 is a successful no-op.  It counts in its own pair (icp_grid_remove_counters, icp_mi355x_debug.h).
 *
 * Statuses.  ICP_BAD_ARGUMENT before any device use: h NULL, k outside [1, 32], cap == 0, radius NaN or negative, q NULL
 * with n > 0 (icp_query_neighbours*), q NULL with a pose (icp_count_within*), counts NULL with n > 0, n >= 2^32 - 1,
 * keep NULL.  Then ICP_NO_DEVICE.  Then, from the handle's state, for the four query calls: ICP_EMPTY_DST (m == 0),
 * ICP_BAD_ARGUMENT (no grid; q NULL with n != m).  Then ICP_OK for n == 0.  ICP_OUT_OF_MEMORY when the host entries' staging cannot be allocated,
 * ICP_HIP_ERROR.  The staging (the points, the rows, the counts, the mask) is kept per device between calls; the calls
 * of one process that use it take turns; icp_trim_pool releases it.  Results are pure functions of the input. */
int icp_query_neighbours(icp_handle *h, const double *q, size_t n, const icp_pose *pose, int k, uint32_t *idx, double *d2);
int icp_query_neighbours_device(icp_handle *h, const double *d_q, size_t n, const icp_pose *pose, int k, uint32_t *d_idx,
                                double *d_d2);
int icp_count_within(icp_handle *h, const double *q, size_t n, const icp_pose *pose, double radius, uint32_t cap,
                     uint32_t *counts);
int icp_count_within_device(icp_handle *h, const double *d_q, size_t n, const icp_pose *pose, double radius, uint32_t cap,
                            uint32_t *d_counts);
int icp_remove_targets(icp_handle *h, const uint8_t *keep, uint32_t *new_index, size_t *removed);
int icp_remove_targets_device(icp_handle *h, const uint8_t *d_keep, uint32_t *new_index, size_t *removed);

/* ================================================================================
 * 25. EXTENSION (not in the reference): voxel centroids -- per voxel the mean, the count and the point-to-voxel map
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  The voxel-grid filter as lidar pipelines know
 * it: one point per occupied voxel, the MEAN of the voxel's points, with the number of members as a weight.  Section 22
 * keeps one sample of every voxel; the mean is the lower-noise source cloud of a registration, the counts serve a
 * weighted consumer or an occupancy threshold.  The reference has no such thing: no parity claim; DESIGN.md section 9w
 * restates the definition, tests/test_voxel_mean_abi.py restates it in numpy (centroids_of).
 *
 * The rule.  For n points of dim coordinates and a voxel size v, every step is the definition of the bits:
 *   membership is section 22's, exactly: the cell is floor(p_a / v) + 0.0 per axis in f64 with ONE division; two points
 *   share a voxel iff their cells are equal as doubles; a point with a NaN or infinite coordinate is in no voxel;
 *   the occupied voxels are numbered in ascending order of their LOWEST member index -- the order of
 *   icp_voxel_downsample's kept points, so first_index here equals kept_index there, element for element;
 *   for voxel r with the members i_0 < i_1 < ... < i_(c-1):
 *     count[r] = c;
 *     per axis a,  sum = fold(x[i_0, a], ..., x[i_(c-1), a]),  fold = the tree of section 9 verbatim: c == 1 -> the value
 *     itself; otherwise, while more than one value is left: pad with +0.0 to a multiple of 256, g[i] += g[i + s] for
 *     s = 128, 64, ..., 1 inside every group of 256, keep every group's g[0];
 *     mean[r, a] = sum / (double)c: one IEEE division, no FMA, never a product with a reciprocal;
 *   voxel_of[i] = the number r of point i's voxel, 0xffffffff for a point in no voxel (the "gone" of the new_index tables).
 * What follows from it:
 *   a voxel of one member returns that point's bytes: a -0.0 stays -0.0;
 *   a voxel of c >= 2 members that are all -0.0 on an axis gives +0.0 there (the padding: -0.0 + +0.0 = +0.0);
 *   a sum that overflows gives +-inf, and the mean with it.  The members of a voxel share their sign on every axis (the
 *   cell 0 holds [0, v) and -0.0, the cells below only negative values), so inf - inf does not arise and no mean is a NaN;
 *   the result is a pure function of the input: the same bytes from every call, every stream, every device.
 * In numpy (kept_index_of: section 22's restatement):
 *   first = kept_index_of(p, v);  voxel_of = rank of each finite point's cell in the order of first;
 *   mean[r] = [fold(p[voxel_of == r, a]) for a] / count[r].
 *
 * icp_voxel_centroids (host arrays) and icp_voxel_centroids_device (device arrays; everything is enqueued on hip_stream,
 * NULL: the default stream, and the entry returns after the one wait that delivers *voxels): dim is 2 or 3; pts holds n
 * points and is never written.  mean (room for n points), count, first_index (room for n words each) and voxel_of (n
 * words) are each nullable, and what is not asked for is not computed; none may overlap pts.  *voxels (required) receives
 * the number of occupied voxels: the first *voxels entries of mean, count and first_index are the result.  n == 0 gives
 * *voxels = 0 and ICP_OK.  device: -1 = the current one.  Statuses: ICP_BAD_ARGUMENT (dim, v as in section 22, voxels
 * NULL, pts NULL with n > 0, n > 2^32 - 2, n > 2^27 when mean or count is asked for -- the limit of the sort underneath --,
 * device < -1: all decided before the device is touched, and a refused call writes nothing; a device number past the
 * last one), ICP_NO_DEVICE, ICP_HIP_ERROR, ICP_OUT_OF_MEMORY.  The workspace is section 22's, grown by the sort keys,
 * the sorted order, the segment starts (4 B per point each), the sort's temporary (about 16 B per point) and the lists of
 * the voxels above 256 members; icp_trim_pool releases all of it.  The calls of one process take turns with section 22's.
 * A voxel of any size is folded by as many workgroups as it has blocks of 65 536 members, and of the points of a wave
 * that share a cell only one goes to the table: a v far too large -- the whole cloud in one voxel -- stays within a small
 * factor of a well-chosen one (DESIGN.md section 9w has the measured row). */
int icp_voxel_centroids(int dim, const double *pts, size_t n, double voxel, double *mean, uint32_t *count,
                        uint32_t *first_index, uint32_t *voxel_of, size_t *voxels, int device);
int icp_voxel_centroids_device(int dim, const double *d_pts, size_t n, double voxel, double *d_mean, uint32_t *d_count,
                               uint32_t *d_first_index, uint32_t *d_voxel_of, size_t *voxels, int device, void *hip_stream);

/* ================================================================================
 * 26. EXTENSION (not in the reference): voxel covariances -- per voxel the mean, the count and the second moments
 * ==============================================================================
 * An addition to ABI 8, detectable by symbol (ICP_ABI_VERSION stays 8).  The other half of the voxel statistic of lidar
 * pipelines: mean and covariance per voxel are what an NDT map, a voxelised GICP, a surfel map or a planarity filter is
 * built from.  The reference has no such thing: no parity claim; DESIGN.md section 9x restates the definition,
 * tests/test_voxel_cov_abi.py restates it in numpy (covariances_of).
 *
 * The rule.  Membership, the numbering of the voxels, count, first_index, voxel_of and mean are section 25's, bit for
 * bit.  For voxel r with the members i_0 < ... < i_(c-1) and the mean m (section 25's bits), over the axis pairs (a, b),
 * a <= b, in the order xx, xy, yy (dim 2) and xx, xy, xz, yy, yz, zz (dim 3):
 *   d_j[a]  = x[i_j, a] - m[a]                    one f64 subtraction;
 *   p_j[ab] = d_j[a] * d_j[b]                     one f64 multiplication, never fused with the addition behind it;
 *   S[ab]   = fold(p_0[ab], ..., p_(c-1)[ab])     the tree of section 9 as section 25 states it: c == 1 -> the value;
 *             otherwise pad with +0.0 to groups of 256, g[i] += g[i + s] for s = 128 ... 1, level after level;
 *   cov[r, ab] = S[ab] / (double)(c - ddof)       one IEEE division; ddof is 0 (the population's) or 1 (the sample's).
 *             A voxel with c <= ddof gets +0.0 in every entry.
 * The two passes (the mean first, the products of the deviations second) are what keeps a cloud far from the origin
 * accurate: the one-pass E[xx] - mm loses every digit once the offset squared outgrows 2^53 variances.
 * What follows from it:
 *   a voxel of one member gives +0.0 in every entry, for either ddof;
 *   a diagonal entry is a sum of squares: never negative, never a NaN for a finite mean;
 *   an off-diagonal entry is a NaN only where products overflow to infinities of both signs (host and device differ in
 *   the sign bit of that NaN: compare such positions as "is a NaN", everything else by bytes);
 *   a mean that overflowed to +-inf on an axis gives infinite deviations there (an entry is then +-inf, or a NaN where the
 *   other axis' deviation is zero or the infinities' signs are mixed);
 *   the result is a pure function of the input: the same bytes from every call, every stream, every device.
 *
 * icp_voxel_covariances (host arrays) and icp_voxel_covariances_device (device arrays; everything is enqueued on
 * hip_stream, NULL: the default stream, and the entry returns after the one wait that delivers *voxels): as section 25's
 * entries, with cov (REQUIRED: room for n * dim (dim + 1) / 2 doubles, the packed order above, voxel after voxel) and
 * ddof in front of section 25's outputs.  mean, count, first_index and voxel_of are each nullable; a mean that is not
 * asked for is computed into the workspace.  The first *voxels rows of cov, mean, count and first_index are the result.
 * n == 0 gives *voxels = 0 and ICP_OK.  Statuses: ICP_BAD_ARGUMENT (section 25's refusals, ddof not 0 or 1, cov NULL,
 * and n > 2^27 always, since cov needs the sort: all decided before the device is touched, and a refused call writes
 * nothing; a device number past the last one), ICP_NO_DEVICE, ICP_HIP_ERROR, ICP_OUT_OF_MEMORY.  The workspace is
 * section 25's, with six sums per record of a voxel above 65 536 members and the host entry's staging of cov;
 * icp_trim_pool releases it.  The calls of one process take turns with sections 22's and 25's. */
int icp_voxel_covariances(int dim, const double *pts, size_t n, double voxel, int ddof, double *cov, double *mean,
                          uint32_t *count, uint32_t *first_index, uint32_t *voxel_of, size_t *voxels, int device);
int icp_voxel_covariances_device(int dim, const double *d_pts, size_t n, double voxel, int ddof, double *d_cov,
                                 double *d_mean, uint32_t *d_count, uint32_t *d_first_index, uint32_t *d_voxel_of,
                                 size_t *voxels, int device, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* ICP_MI355X_H */
