/* Observability of libicp_mi355x.so: which pipeline served what, timing hooks of the benchmark.  Test and profiling
 * infrastructure -- NOT part of the drop-in boundary (include/icp_mi355x.h, sections 1-7, is what a binding of the
 * reference's API needs); the symbols are exported by the product library so that the -m gpu tests can prove which
 * path ran.  No result depends on any of them. */
#ifndef ICP_MI355X_DEBUG_H
#define ICP_MI355X_DEBUG_H

#include "icp_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Observability for tests: which pipeline served the weighted Gauss-Newton evaluations of
 * this handle (NULL: the scratch handle behind the free functions) since it was created.
 * out[0] evaluations started with the three-launch window pipeline, out[1] how many of those
 * missed their window and were repeated, out[2] evaluations by the seven-launch (or
 * single-workgroup) pipeline, out[3] by the full-key selection; out[4] / out[5]
 * speculative searches of icp_estimate[_device] whose pose was confirmed / discarded.  Every
 * path returns the same bits; the counters only show that a test exercised what it meant to. */
int icp_gn_path_counters(icp_handle *h, uint64_t out[6]);

/* ... and the one-launch inner loop (gn_loop.hip: the whole estimate_transform loop, src/lib.rs:59-84, of a pair set of
 * up to 2^20 in one launch): out[0] launches, out[1] evaluations they served (counted in out[0] of
 * icp_gn_path_counters as well), out[2] launches that handed an evaluation back to the host-stepped pipelines. */
int icp_gn_loop_counters(icp_handle *h, uint64_t out[3]);
/* launches of the one-launch inner loop that were not fully resident and gave up their bounded wait (2 ms without a
 * workgroup arriving at the grid barrier; 3 s between the ranks of a sharded launch).  After one, the handle steps its
 * next 64 inner loops from the host and then tries the launch again. */
int icp_gn_loop_timeouts(icp_handle *h, uint64_t *out);
/* outer iterations of icp_estimate[_device] that were not run because the one before them had left the pose as it found
 * it, bit for bit: every later iteration would repeat it (src/lib.rs:105-130 is a function of the pose and the clouds),
 * so only the last one -- which reports the correspondences -- still runs.  The inner counts of the skipped ones are 0. */
int icp_fixed_point_skips(icp_handle *h, uint64_t *out);

/* ... and the run-ahead searches of icp_estimate[_device] (a search enqueued behind the pre-launched first evaluation
 * of the next iteration, its pose derived on the device): out[0] the host derived the same pose bit for bit and took
 * the pairs, out[1] it derived another (the search was repeated for the host's pose).  A run-ahead search behind an
 * evaluation that missed its window finds no pose on the device, does not run and is counted in neither. */
int icp_run_ahead_counters(icp_handle *h, uint64_t out[2]);

/* Observability: evaluations with filed candidates (gn_win.hip: k_win_hist_sums_bkt / _bkt2 and the finishing launches
 * k_win_pick / k_win_pick2, one workgroup per dimension; the sharded finish counts too).  out[0] = such evaluations
 * launched since the handle was created, out[1] = window evaluations still to take the second pass over the points
 * after files that were not usable (they count down to 0).  h = NULL: the scratch handle behind the free functions. */
int icp_gn_filed_counters(icp_handle *h, uint64_t out[2]);

/* Observability: certified matches (the searches of an estimate call after the first, beyond 65 536 source points:
 * a query whose previous match is provably still its nearest neighbour -- it has moved less than the margin the
 * last walk left it -- is not searched again).  out[0] = searches that checked certificates
 * since the handle was created, out[1] = queries whose certificate failed in the last of them (searched as ever).
 * (The library reads no tuning variables) */
int icp_nn_cert_counters(icp_handle *h, uint64_t out[2]);

int icp_single_launch_counters(icp_handle *h, uint64_t out[3]);

/* Observability: out[0] = appends served incrementally (the sorted records of the search grid move up by their cells'
 * shifts and the new ones fill the gaps: possible while every new point lies within half a cell of the grid's box and
 * the cloud has grown by less than half since the grid's cell size was chosen), out[1] = appends that rebuilt the grid.
 * Either way the handle afterwards answers like a fresh handle on the concatenated cloud (in the sense stated at the
 * top of this section). */
int icp_grid_append_counters(const icp_handle *h, uint64_t out[2]);

/* ... and of icp_crop_targets (icp_mi355x.h section 11): out[0] = crops served by moving the grid's sorted records
 * (a second stable compaction in record order, cell offsets by one gather: no atomics, no re-sort; the grid keeps the box
 * and cell size of its last full build), out[1] = crops that rebuilt the grid (no grid was built, nothing was kept, or
 * the kept cloud fell below 1 / 1.5 of the cloud the cell size was chosen for).  A crop that removes nothing counts in
 * neither. */
int icp_grid_crop_counters(const icp_handle *h, uint64_t out[2]);

/* ... and of icp_thin_targets (icp_mi355x.h section 22), which shares the crop's back half and counts for itself:
 * out[0] = thins served by moving the grid's sorted records, out[1] = thins that rebuilt the grid, under the same
 * conditions.  A thin that removes nothing counts in neither; a thin never moves the crop's counters. */
int icp_grid_thin_counters(const icp_handle *h, uint64_t out[2]);
/* ... and of icp_remove_radius_outliers / icp_remove_statistical_outliers (icp_mi355x.h section 23), which count
 * together and for themselves: out[0] = filters served by moving the grid's sorted records, out[1] = filters that rebuilt
 * the grid, under the same conditions.  A filter that removes nothing counts in neither. */
int icp_grid_outlier_counters(const icp_handle *h, uint64_t out[2]);

int icp_multi_counters(const icp_multi *M, uint64_t out[2]);

/* ... and of the one-launch inner loop across the ranks (section 5b): out[0] launches (per rank), out[1] evaluations they
 * served, out[2] launches that handed an evaluation back to the stage calls.  ICP_NO_GN_LOOP=1: stage calls only; an icp_multi whose launches once gave up
 * waiting for each other (ranks that share a device need all their workgroups running at once) serves through the stage
 * calls from then on, silently: the results are the same bits either way. */
int icp_multi_loop_counters(const icp_multi *M, uint64_t out[3]);

/* ... and of the pipelined sharded registration (section 5c): outer iterations it served over the life of `M`; per
 * handle: out[0] iterations served, out[1] hand-backs, out[2] waits for a peer that ran out, out[3] run-ahead searches
 * whose pose the host confirmed. */
int icp_multi_pipe_iterations(const icp_multi *M, uint64_t *out);
int icp_pipe_counters(icp_handle *h, uint64_t out[4]);

/* enable = 0: icp_estimate[_device] on this handle runs every one of its max_iter outer iterations, also those behind a
 * fixed point of the loop (the default leaves them out: they repeat the fixed point -- same pose, indices and inner
 * counts either way).  What bench.py's `converging_pair.all_twenty_run` times.  Large clouds only (the one-launch
 * registration of clouds of up to 1 024 points has its own exit). */
int icp_set_fixed_point_exit(icp_handle *h, int enable);

/* The per-call sort of the source points by target-grid cell (csrc/qsort.hip: hand-written LSD radix sort, digits of up to
 * eleven bits) alone, on host arrays: keys_out = the keys ascending, perm_out = their original indices, equal keys in
 * ascending index -- the order icp_last_fold_order documents.  bits: the keys' significant bits (1 .. 32). */
int icp_debug_sort_cells(const uint32_t *keys, size_t n, unsigned bits, uint32_t *keys_out, uint32_t *perm_out);

/* Batched small registrations (icp_mi355x.h section 8), since icp_batch_create: out[0] items served inside a batch
 * launch, out[1] items served one by one through icp_create_device + icp_estimate_device (too large, handed back by
 * their workgroup, or no LDS grant), out[2] batch launches, out[3] launches not made because the runtime refused the
 * kernels their LDS (every item of those went one by one). */
int icp_batch_counters(icp_batch *b, uint64_t out[4]);
/* ... and of icp_batch_evaluate[_device] (icp_mi355x.h section 9): out[0] items served inside a batch launch, out[1]
 * items served one by one through icp_create_device + icp_evaluate_device, out[2] batch launches. */
int icp_batch_evaluate_counters(icp_batch *b, uint64_t out[3]);
/* ... and of icp_batch_estimate_point_to_line[_device] (icp_mi355x.h section 15): out[0] items served inside a batch
 * launch, out[1] items served one by one through icp_create_device + icp_compute_target_line_normals +
 * icp_estimate_point_to_line_device (outside the limits, handed back by their workgroup, or no LDS grant), out[2] batch
 * launches, out[3] launches not made because the runtime refused the kernels their LDS. */
int icp_batch_line_counters(icp_batch *b, uint64_t out[4]);
/* ... and of icp_batch_evaluate_point_to_line[_device] (icp_mi355x.h section 16): out[0] items served inside a batch
 * launch, out[1] items served one by one through icp_create_device + icp_compute_target_line_normals +
 * icp_evaluate_point_to_line_device (outside the limits, handed back by their workgroup, or no LDS grant), out[2] batch
 * launches, out[3] launches not made because the runtime refused the kernel its LDS. */
int icp_batch_line_quality_counters(icp_batch *b, uint64_t out[4]);
/* ... and of icp_batch_estimate_point_to_line_gated[_device] (icp_mi355x.h section 17): out[0] items served inside a
 * batch launch, out[1] items served one by one through icp_create_device + icp_compute_target_line_normals +
 * icp_estimate_point_to_line_gated_device (outside the limits, handed back by their workgroup, or no LDS grant), out[2]
 * batch launches, out[3] launches not made because the runtime refused the kernels their LDS. */
int icp_batch_line_gated_counters(icp_batch *b, uint64_t out[4]);
/* ... and of icp_batch_estimate_point_to_plane[_device] (icp_mi355x.h section 18): out[0] items served inside a batch
 * launch, out[1] items served one by one through icp_create_device + icp_compute_target_normals +
 * icp_estimate_point_to_plane_device (outside the limits, handed back by their workgroup, or no LDS grant), out[2] batch
 * launches, out[3] launches not made because the runtime refused the kernels their LDS. */
int icp_batch_plane_counters(icp_batch *b, uint64_t out[4]);
/* The LDS plan of a launch of section 18's kernel for workgroups of `threads` (512 or 1024)
 * threads whose items have at most m targets (1 .. 2048): out[0] targets whose neighbour lists one round of the normals
 * holds, out[1] bytes of the region the sort keys, the lists and the sort buffers use in turn, out[2] bytes beside it,
 * out[3] dynamic LDS of the launch (out[1] + out[2]).  Host arithmetic: no device use. */
int icp_debug_plane_batch_plan(unsigned threads, unsigned m, uint32_t out[4]);
/* ... and of icp_batch_estimate_point_to_plane_gated[_device] (icp_mi355x.h section 19): out[0] items served inside a
 * batch launch, out[1] items served one by one through icp_create_device + icp_compute_target_normals +
 * icp_estimate_point_to_plane_gated_device (outside the limits, handed back by their workgroup, or no LDS grant), out[2]
 * batch launches, out[3] launches not made because the runtime refused the kernels their LDS. */
int icp_batch_plane_gated_counters(icp_batch *b, uint64_t out[4]);
/* The LDS plan of a launch of section 19's kernel, laid out as icp_debug_plane_batch_plan's: the
 * same rounds of the normals (out[0]), and a shared region (out[1]) that also holds, behind the three sort buffers, one
 * 4-byte word per thread and sixteen wave counts for the gate.  Host arithmetic: no device use. */
int icp_debug_plane_gated_batch_plan(unsigned threads, unsigned m, uint32_t out[4]);
/* ... and of icp_batch_evaluate_point_to_plane[_device] (icp_mi355x.h section 20): out[0] items scored inside a batch
 * launch, out[1] items scored one by one through icp_create_device + icp_compute_target_normals +
 * icp_evaluate_point_to_plane_device (outside the limits, handed back by their workgroup, or no LDS grant), out[2] batch
 * launches, out[3] launches not made because the runtime refused the kernel its LDS. */
int icp_batch_plane_quality_counters(icp_batch *b, uint64_t out[4]);
/* The LDS plan of a launch of section 20's kernel, 1024 threads per workgroup, for items of at
 * most m targets (1 .. 2048), laid out as icp_debug_plane_batch_plan's: out[0] targets whose neighbour lists one round of
 * the normals holds, out[1] bytes of the region the sort keys, the lists and the fold use in turn, out[2] bytes beside it
 * (x | y | z, the screen records, the normals, 256 B of control words), out[3] dynamic LDS of the launch (out[1] +
 * out[2]).  Host arithmetic: no device use. */
int icp_debug_plane_quality_batch_plan(unsigned m, uint32_t out[4]);
/* ... and of icp_batch_estimate_gated[_device] (icp_mi355x.h section 21): out[0] items served inside a batch launch,
 * out[1] items served one by one through icp_create_device + icp_estimate_gated_device (outside the limits, handed back
 * by their workgroup, or no LDS grant), out[2] batch launches, out[3] launches not made because the runtime refused the
 * kernels their LDS.  Section 8's counters (icp_batch_counters) do not move with these calls. */
int icp_batch_gated_counters(icp_batch *b, uint64_t out[4]);
/* icp_remove_targets[_device] (icp_mi355x.h section 24): out[0] removals served by moving the search grid's sorted
 * records, out[1] removals that rebuilt the grid.  Its own pair: the crop's, the thin's and the outlier filters' pairs do
 * not move with it. */
int icp_grid_remove_counters(const icp_handle *h, uint64_t out[2]);
/* icp_query_neighbours* / icp_count_within* (section 24): out[0] calls whose lanes ran in cell order (the per-call sort;
 * for icp_count_within* without points, the targets' record order), out[1] calls served in the caller's order.  Calls
 * that launch nothing (n == 0, no output asked for) count in neither. */
int icp_query_counters(const icp_handle *h, uint64_t out[2]);
/* For measurements of the two orders: mode 0 = the library's threshold, 1 = cell order for every call the handle's sort
 * orders at all (more than 65 536 points), -1 = the caller's order.  Reset to 0 when the handle is destroyed. */
int icp_query_force_order(icp_handle *h, int mode);

/* Live kernel timing for the benchmark: with enable = k > 0, HIP events bracket every
 * k-th launch of the nearest-neighbour search kernel on the handle's stream (an event pair
 * costs a few us of stream time, so the benchmark samples instead of timing every launch);
 * 0 switches it off.  icp_profile_read synchronises the stream, returns the summed device
 * time (ms) of the timed launches and their count since the last read, and clears them. */
int icp_profile_enable(icp_handle *h, int enable);
int icp_profile_read(icp_handle *h, double *nn_kernel_ms, uint64_t *nn_kernel_launches);

#ifdef __cplusplus
}
#endif

#endif /* ICP_MI355X_DEBUG_H */
