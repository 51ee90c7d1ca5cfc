// What the translation units of the C ABI share (api.hip: handles, stage calls, the loops of Icp::estimate; api_shard.hip:
// the sharded registration; api_ext.hip, api_normal.hip and the others: the extensions beyond the reference).  Internal:
// nothing here is exported (csrc/exports.map).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "common.hpp"
#include "gn_loop.hpp"

#define HIP_TRY(expr)                                      \
  do {                                                     \
    hipError_t e__ = (expr);                               \
    if (e__ != hipSuccess) return ::icp::api::map_hip(e__); \
  } while (0)
#define ICP_TRY_RC(expr)             \
  do {                               \
    const int rc__ = (expr);         \
    if (rc__ != ICP_OK) return rc__; \
  } while (0)

namespace icp {
namespace api {

int map_hip(hipError_t e);
// the host's wait for a result block (polls its sequence number, then the stream the work was enqueued on)
hipError_t wait_seq(icp_handle *h, volatile unsigned *seq, unsigned want, hipStream_t stream = nullptr);
hipError_t wait_result(icp_handle *h, hipStream_t stream = nullptr);
// weighted_gauss_newton_update + huber_error on device pairs through whatever pipeline serves (api.hip: wgn_step)
int wgn_step(icp_handle *h, const double *d_a, const double *d_b, size_t n, const Pose &T, double delta[3], double *huber_err,
             bool pre_launched = false, int kind = 2);
int resolved_nn_mode(const icp_handle *h);
// check_input_size, src/lib.rs:186-189
inline bool input_size_ok(size_t n) { return n > 0 && n >= 2; }

// ---- what the entries of the extensions share (each entry keeps its own ORDER of decisions: tests/test_*_abi.py) ----
// is there a device to run on (ICP_NO_DEVICE otherwise)
inline bool have_device() {
  int count = 0;
  return hipGetDeviceCount(&count) == hipSuccess && count > 0;
}
// the arguments of an entry that takes a cloud of n points, a pose and a distance (max_dist >= 0 is false for a NaN)
inline bool sized_args_ok(const icp_handle *h, const void *src, size_t n, const icp_pose *pose, double max_dist,
                          const void *out) {
  return h && pose && out && (n == 0 || src) && max_dist >= 0. && n < 0xffffffffull;
}
// points to ask ensure_workspace for: the scratch of a gate or an evaluation (tile counts, level records) lives in the
// per-point buffers and needs 256 points' worth even for the smallest cloud
inline size_t workspace_points(size_t n) { return n < 256 ? 256 : n; }
// n and zeros: what the *out of an evaluation (icp_quality, icp_plane_quality, icp_line_quality) holds unless a result
// replaces it
template <typename Q>
void quality_clear(size_t n, Q *q) {
  std::memset(q, 0, sizeof(*q));
  q->n = n;
}
// Whatever way the call that holds it ends, nothing of it is in flight on h->stream afterwards, and the search snapshot
// it may have taken (the cell-sorted copy, keyed on a buffer the caller may now rewrite) is dropped, as
// icp_estimate_device drops its own.  slot_order is cleared for icp_estimate_gated_device, the one holder that sets it;
// for the others it is already false: only that entry and icp_estimate_device set it, each behind its guard, which
// clears it on every exit.
struct Quiesce {
  icp_handle *h;
  ~Quiesce() {
    (void)hipStreamSynchronize(h->stream);
    h->qsort.valid = false;
    h->qsort.have_prev = false;
    h->qsort.slot_order = false;
  }
};
// what the next evaluation's window is centred on: this evaluation's exact median and sigma (api.hip)
void record_statistics(Workspace &w, int kind, bool has_median, const GnResult &r);

// ---- the one-launch inner loop (gn_loop.hip), host side ----
// What a launch of the device-resident loop is planned with, and what its result is read against: the window
// predictions for its first two evaluations (taken from the handle's per-kind history, common.hpp: Workspace::win_kind).
struct LoopPlan {
  LoopArgs A;
  int first_kind = 0, second_kind = 1, it0 = 0;
  bool own0 = false;
  double p_med[2][2], p_sigma[2][2];
  int kind_of(int i) const { return i == 0 ? first_kind : (i == 1 ? second_kind : 2); }
};
bool loop_plan(icp_handle *h, size_t n, int it, int first_kind, int second_kind, bool hints, LoopPlan *pl);
int loop_finish(icp_handle *h, const LoopPlan &pl, const LoopResult *res, Pose *T, double *prev_error, uint32_t *applied,
                int *it, bool *finished);
hipError_t ensure_loop(icp_handle *h);
void loop_timed_out(Workspace &w);
void free_loop_inbox(Workspace &w);  // (api_shard.hip)
void free_loop_plan(void *p);

// estimate_transform (src/lib.rs:59-84) on device pairs as the library's own loops run it (api.hip:
// estimate_transform_loop, everything on h->stream, no hook); first_kind / second_kind name the window predictions of
// its first two evaluations (common.hpp: Workspace::win_kind)
int estimate_transform_on_pairs(icp_handle *h, const double *d_a, const double *d_b, size_t n, Pose *out,
                                uint32_t *inner_iters, int first_kind, int second_kind);
// the gate of a registration with a maximum correspondence distance (gate.hip): enqueues the stable compaction of the
// pairs with d2 <= r2 on h->stream; gate_count is the survivors' number once that stream has been waited for
hipError_t launch_gate(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx, double r2,
                       double *d_a, double *d_b, uint32_t *d_kept);
size_t gate_count(const icp_handle *h);
// ... of a registration under a normal residual (gate_plane.hip): the same compaction, fused with what the gather of the
// handle's dimension does -- the survivors' PlanePairs (8 doubles each; dz = nz = 0 on a 2-D handle) in d_pairs, their
// source positions in d_kept (nullable); the count as above.  Needs ensure_workspace(max(n, 256)), ensure_plane_stage(n)
// and current normals.
hipError_t launch_gate_normal(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx, double r2,
                              void *d_pairs, uint32_t *d_kept);
// the per-pair scratch of an inner loop under a normal residual, and the staging buffer of its gate (api_normal.hip)
int ensure_plane_buffers(icp_handle *h, size_t n);
int ensure_plane_stage(icp_handle *h, size_t n);
// the inner loop (src/lib.rs:59-84 around the plane residual) on the k pairs in h->d_plane_pairs (api_normal.hip)
int p2pl_loop_on_pairs(icp_handle *h, size_t k, Pose *dT, uint32_t *applied_out);

// ---- removing targets from a handle (crop.hip): the half icp_crop_targets and icp_thin_targets (voxel.hip) share ----
// a removed target's mark, and its entry of the new_index table
constexpr uint32_t kCropGone = 0xffffffffu;
// Waits for everything in flight on the handle, then hands out the device words a keep rule fills for the h->m > 0
// targets: *w, one mark per target (0 or kCropGone), and *cnt, the kept targets of every tile of kCompactTile
// consecutive ones (the words behind them are remove_marked_targets' own).  Both are build temporaries of the grid.
int target_marks(icp_handle *h, uint32_t **w, uint32_t **cnt);
// Everything a removal does behind its mark launch (enqueued on h->stream, marks from target_marks): the chunk sums, the
// "nothing to remove" exit, the kept points and normals into the second buffers, new_index (nullable, host), the grid's
// records moved (++moved) or the grid rebuilt (++rebuilt), the brute engine's arrays, the swap and the way back.
int remove_marked_targets(icp_handle *h, uint32_t *w, uint32_t *cnt, unsigned long long &moved,
                          unsigned long long &rebuilt, uint32_t *new_index, size_t *removed);
// the cached workspace of icp_voxel_downsample* and icp_thin_targets (voxel.hip), for icp_trim_pool
void voxel_trim();
// ... of icp_target_neighbours and the two outlier filters (outlier.hip)
void outlier_trim();
// ... of the query entries and icp_remove_targets (query.hip)
void query_trim();

}  // namespace api
}  // namespace icp
// One outer iteration's point-to-plane inner loop for given correspondences of the whole source cloud (api_normal.hip), and
// the same on the inliers of a gate at max_dist (*kept: their number)
int icp_p2pl_inner_loop_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                               icp_pose *dT, uint32_t *applied_out);
int icp_p2pl_gated_inner_loop_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                                     double max_dist, icp_pose *dT, uint32_t *applied_out, size_t *kept);
