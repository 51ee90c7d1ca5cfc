// EXTENSION beyond the reference (include/icp_mi355x.h section 10): registration with a maximum correspondence
// distance.  The outer loop of Icp{2,3}d::estimate (src/lib.rs:105-130, 148-173) in which estimate_transform
// (src/lib.rs:59-84) sees only the inlier pairs of the iteration's search -- d2 <= r * r, the rule icp_evaluate scores
// a pose by -- in fold order, the others removed (gate.hip).  Per outer iteration: search -> gate (two launches and
// the wait that brings the count) -> the inner loop on the survivors -> compose.  The next pose's pairs are not known
// before its gate has run, so there is no bet and no run-ahead search here: those belong to icp_estimate_device.
#include <cstring>

#include "api_internal.hpp"

using namespace icp;
using namespace icp::api;

namespace {

int estimate_gated(icp_handle *h, const double *d_src, size_t n, const Pose &init, size_t max_iter, double max_dist,
                   Pose *out, uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  // Whatever way this call ends, nothing of it is in flight afterwards and its search snapshot is dropped
  // (icp_estimate_device's discipline: the snapshot is keyed on a buffer the caller may now rewrite).
  Quiesce quiesce_on_exit{h};
  Workspace &w = h->ws;
  h->qsort.fold_n = 0;  // (identity, until this call takes a snapshot)
  Pose T = init;
  if (max_iter > 0) ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &init));
  // the fold order of icp_estimate_device: beyond kGridCoopMaxN points on the grid engine the call lives in the
  // snapshot's order (searches emit slot k at k, the gate reads the sorted copy), else in the caller's
  const bool slot = h->qsort.valid && h->qsort.src == d_src && h->qsort.n == n && (long)n > kGridCoopMaxN;
  h->qsort.slot_order = slot;
  if (slot) h->qsort.fold_n = n;
  const double *gate_src = slot ? h->qsort.d_sorted : d_src;
  uint32_t *const idx = slot ? w.d_idx_slot : (d_last_idx ? d_last_idx : w.d_idx);
  const double r2 = max_dist * max_dist;
  for (size_t it = 0; it < max_iter; ++it) {
    ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, w.d_a, w.d_b, idx));
    HIP_TRY(launch_gate(h, gate_src, n, T, idx, r2, w.d_a2, w.d_b2, nullptr));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t kept = gate_count(h);
    if (inliers) inliers[it] = (uint32_t)kept;
    Pose dT;
    uint32_t inner = 0;
    // (fewer than two survivors: check_input_size -- the identity, no update)
    ICP_TRY_RC(estimate_transform_on_pairs(h, w.d_a2, w.d_b2, kept, &dT, &inner, it == 0 ? 3 : 0, it == 0 ? 4 : 1));
    if (inner_iters) inner_iters[it] = inner;
    const Pose T_next = transform_mul(dT, T);  // src/lib.rs:127, 170
    // a fixed point of the loop (icp_estimate_device): the iterations behind it would repeat it -- same pose, same
    // pairs, same count; only the last one still runs (it reports the correspondences)
    if (h->fixed_point_exit && inner == 0 && it + 2 < max_iter && memcmp(&T_next, &T, sizeof(Pose)) == 0) {
      for (size_t k = it + 1; k + 1 < max_iter; ++k) {
        if (inner_iters) inner_iters[k] = 0;
        if (inliers) inliers[k] = (uint32_t)kept;
      }
      w.fixed_point_skips += max_iter - 2 - it;
      it = max_iter - 2;
    }
    T = T_next;
  }
  if (slot && d_last_idx && max_iter > 0 && n > 0) HIP_TRY(launch_unpermute_idx(h, w.d_idx_slot, n, d_last_idx));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *out = T;
  return ICP_OK;
}

}  // namespace

extern "C" int icp_estimate_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                         size_t max_iter, double max_dist, icp_pose *out, uint32_t *d_last_idx,
                                         uint32_t *inner_iters, uint32_t *inliers) {
  if (!sized_args_ok(h, d_src, n, init, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  HIP_TRY(hipSetDevice(h->device));
  return estimate_gated(h, d_src, n, *init, max_iter, max_dist, out, d_last_idx, inner_iters, inliers);
}

extern "C" int icp_estimate_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                                  double max_dist, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters,
                                  uint32_t *inliers) {
  if (!sized_args_ok(h, src, n, init, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * h->dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ICP_TRY_RC(estimate_gated(h, h->ws.d_src, n, *init, max_iter, max_dist, out, last_idx ? h->ws.d_idx : nullptr,
                            inner_iters, inliers));
  if (last_idx && n > 0 && max_iter > 0) {
    HIP_TRY(hipMemcpyAsync(last_idx, h->ws.d_idx, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return ICP_OK;
}
