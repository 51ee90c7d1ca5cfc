// EXTENSION beyond the reference (include/icp_mi355x.h section 12): point-to-plane registration with a maximum
// correspondence distance.  The outer loop of icp_estimate_point_to_plane_device (api_ext.hip) in which the inner loop
// sees only the inlier pairs of the iteration's search -- d2 <= r * r, the rule icp_evaluate scores a pose by -- in the
// caller's order, the others removed (gate_plane.hip).  Per outer iteration: search -> gate (two launches and the wait
// that brings the count) -> the inner loop on the survivors -> compose.  Every entry decides on its arguments first, on
// the device next, and reads the handle only then.
#include "api_internal.hpp"

using namespace icp;
using namespace icp::api;

namespace {

// what icp_estimate_point_to_plane_device decides on the handle, in its order; *done: nothing to run, *out is set
int gated_plane_handle_ok(const icp_handle *h, size_t n, const icp_pose *init, size_t max_iter, icp_pose *out, bool *done) {
  *done = false;
  if (h->dim != 3) return ICP_BAD_ARGUMENT;
  if (h->m == 0) {  // index.unwrap() on an empty tree, src/lib.rs:165 -- only when a search would run
    if (n > 0 && max_iter > 0) return ICP_EMPTY_DST;
    *out = *init;
    *done = true;
    return ICP_OK;
  }
  if (h->normals_m != h->m) return ICP_BAD_ARGUMENT;  // icp_compute_target_normals first (again after an append)
  return ICP_OK;
}

int estimate_plane_gated(icp_handle *h, const double *d_src, size_t n, const Pose &init, size_t max_iter, double max_dist,
                         Pose *out, uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  ICP_TRY_RC(ensure_plane_buffers(h, n));
  ICP_TRY_RC(ensure_plane_stage(h, n));
  Workspace &w = h->ws;
  Pose T = init;
  if (max_iter > 0) ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &init));
  Quiesce quiesce_on_exit{h};
  for (size_t it = 0; it < max_iter; ++it) {
    uint32_t *idx = (it + 1 == max_iter && d_last_idx) ? d_last_idx : w.d_idx;
    ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, nullptr, nullptr, idx));  // exact 3-D NN, src/lib.rs:161-167
    Pose Ti;
    uint32_t applied = 0;
    size_t kept = 0;
    ICP_TRY_RC(icp_p2pl_gated_inner_loop_device(h, d_src, n, &T, idx, max_dist, &Ti, &applied, &kept));
    if (inner_iters) inner_iters[it] = applied;
    if (inliers) inliers[it] = (uint32_t)kept;
    T = transform_mul(Ti, T);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  *out = T;
  return ICP_OK;
}

}  // namespace

extern "C" int icp_estimate_point_to_plane_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                        size_t max_iter, double max_dist, icp_pose *out,
                                                        uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  if (!sized_args_ok(h, d_src, n, init, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  bool done;
  ICP_TRY_RC(gated_plane_handle_ok(h, n, init, max_iter, out, &done));
  if (done) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  return estimate_plane_gated(h, d_src, n, *init, max_iter, max_dist, out, d_last_idx, inner_iters, inliers);
}

extern "C" int icp_estimate_point_to_plane_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                                                 size_t max_iter, double max_dist, icp_pose *out, uint32_t *last_idx,
                                                 uint32_t *inner_iters, uint32_t *inliers) {
  if (!sized_args_ok(h, src, n, init, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  bool done;
  ICP_TRY_RC(gated_plane_handle_ok(h, n, init, max_iter, out, &done));
  if (done) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  if (n > 0) HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  uint32_t *d_li = nullptr;
  if (last_idx && n > 0) HIP_TRY(hipMalloc(&d_li, n * sizeof(uint32_t)));
  int rc = estimate_plane_gated(h, h->ws.d_src, n, *init, max_iter, max_dist, out, d_li, inner_iters, inliers);
  if (rc == ICP_OK && d_li && max_iter > 0) {
    if (hipMemcpy(last_idx, d_li, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = ICP_HIP_ERROR;
  }
  (void)hipFree(d_li);
  return rc;
}

extern "C" int icp_gate_plane_pairs_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                           const uint32_t *d_idx, double max_dist, double *d_pairs, uint32_t *d_kept,
                                           size_t *kept) {
  // (max_dist >= 0 is false for a NaN)
  if (!h || !T || !kept || (n > 0 && (!d_src || !d_idx || !d_pairs)) || !(max_dist >= 0.) || n >= 0xffffffffull)
    return ICP_BAD_ARGUMENT;
  *kept = 0;
  if (n == 0) return ICP_OK;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != 3) return ICP_BAD_ARGUMENT;
  if (h->m == 0) return ICP_EMPTY_DST;
  if (h->normals_m != h->m) return ICP_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  ICP_TRY_RC(ensure_plane_stage(h, n));
  HIP_TRY(launch_gate_plane(h, d_src, n, *T, d_idx, max_dist * max_dist, d_pairs, d_kept));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *kept = gate_count(h);
  return ICP_OK;
}
