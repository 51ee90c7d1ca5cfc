// C ABI, EXTENSION beyond the reference (include/icp_mi355x.h section 14): point-to-line registration for 2-D handles --
// the line normals of the targets (kept in the handle's d_normals at a stride of 3 with nz = +0.0, so that the append's
// invalidation and the crop's carry-over of section 7's normals apply as they are) and the outer loop of
// icp_estimate_point_to_plane[_gated]_device around them.  Per outer iteration: the handle's exact 2-D search -> the
// pairs (one gather; gated: two launches and the wait that brings the count, p2line.hip) -> section 7's inner loop on
// them (p2pl_loop_on_pairs: host-stepped, five launches and a wait per evaluation) -> compose.  Every entry decides on its
// arguments first, on the device next, and reads the handle only then.
#include "api_internal.hpp"

using namespace icp;
using namespace icp::api;

namespace {

// what the estimate entries decide on the handle, in section 7's order; *done: nothing to run, *out is set
int line_handle_ok(const icp_handle *h, size_t n, const icp_pose *init, size_t max_iter, icp_pose *out, bool *done) {
  *done = false;
  if (h->dim != 2) return ICP_BAD_ARGUMENT;
  if (h->m == 0) {  // index.unwrap() on an empty tree, src/lib.rs:122 -- only when a search would run
    if (n > 0 && max_iter > 0) return ICP_EMPTY_DST;
    *out = *init;
    *done = true;
    return ICP_OK;
  }
  if (h->normals_m != h->m) return ICP_BAD_ARGUMENT;  // icp_compute_target_line_normals first (again after an append)
  return ICP_OK;
}

// gated: the inner loop sees the inliers of the iteration's search only (d2 <= max_dist^2); otherwise every pair
int estimate_line(icp_handle *h, const double *d_src, size_t n, const Pose &init, size_t max_iter, bool gated,
                  double max_dist, Pose *out, uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  HIP_TRY(ensure_workspace(h, gated ? workspace_points(n) : n, false));
  ICP_TRY_RC(ensure_plane_buffers(h, n));
  if (gated) ICP_TRY_RC(ensure_plane_stage(h, n));
  Workspace &w = h->ws;
  Pose T = init;
  if (max_iter > 0) ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &init));
  Quiesce quiesce_on_exit{h};
  for (size_t it = 0; it < max_iter; ++it) {
    uint32_t *idx = (it + 1 == max_iter && d_last_idx) ? d_last_idx : w.d_idx;
    ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, nullptr, nullptr, idx));  // exact 2-D NN, src/lib.rs:118-124
    size_t kept = n;
    if (gated) {
      HIP_TRY(launch_gate_line(h, d_src, n, T, idx, max_dist * max_dist, h->d_plane_pairs, nullptr));
      HIP_TRY(hipStreamSynchronize(h->stream));
      kept = gate_count(h);
    } else {
      HIP_TRY(launch_line_gather(h, d_src, n, T, idx, h->d_normals, h->d_plane_pairs));
    }
    Pose Ti;
    uint32_t applied = 0;
    ICP_TRY_RC(p2pl_loop_on_pairs(h, kept, &Ti, &applied));
    if (inner_iters) inner_iters[it] = applied;
    if (inliers) inliers[it] = (uint32_t)kept;
    T = transform_mul(Ti, T);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  *out = T;
  return ICP_OK;
}

// the entries that take a host cloud: staged through the handle's source buffer, the last indices through a temporary
int estimate_line_host(icp_handle *h, const double *src, size_t n, const Pose &init, size_t max_iter, bool gated,
                       double max_dist, Pose *out, uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  if (n > 0) HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  uint32_t *d_li = nullptr;
  if (last_idx && n > 0) HIP_TRY(hipMalloc(&d_li, n * sizeof(uint32_t)));
  int rc = estimate_line(h, h->ws.d_src, n, init, max_iter, gated, max_dist, out, d_li, inner_iters, inliers);
  if (rc == ICP_OK && d_li && max_iter > 0) {
    if (hipMemcpy(last_idx, d_li, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = ICP_HIP_ERROR;
  }
  (void)hipFree(d_li);
  return rc;
}

// (an ungated entry passes max_dist = 0; max_dist >= 0 is false for a NaN)
int line_entry(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter, bool gated, double max_dist,
               icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers, bool on_device) {
  if (!sized_args_ok(h, src, n, init, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  bool done;
  ICP_TRY_RC(line_handle_ok(h, n, init, max_iter, out, &done));
  if (done) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  return on_device ? estimate_line(h, src, n, *init, max_iter, gated, max_dist, out, last_idx, inner_iters, inliers)
                   : estimate_line_host(h, src, n, *init, max_iter, gated, max_dist, out, last_idx, inner_iters, inliers);
}

bool normals_args_ok(const icp_handle *h, int k) { return h && k >= 3 && k <= 16; }

}  // namespace

extern "C" int icp_compute_target_line_normals(icp_handle *h, int k) {
  if (!normals_args_ok(h, k)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != 2) return ICP_BAD_ARGUMENT;
  return compute_normals_with(h, k, launch_line_normals);
}

// The targets appended since the normals were last computed get theirs (from their k nearest targets in the cloud as it
// is NOW); the older targets keep the normals they have, as icp_update_target_normals keeps a 3-D handle's.
extern "C" int icp_update_target_line_normals(icp_handle *h, int k) {
  if (!normals_args_ok(h, k)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != 2) return ICP_BAD_ARGUMENT;
  return update_normals_with(h, k, launch_line_normals);
}

extern "C" int icp_read_target_line_normals(icp_handle *h, size_t first, size_t count, double *out) {
  if (!h || (count > 0 && !out)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != 2 || h->normals_m != h->m || h->m == 0 || first > h->m || count > h->m - first) return ICP_BAD_ARGUMENT;
  if (count == 0) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  // (nx, ny) of the stored (nx, ny, +0.0): a strided copy
  HIP_TRY(hipMemcpy2DAsync(out, 2 * sizeof(double), h->d_normals + first * 3, 3 * sizeof(double), 2 * sizeof(double), count,
                           hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ICP_OK;
}

extern "C" int icp_estimate_point_to_line(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                                          icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters) {
  return line_entry(h, src, n, init, max_iter, false, 0., out, last_idx, inner_iters, nullptr, false);
}

extern "C" int icp_estimate_point_to_line_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                 size_t max_iter, icp_pose *out, uint32_t *d_last_idx,
                                                 uint32_t *inner_iters) {
  return line_entry(h, d_src, n, init, max_iter, false, 0., out, d_last_idx, inner_iters, nullptr, true);
}

extern "C" int icp_estimate_point_to_line_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                                                size_t max_iter, double max_dist, icp_pose *out, uint32_t *last_idx,
                                                uint32_t *inner_iters, uint32_t *inliers) {
  return line_entry(h, src, n, init, max_iter, true, max_dist, out, last_idx, inner_iters, inliers, false);
}

extern "C" int icp_estimate_point_to_line_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                       size_t max_iter, double max_dist, icp_pose *out,
                                                       uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  return line_entry(h, d_src, n, init, max_iter, true, max_dist, out, d_last_idx, inner_iters, inliers, true);
}
