// C ABI, EXTENSIONS beyond the reference: registration under a NORMAL residual n_q . (T p - q) -- point-to-plane on a 3-D
// handle (include/icp_mi355x.h sections 7 and 12), point-to-line on a 2-D one (section 14) -- with or without a maximum
// correspondence distance.  Not in the reference (no normals anywhere in src/); definitions: p2plane.hip, the CPU
// checkers under tests (tests/test_p2plane.py, tests/test_line_abi.py).  Everything around the residual is the
// reference's: the handle's exact nearest neighbour, the SE(2) pose on xy, Huber / MAD Gauss-Newton, the inner loop's
// break tests.  The targets' normals live in the handle's d_normals as m x 3 in both dimensions (a line normal with
// nz = +0.0), so that the append's invalidation and the crop's carry-over apply as they are.
// Per outer iteration: the search of icp_correspond_device -> the pairs (one gather; gated: two launches and the wait
// that brings the count, gate_plane.hip) -> the inner loop on them (p2pl_loop_on_pairs: host-stepped, five launches and
// a wait per evaluation) -> compose.  ONE body per step serves both dimensions and both gates; what an entry keeps of
// its own is the ORDER in which it decides (Order below; tests/test_*_abi.py pin it on a machine without a device).
#include <cfloat>

#include "api_internal.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace api {

// the per-pair scratch of an inner loop under a normal residual
int ensure_plane_buffers(icp_handle *h, size_t n) {
  if (n > h->cap_plane) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(h->d_plane_pairs);
    (void)hipFree(h->d_plane_fa);
    (void)hipFree(h->d_plane_fb);
    h->d_plane_pairs = nullptr;
    h->d_plane_fa = h->d_plane_fb = nullptr;
    h->cap_plane = 0;
    HIP_TRY(hipMalloc(&h->d_plane_pairs, n * p2pl_pair_bytes()));
    HIP_TRY(hipMalloc(&h->d_plane_fa, n * 2 * sizeof(double)));
    HIP_TRY(hipMalloc(&h->d_plane_fb, n * 2 * sizeof(double)));
    h->cap_plane = n;
  }
  return ICP_OK;
}

// ... and the staging buffer of its gate (gate_plane.hip: n pairs; only a gated call asks for it)
int ensure_plane_stage(icp_handle *h, size_t n) {
  if (n > h->cap_plane_stage) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(h->d_plane_stage);
    h->d_plane_stage = nullptr;
    h->cap_plane_stage = 0;
    HIP_TRY(hipMalloc(&h->d_plane_stage, n * p2pl_pair_bytes()));
    h->cap_plane_stage = n;
  }
  return ICP_OK;
}

// The inner loop (src/lib.rs:59-84 around the normal residual) on the k pairs in h->d_plane_pairs, whoever wrote them
// (the gather of all correspondences, or the gate's survivors): the pose update dT and the updates applied.  Fewer than
// two pairs: check_input_size -- the identity, no update.
int p2pl_loop_on_pairs(icp_handle *h, size_t k, Pose *dT, uint32_t *applied_out) {
  Workspace &w = h->ws;
  Pose Ti = transform_identity();
  uint32_t applied = 0;
  if (k >= 2) {
    double prev_error = DBL_MAX;
    for (int it = 0; it < ICP_INNER_MAX_ITER; ++it) {
      HIP_TRY(launch_p2pl_eval(h, h->d_plane_pairs, k, Ti, h->d_plane_fa, h->d_plane_fb));
      HIP_TRY(hipStreamSynchronize(h->stream));
      const GnResult &r = *w.h_res;
      if (r.nan_flag) {
        w.gn_dirty = true;  // (the flag stays in the selection scratch)
        return ICP_NAN_INPUT;
      }
      double delta[3];
      if (!solve_update(r.acc, r.acc + 9, delta)) break;
      if ((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2] < ICP_DELTA_NORM_THRESHOLD) break;
      if (r.acc[12] > prev_error) break;
      prev_error = r.acc[12];
      Ti = transform_mul(transform_new(delta), Ti);
      ++applied;
    }
  }
  *dT = Ti;
  if (applied_out) *applied_out = applied;
  return ICP_OK;
}

}  // namespace api
}  // namespace icp

namespace {

// The order in which an entry decides.  Section 7's entries (the normals and the ungated estimates of a 3-D handle, the
// oldest) test the handle's dimension with their arguments and never ask whether there is a device; icp_read_target_normals
// never asks for the dimension at all, and icp_estimate_point_to_plane sets the device and stages the cloud before the
// handle is looked at.  Every later entry goes arguments -> have_device() -> handle -> device.
enum class Order { Section7, ArgsDeviceHandle };

// the pairs of one outer iteration, enqueued: every correspondence (kept = n), or the gate's survivors and the wait that
// brings their number
int make_pairs(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx, bool gated,
               double max_dist, size_t *kept) {
  *kept = n;
  if (!gated) {
    HIP_TRY(launch_normal_gather(h, d_src, n, T, d_idx, h->d_normals, h->d_plane_pairs));
    return ICP_OK;
  }
  HIP_TRY(launch_gate_normal(h, d_src, n, T, d_idx, max_dist * max_dist, h->d_plane_pairs, nullptr));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *kept = gate_count(h);
  return ICP_OK;
}

// the scratch make_pairs and the loop behind it need (a gate's tile counts live in the per-point buffers: the floor)
int ensure_pair_scratch(icp_handle *h, size_t n, bool gated) {
  HIP_TRY(ensure_workspace(h, gated ? workspace_points(n) : n, false));
  ICP_TRY_RC(ensure_plane_buffers(h, n));
  if (gated) ICP_TRY_RC(ensure_plane_stage(h, n));
  return ICP_OK;
}

// what the normals entries share once each has decided on the handle's dimension (the normals are m x 3 either way)
int compute_normals(icp_handle *h, int k) {
  if (h->m == 0) return ICP_EMPTY_DST;
  if (!h->grid.built) return ICP_BAD_ARGUMENT;  // non-finite targets: no grid to search neighbourhoods with
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(reserve(h->d_normals, h->cap_normals, h->m * 3));
  HIP_TRY(launch_normals(h, k, h->d_normals, 0));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->normals_m = h->m;
  h->normals_k = k;
  return ICP_OK;
}

// The targets appended since the normals were last computed get theirs (from their k nearest targets in the cloud as it
// is NOW); the older targets keep the normals they have -- "normals at insertion time", the definition a map that grows
// frame by frame uses (a full compute re-derives all of them from the current cloud).
int update_normals(icp_handle *h, int k) {
  if (h->m == 0) return ICP_EMPTY_DST;
  if (!h->grid.built || h->normals_m > h->m) return ICP_BAD_ARGUMENT;
  if (h->normals_m > 0 && h->normals_k != k) return ICP_BAD_ARGUMENT;  // one neighbourhood size per cloud
  HIP_TRY(hipSetDevice(h->device));
  if (h->m * 3 > h->cap_normals || !h->d_normals) {  // grow, keeping the normals that exist
    double *old = h->d_normals;
    const size_t keep = h->normals_m * 3;
    h->d_normals = nullptr;
    h->cap_normals = 0;
    hipError_t e = reserve(h->d_normals, h->cap_normals, h->m * 3);
    if (e == hipSuccess && old && keep)
      e = hipMemcpyAsync(h->d_normals, old, keep * sizeof(double), hipMemcpyDeviceToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(old);
    if (e != hipSuccess) {
      h->normals_m = 0;
      return map_hip(e);
    }
  }
  HIP_TRY(launch_normals(h, k, h->d_normals, h->normals_m));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->normals_m = h->m;
  h->normals_k = k;
  return ICP_OK;
}

int normals_entry(icp_handle *h, int dim, Order order, int k, bool update) {
  if (!h || k < 3 || k > 16) return ICP_BAD_ARGUMENT;
  if (order != Order::Section7 && !have_device()) return ICP_NO_DEVICE;
  if (h->dim != dim) return ICP_BAD_ARGUMENT;
  return update ? update_normals(h, k) : compute_normals(h, k);
}

// `dim` doubles per target to out: (nx, ny, nz), or (nx, ny) of the stored (nx, ny, +0.0)
int read_normals_entry(icp_handle *h, int dim, Order order, size_t first, size_t count, double *out) {
  if (!h || (count > 0 && !out)) return ICP_BAD_ARGUMENT;
  if (order != Order::Section7 && !have_device()) return ICP_NO_DEVICE;
  if ((order != Order::Section7 && h->dim != dim) || h->normals_m != h->m || h->m == 0 || first > h->m ||
      count > h->m - first)
    return ICP_BAD_ARGUMENT;
  if (count == 0) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (dim == 3)
    HIP_TRY(hipMemcpyAsync(out, h->d_normals + first * 3, count * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  else  // a strided copy
    HIP_TRY(hipMemcpy2DAsync(out, 2 * sizeof(double), h->d_normals + first * 3, 3 * sizeof(double), 2 * sizeof(double),
                             count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ICP_OK;
}

// what the estimate entries decide on the handle; *done: nothing to run, *out is set
int handle_ok(const icp_handle *h, int dim, size_t n, const icp_pose *init, size_t max_iter, icp_pose *out, bool *done) {
  *done = false;
  if (h->dim != dim) return ICP_BAD_ARGUMENT;
  if (h->m == 0) {  // index.unwrap() on an empty tree, src/lib.rs:122 / :165 -- only when a search would run
    if (n > 0 && max_iter > 0) return ICP_EMPTY_DST;
    *out = *init;
    *done = true;
    return ICP_OK;
  }
  if (h->normals_m != h->m) return ICP_BAD_ARGUMENT;  // compute the normals first (again after an append)
  return ICP_OK;
}

// The outer loop.  gated: the inner loop sees the inliers of the iteration's search only (d2 <= max_dist^2, the rule
// icp_evaluate scores a pose by), in the caller's order; otherwise every pair.
int estimate_normal(icp_handle *h, const double *d_src, size_t n, const Pose &init, size_t max_iter, bool gated,
                    double max_dist, Pose *out, uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  ICP_TRY_RC(ensure_pair_scratch(h, n, gated));
  Workspace &w = h->ws;
  Pose T = init;
  if (max_iter > 0) ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &init));
  Quiesce quiesce_on_exit{h};
  for (size_t it = 0; it < max_iter; ++it) {
    uint32_t *idx = (it + 1 == max_iter && d_last_idx) ? d_last_idx : w.d_idx;
    ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, nullptr, nullptr, idx));  // exact NN, src/lib.rs:118-124, :161-167
    size_t kept;
    ICP_TRY_RC(make_pairs(h, d_src, n, T, idx, gated, max_dist, &kept));
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

// The entries that take a host cloud: staged through the handle's source buffer, the last indices through a temporary.
// Section 7's entry asks for n points and looks at the handle only now; the later ones have, and ask for the floor.
int estimate_normal_host(icp_handle *h, int dim, Order order, const double *src, size_t n, const icp_pose *init,
                         size_t max_iter, bool gated, double max_dist, icp_pose *out, uint32_t *last_idx,
                         uint32_t *inner_iters, uint32_t *inliers) {
  const bool s7 = order == Order::Section7;
  HIP_TRY(ensure_workspace(h, s7 ? n : workspace_points(n), true));
  if (n > 0) HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  uint32_t *d_li = nullptr;
  if (last_idx && n > 0) HIP_TRY(hipMalloc(&d_li, n * sizeof(uint32_t)));
  bool done = false;
  int rc = s7 ? handle_ok(h, dim, n, init, max_iter, out, &done) : ICP_OK;
  if (rc == ICP_OK && !done)
    rc = estimate_normal(h, h->ws.d_src, n, *init, max_iter, gated, max_dist, out, d_li, inner_iters, inliers);
  if (rc == ICP_OK && d_li && max_iter > 0) {
    if (hipMemcpy(last_idx, d_li, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = ICP_HIP_ERROR;
  }
  (void)hipFree(d_li);
  return rc;
}

// (an ungated entry passes max_dist = 0; max_dist >= 0 is false for a NaN)
int estimate_entry(icp_handle *h, int dim, Order order, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                   bool gated, double max_dist, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters,
                   uint32_t *inliers, bool on_device) {
  if (!sized_args_ok(h, src, n, init, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (order == Order::Section7) {
    if (h->dim != dim) return ICP_BAD_ARGUMENT;
    if (!on_device) {
      HIP_TRY(hipSetDevice(h->device));
      return estimate_normal_host(h, dim, order, src, n, init, max_iter, gated, max_dist, out, last_idx, inner_iters, inliers);
    }
  } else if (!have_device()) {
    return ICP_NO_DEVICE;
  }
  bool done;
  ICP_TRY_RC(handle_ok(h, dim, n, init, max_iter, out, &done));
  if (done) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  if (on_device) return estimate_normal(h, src, n, *init, max_iter, gated, max_dist, out, last_idx, inner_iters, inliers);
  return estimate_normal_host(h, dim, order, src, n, init, max_iter, gated, max_dist, out, last_idx, inner_iters, inliers);
}

}  // namespace

// One outer iteration's inner loop of a 3-D handle for given correspondences d_idx of the WHOLE source cloud under pose
// T: make the pairs, loop on them.  (icp_multi_estimate_point_to_plane[_gated] runs these on every rank after the ranks
// have exchanged the indices of their slices.)  Gated: the pairs of the inliers only, *kept their number.
static int p2pl_inner_loop(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                           bool gated, double max_dist, icp_pose *dT, uint32_t *applied_out, size_t *kept) {
  if (!h || h->dim != 3 || !T || !dT || (n > 0 && (!d_src || !d_idx)) || !(max_dist >= 0.) || h->normals_m != h->m ||
      h->m == 0)
    return ICP_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(h->device));
  ICP_TRY_RC(ensure_pair_scratch(h, n, gated));
  ICP_TRY_RC(make_pairs(h, d_src, n, *T, d_idx, gated, max_dist, kept));
  return p2pl_loop_on_pairs(h, *kept, dT, applied_out);
}
int icp_p2pl_inner_loop_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                               icp_pose *dT, uint32_t *applied_out) {
  size_t kept;
  return p2pl_inner_loop(h, d_src, n, T, d_idx, false, 0., dT, applied_out, &kept);
}
int icp_p2pl_gated_inner_loop_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, const uint32_t *d_idx,
                                     double max_dist, icp_pose *dT, uint32_t *applied_out, size_t *kept) {
  return kept ? p2pl_inner_loop(h, d_src, n, T, d_idx, true, max_dist, dT, applied_out, kept) : ICP_BAD_ARGUMENT;
}

// ---- section 7: the normals of a 3-D handle's targets
extern "C" int icp_compute_target_normals(icp_handle *h, int k) { return normals_entry(h, 3, Order::Section7, k, false); }
extern "C" int icp_update_target_normals(icp_handle *h, int k) { return normals_entry(h, 3, Order::Section7, k, true); }
extern "C" int icp_read_target_normals(icp_handle *h, size_t first, size_t count, double *out) {
  return read_normals_entry(h, 3, Order::Section7, first, count, out);
}
// ---- section 14: the line normals of a 2-D handle's targets
extern "C" int icp_compute_target_line_normals(icp_handle *h, int k) {
  return normals_entry(h, 2, Order::ArgsDeviceHandle, k, false);
}
extern "C" int icp_update_target_line_normals(icp_handle *h, int k) {
  return normals_entry(h, 2, Order::ArgsDeviceHandle, k, true);
}
extern "C" int icp_read_target_line_normals(icp_handle *h, size_t first, size_t count, double *out) {
  return read_normals_entry(h, 2, Order::ArgsDeviceHandle, first, count, out);
}

// ---- sections 7 and 12: point-to-plane
extern "C" int icp_estimate_point_to_plane(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                                           size_t max_iter, icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters) {
  return estimate_entry(h, 3, Order::Section7, src, n, init, max_iter, false, 0., out, last_idx, inner_iters, nullptr, false);
}
extern "C" int icp_estimate_point_to_plane_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                  size_t max_iter, icp_pose *out, uint32_t *d_last_idx,
                                                  uint32_t *inner_iters) {
  return estimate_entry(h, 3, Order::Section7, d_src, n, init, max_iter, false, 0., out, d_last_idx, inner_iters, nullptr,
                        true);
}
extern "C" int icp_estimate_point_to_plane_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                                                 size_t max_iter, double max_dist, icp_pose *out, uint32_t *last_idx,
                                                 uint32_t *inner_iters, uint32_t *inliers) {
  return estimate_entry(h, 3, Order::ArgsDeviceHandle, src, n, init, max_iter, true, max_dist, out, last_idx, inner_iters,
                        inliers, false);
}
extern "C" int icp_estimate_point_to_plane_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                        size_t max_iter, double max_dist, icp_pose *out,
                                                        uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  return estimate_entry(h, 3, Order::ArgsDeviceHandle, d_src, n, init, max_iter, true, max_dist, out, d_last_idx,
                        inner_iters, inliers, true);
}

// ---- section 14: point-to-line
extern "C" int icp_estimate_point_to_line(icp_handle *h, const double *src, size_t n, const icp_pose *init, size_t max_iter,
                                          icp_pose *out, uint32_t *last_idx, uint32_t *inner_iters) {
  return estimate_entry(h, 2, Order::ArgsDeviceHandle, src, n, init, max_iter, false, 0., out, last_idx, inner_iters,
                        nullptr, false);
}
extern "C" int icp_estimate_point_to_line_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                 size_t max_iter, icp_pose *out, uint32_t *d_last_idx,
                                                 uint32_t *inner_iters) {
  return estimate_entry(h, 2, Order::ArgsDeviceHandle, d_src, n, init, max_iter, false, 0., out, d_last_idx, inner_iters,
                        nullptr, true);
}
extern "C" int icp_estimate_point_to_line_gated(icp_handle *h, const double *src, size_t n, const icp_pose *init,
                                                size_t max_iter, double max_dist, icp_pose *out, uint32_t *last_idx,
                                                uint32_t *inner_iters, uint32_t *inliers) {
  return estimate_entry(h, 2, Order::ArgsDeviceHandle, src, n, init, max_iter, true, max_dist, out, last_idx, inner_iters,
                        inliers, false);
}
extern "C" int icp_estimate_point_to_line_gated_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *init,
                                                       size_t max_iter, double max_dist, icp_pose *out,
                                                       uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  return estimate_entry(h, 2, Order::ArgsDeviceHandle, d_src, n, init, max_iter, true, max_dist, out, d_last_idx,
                        inner_iters, inliers, true);
}

// ---- section 12: the gate alone
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
  HIP_TRY(launch_gate_normal(h, d_src, n, *T, d_idx, max_dist * max_dist, d_pairs, d_kept));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *kept = gate_count(h);
  return ICP_OK;
}
