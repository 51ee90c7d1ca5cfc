// EXTENSION beyond the reference (include/icp_mi355x.h section 13): the quality of a pose under the point-to-plane
// residual -- fitness, inlier RMSE, plane RMSE, error / huber_error of the plane residual and the SE(2) information
// matrix that residual gives (the jtj of k_p2pl_accumulate at the identity inner pose, unweighted, on the inlier pairs),
// at a GIVEN pose, with the handle's own exact search and its normals.
//   k_plane_quality_terms  one workgroup per 256 source points: a lane gathers src[i], idx[i], dst[j], nrm[j] once
//                          (76 B), forms the ten terms of section 13, and the group folds them by the tree of section 9
//                          (fold_device.hpp) into one 96-byte record
//   k_fold_level<10>       the next level of the same tree: one workgroup per 256 records (as many launches as levels)
// Every sum is the fixed tree, so a result is a pure function of the inputs.
#include <cmath>
#include <cstring>

#include "api_internal.hpp"
#include "fold_device.hpp"
#include "gn_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace {

constexpr int kPlaneSums = 10;  // S_d2, S_p2, E, H, Ixx, Ixy, Iyy, Ixt, Iyt, Itt
using PlaneQualityPart = FoldPart<kPlaneSums>;
static_assert(sizeof(PlaneQualityPart) == 96, "twelve doubles per record: ceil(n / 256) of them fit in max(n, 256)");

}  // namespace

// level 1: the terms of source points [256 g, 256 g + 256), folded -> out[g].  n == 1: out[0] is the one point's terms
// (the fold of one value is the value: no +0.0 added, a -0.0 stays).  The library is built with -ffp-contract=off: no
// FMA in any expression below.
__global__ __launch_bounds__(256) void k_plane_quality_terms(const double *__restrict__ src, unsigned n, Pose T,
                                                             const uint32_t *__restrict__ idx,
                                                             const double *__restrict__ dst,
                                                             const double *__restrict__ nrm, unsigned m, double r2,
                                                             PlaneQualityPart *__restrict__ out) {
  __shared__ FoldLds<kPlaneSums> L;
  const unsigned tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kFoldGroup + tid;
  double v[kPlaneSums] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (i < n) {
    const double px = src[i * 3], py = src[i * 3 + 1], pz = src[i * 3 + 2];
    const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (T.r10 * px + T.r11 * py) + T.ty;
    uint32_t j = idx[i];
    if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the reads in bounds)
    const double *b = dst + (size_t)j * 3, *nj = nrm + (size_t)j * 3;
    const double nx = nj[0], ny = nj[1], nz = nj[2];
    const double ex = qx - b[0], ey = qy - b[1], dz = pz - b[2];
    const double d2 = (ex * ex + ey * ey) + dz * dz;  // section 9's d2
    const bool inl = d2 <= r2;                        // (false for a NaN d2)
    const double rp = (nx * ex + ny * ey) + nz * dz;  // plane_residual (p2plane_device.hpp) at the identity inner pose
    const double p2 = rp * rp;
    const double c = nx * (-qy) + ny * qx;  // J[2] of k_p2pl_accumulate at identity, a = q; J[0] = nx, J[1] = ny
    v[0] = inl ? d2 : 0.;
    v[1] = inl ? p2 : 0.;
    v[2] = p2;
    v[3] = huber_rho(p2);
    v[4] = inl ? nx * nx : 0.;
    v[5] = inl ? nx * ny : 0.;
    v[6] = inl ? ny * ny : 0.;
    v[7] = inl ? nx * c : 0.;
    v[8] = inl ? ny * c : 0.;
    v[9] = inl ? c * c : 0.;
    in = inl ? 1u : 0u;
    nan = (p2 != p2) ? 1u : 0u;
  }
  if (n == 1) {
    if (tid == 0) out[0] = fold_part(v, in, nan);
    return;
  }
  fold_put(L, tid, v, in, nan);
  fold_group(L, tid);
  if (tid == 0) out[blockIdx.x] = fold_take(L);
}

}  // namespace icp

namespace {

// n and zeros: what *out holds unless a result replaces it
void plane_quality_clear(size_t n, icp_plane_quality *q) {
  std::memset(q, 0, sizeof(*q));
  q->n = n;
}

// The fields of section 13 from the root record, on the host (both entries share it: same bits).
int plane_quality_result(size_t n, const PlaneQualityPart &p, icp_plane_quality *q) {
  plane_quality_clear(n, q);
  if (n == 0) return ICP_OK;
  if (p.nan) return ICP_NAN_INPUT;  // (the estimator's rule: a NaN residual)
  q->inliers = p.inliers;
  q->fitness = (double)p.inliers / (double)n;
  q->inlier_sum_d2 = p.v[0];
  q->inlier_rmse = p.inliers ? std::sqrt(p.v[0] / (double)p.inliers) : 0.;
  q->plane_sum_r2 = p.v[1];
  q->plane_rmse = p.inliers ? std::sqrt(p.v[1] / (double)p.inliers) : 0.;
  q->error = p.v[2];
  q->huber_error = p.v[3];
  const double ixx = p.v[4], ixy = p.v[5], iyy = p.v[6], ixt = p.v[7], iyt = p.v[8], itt = p.v[9];
  const double info[9] = {ixx, ixy, ixt, ixy, iyy, iyt, ixt, iyt, itt};
  std::memcpy(q->information, info, sizeof(info));
  // the eigenvalues of the translation block with + - * sqrt only (host code is built without FMA contraction too)
  const double h = (ixx + iyy) * 0.5;
  const double g = (ixx - iyy) * 0.5;
  const double s = std::sqrt(g * g + ixy * ixy);
  q->translation_eig[0] = h - s;
  q->translation_eig[1] = h + s;
  return ICP_OK;
}

// What both entries decide before any work, in the order section 13 gives: the arguments, n == 0, the device, and only
// then the handle.  *done: the status is final.
int plane_evaluate_enter(icp_handle *h, const void *src, size_t n, const icp_pose *T, double max_dist,
                         icp_plane_quality *out, bool *done) {
  *done = true;
  if (out) plane_quality_clear(n, out);
  if (!sized_args_ok(h, src, n, T, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (n == 0) return ICP_OK;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != 3 || h->normals_m != h->m) return ICP_BAD_ARGUMENT;  // icp_compute_target_normals first (again after an append)
  if (h->m == 0) return ICP_EMPTY_DST;
  *done = false;
  return ICP_OK;
}

// The device part of both entries: the handle's search at T, then the terms and the tree.
int plane_evaluate(icp_handle *h, const double *d_src, size_t n, const Pose &T, double max_dist, icp_plane_quality *out,
                   uint32_t *d_idx) {
  Quiesce quiesce_on_exit{h};
  Workspace &w = h->ws;
  // (the level records live in the residual buffers: ceil(n / 256) records of 12 doubles fit in max(n, 256) doubles)
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  uint32_t *idx = d_idx ? d_idx : w.d_idx;
  ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &T));
  ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, nullptr, nullptr, idx));  // exact 3-D NN
  const double r2 = max_dist * max_dist;
  const unsigned k = (unsigned)((n + kFoldGroup - 1) / kFoldGroup);
  PlaneQualityPart *cur = reinterpret_cast<PlaneQualityPart *>(w.d_rx), *nxt = reinterpret_cast<PlaneQualityPart *>(w.d_ry);
  hipLaunchKernelGGL(k_plane_quality_terms, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                     (const double *)h->d_normals, (unsigned)h->m, r2, cur);
  HIP_TRY(hipGetLastError());
  PlaneQualityPart r, *root;
  HIP_TRY(fold_levels(cur, nxt, k, h->stream, &root));
  HIP_TRY(hipMemcpyAsync(&r, root, sizeof(r), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return plane_quality_result(n, r, out);
}

}  // namespace

extern "C" int icp_evaluate_point_to_plane_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                                  double max_dist, icp_plane_quality *out, uint32_t *d_idx) {
  bool done;
  const int rc = plane_evaluate_enter(h, d_src, n, T, max_dist, out, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return plane_evaluate(h, d_src, n, *T, max_dist, out, d_idx);
}

extern "C" int icp_evaluate_point_to_plane(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                                           icp_plane_quality *out, uint32_t *idx) {
  bool done;
  const int erc = plane_evaluate_enter(h, src, n, T, max_dist, out, &done);
  if (done) return erc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int rc = plane_evaluate(h, h->ws.d_src, n, *T, max_dist, out, h->ws.d_idx);
  if ((rc == ICP_OK || rc == ICP_NAN_INPUT) && idx) {  // (the search ran: its correspondences are there either way)
    HIP_TRY(hipMemcpyAsync(idx, h->ws.d_idx, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return rc;
}
