// What the three pose qualities share above the fold tree (fold_device.hpp): point (quality.hip, include/icp_mi355x.h
// section 9), point-to-plane (quality_plane.hip, section 13) and point-to-line (quality_line.hip, section 16).
//   device  normal_quality_terms<DIM>   the ten terms of a normal-based residual (plane: DIM 3, line: DIM 2)
//           quality_level1              the body of a single call's first launch, around a point's terms
//           normal_quality_level1<DIM>  ... with normal_quality_terms: k_plane_quality_terms and k_line_quality_terms
//   host    evaluate_on_handle          the single calls' driver: search, level 1, the levels above, the root record
//           evaluate_staged             the host entries around it: the cloud staged, the indices read back
//           normal_evaluate_enter       what the plane and line entries decide before any work
//           quality_head, normal_quality_result   a result's fields from the root record
// The kernels themselves stay in their own files (each its own translation unit, names and signatures as they were);
// each entry keeps its own order of decisions (tests/test_*_abi.py).
#pragma once
#include <cmath>
#include <cstring>

#include "api_internal.hpp"
#include "fold_device.hpp"
#include "gn_device.hpp"

namespace icp {

// A point's terms under a normal-based residual (the library is built with -ffp-contract=off: no FMA).  q is the moved
// source point (its third coordinate is the source's own: the pose is SE(2)), b the matched target, nrm its unit normal;
// DIM == 2 reads two of each.  DIM == 3 (section 13): d2 is section 9's, rp is plane_residual (p2plane_device.hpp) at the
// identity inner pose.  DIM == 2 (section 16): the 2-D icp_evaluate's d2; plane_residual would add a trailing + nz dz =
// + 0.0 to rp; the square does not see it (it only turns a -0.0 into +0.0), so it is left out here.
template <int DIM>
__device__ __forceinline__ void normal_quality_terms(const double *q, const double *b, const double *nrm, double r2,
                                                     double (&v)[kNormalQualitySums], unsigned &in, unsigned &nan) {
  const double qx = q[0], qy = q[1], nx = nrm[0], ny = nrm[1];
  const double ex = qx - b[0], ey = qy - b[1];
  double d2 = ex * ex + ey * ey;
  double rp = nx * ex + ny * ey;
  if (DIM == 3) {
    const double dz = q[2] - b[2];
    d2 = d2 + dz * dz;
    rp = rp + nrm[2] * dz;
  }
  const bool inl = d2 <= r2;  // (false for a NaN d2)
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

// Level 1 of a single call, one workgroup of kFoldGroup threads: the terms of source points [256 g, 256 g + 256), folded
// -> out[g].  terms(q, j, v, in, nan) forms the terms of the moved point q = (qx, qy, pz) matched to target j.  n == 1:
// out[0] is the one point's terms (the fold of one value is the value: no +0.0 added, a -0.0 stays).
template <int DIM, int SUMS, typename Terms>
__device__ __forceinline__ void quality_level1(const double *__restrict__ src, unsigned n, const Pose &T,
                                               const uint32_t *__restrict__ idx, unsigned m,
                                               FoldPart<SUMS> *__restrict__ out, Terms terms) {
  __shared__ FoldLds<SUMS> L;
  const unsigned tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kFoldGroup + tid;
  double v[SUMS] = {};
  unsigned in = 0, nan = 0;
  if (i < n) {
    const double px = src[i * DIM], py = src[i * DIM + 1];
    const double pz = DIM == 3 ? src[i * DIM + 2] : 0.;
    const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (T.r10 * px + T.r11 * py) + T.ty;
    uint32_t j = idx[i];
    if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the reads in bounds)
    const double q[3] = {qx, qy, pz};
    terms(q, j, v, in, nan);
  }
  if (n == 1) {
    if (tid == 0) out[0] = fold_part(v, in, nan);
    return;
  }
  fold_put(L, tid, v, in, nan);
  fold_group(L, tid);
  if (tid == 0) out[blockIdx.x] = fold_take(L);
}

// ... for a normal-based residual: a lane gathers src[i], idx[i], dst[j], nrm[j] once.  dst at a stride of DIM; the
// normals at the stride of 3 they are stored with (a 2-D handle's nz = +0.0 is there and is not read).
template <int DIM>
__device__ __forceinline__ void normal_quality_level1(const double *__restrict__ src, unsigned n, const Pose &T,
                                                      const uint32_t *__restrict__ idx, const double *__restrict__ dst,
                                                      const double *__restrict__ nrm, unsigned m, double r2,
                                                      NormalQualityPart *__restrict__ out) {
  quality_level1<DIM>(src, n, T, idx, m, out,
                      [=](const double *q, uint32_t j, double (&v)[kNormalQualitySums], unsigned &in, unsigned &nan) {
                        normal_quality_terms<DIM>(q, dst + (size_t)j * DIM, nrm + (size_t)j * 3, r2, v, in, nan);
                      });
}

namespace api {

// The device part of every single call: the handle's exact search at T, then launch_level1(idx, k, cur) -- the entry's
// own kernel over k = ceil(n / 256) workgroups, one record each into cur -- the levels above it and the root record in
// *root.  want_pairs: the search also materialises the pairs (section 9's entries ask for them; the others do not).
template <int SUMS, typename Launch>
int evaluate_on_handle(icp_handle *h, const double *d_src, size_t n, const Pose &T, uint32_t *d_idx, bool want_pairs,
                       Launch launch_level1, FoldPart<SUMS> *root) {
  // the level records live in the residual buffers: ceil(n / 256) records fit in max(n, 256) doubles
  static_assert(sizeof(FoldPart<SUMS>) <= kFoldGroup * sizeof(double), "a record per 256 points, in a double per point");
  Quiesce quiesce_on_exit{h};
  Workspace &w = h->ws;
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  uint32_t *idx = d_idx ? d_idx : w.d_idx;
  ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &T));
  ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, want_pairs ? w.d_a : nullptr, want_pairs ? w.d_b : nullptr, idx));
  const unsigned k = (unsigned)((n + kFoldGroup - 1) / kFoldGroup);
  FoldPart<SUMS> *cur = reinterpret_cast<FoldPart<SUMS> *>(w.d_rx), *nxt = reinterpret_cast<FoldPart<SUMS> *>(w.d_ry);
  launch_level1(idx, k, cur);
  HIP_TRY(hipGetLastError());
  FoldPart<SUMS> *d_root;
  HIP_TRY(fold_levels(cur, nxt, k, h->stream, &d_root));
  HIP_TRY(hipMemcpyAsync(root, d_root, sizeof(*root), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ICP_OK;
}

// A host entry around its device part: the cloud staged in the workspace, evaluate(d_src, d_idx), and the
// correspondences read back into idx (nullable) where the search ran.
template <typename Evaluate>
int evaluate_staged(icp_handle *h, const double *src, size_t n, uint32_t *idx, Evaluate evaluate) {
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * h->dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int rc = evaluate(h->ws.d_src, h->ws.d_idx);
  if ((rc == ICP_OK || rc == ICP_NAN_INPUT) && idx) {  // (the search ran: its correspondences are there either way)
    HIP_TRY(hipMemcpyAsync(idx, h->ws.d_idx, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return rc;
}

// What the entries of sections 13 and 16 decide before any work, in the order those sections give: the arguments,
// n == 0, the device, and only then the handle (need_dim: 3 for planes, 2 for lines; normals_m: the normals of
// icp_compute_target_normals / icp_compute_target_line_normals must be current, again after an append).  *done: the
// status is final.
template <typename Q>
int normal_evaluate_enter(icp_handle *h, const void *src, size_t n, const icp_pose *T, double max_dist, Q *out,
                          int need_dim, bool *done) {
  *done = true;
  if (out) quality_clear(n, out);
  if (!sized_args_ok(h, src, n, T, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (n == 0) return ICP_OK;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != need_dim || h->normals_m != h->m) return ICP_BAD_ARGUMENT;
  if (h->m == 0) return ICP_EMPTY_DST;
  *done = false;
  return ICP_OK;
}

}  // namespace api

// The fields every quality shares, from the root record on the host (its first sum is the inliers' d2): *q is n and zeros
// first.  false: *rc is the result -- ICP_OK for n == 0, ICP_NAN_INPUT where the record carries the flag (src/stats.rs:12's
// rule and the estimators': a NaN residual); true: the residual's own fields follow.
template <typename Q, int SUMS>
bool quality_head(size_t n, const FoldPart<SUMS> &p, Q *q, int *rc) {
  api::quality_clear(n, q);
  *rc = (n > 0 && p.nan) ? ICP_NAN_INPUT : ICP_OK;
  if (n == 0 || p.nan) return false;
  q->inliers = p.inliers;
  q->fitness = (double)p.inliers / (double)n;
  q->inlier_sum_d2 = p.v[0];
  q->inlier_rmse = p.inliers ? std::sqrt(p.v[0] / (double)p.inliers) : 0.;
  return true;
}

// The fields of sections 13 and 16 (icp_plane_quality and icp_line_quality: one layout, two names for the residual's sum
// and RMSE) from the root record, on the host: every entry and the batch share it, same bits.
template <typename Q>
int normal_quality_result(size_t n, const NormalQualityPart &p, Q *q, double Q::*sum_r2, double Q::*rmse) {
  int rc;
  if (!quality_head(n, p, q, &rc)) return rc;
  q->*sum_r2 = p.v[1];
  q->*rmse = p.inliers ? std::sqrt(p.v[1] / (double)p.inliers) : 0.;
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

}  // namespace icp
