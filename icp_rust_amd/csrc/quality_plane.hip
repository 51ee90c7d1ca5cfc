// EXTENSION beyond the reference (include/icp_mi355x.h section 13): the quality of a pose under the point-to-plane
// residual -- fitness, inlier RMSE, plane RMSE, error / huber_error of the plane residual and the SE(2) information
// matrix that residual gives (the jtj of k_p2pl_accumulate at the identity inner pose, unweighted, on the inlier pairs),
// at a GIVEN pose, with the handle's own exact search and its normals.
//   k_plane_quality_terms  one workgroup per 256 source points: a lane gathers src[i], idx[i], dst[j], nrm[j] once
//                          (76 B), forms the ten terms of section 13, and the group folds them by the tree of section 9
//                          (fold_device.hpp) into one 96-byte record; its body is normal_quality_level1<3>
//   k_fold_level<10>       the next level of the same tree: one workgroup per 256 records (as many launches as levels)
// Every sum is the fixed tree, so a result is a pure function of the inputs.  The terms, the level-1 body, the single
// calls' driver, the entries' decisions and the result's fields are the ones section 16 (quality_line.hip) uses too:
// quality_device.hpp.
#include "quality_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

__global__ __launch_bounds__(256) void k_plane_quality_terms(const double *__restrict__ src, unsigned n, Pose T,
                                                             const uint32_t *__restrict__ idx,
                                                             const double *__restrict__ dst,
                                                             const double *__restrict__ nrm, unsigned m, double r2,
                                                             NormalQualityPart *__restrict__ out) {
  normal_quality_level1<3>(src, n, T, idx, dst, nrm, m, r2, out);
}

}  // namespace icp

namespace {

// The device part of both entries: the handle's exact 3-D search at T, then the terms and the tree.
int plane_evaluate(icp_handle *h, const double *d_src, size_t n, const Pose &T, double max_dist, icp_plane_quality *out,
                   uint32_t *d_idx) {
  const double r2 = max_dist * max_dist;
  NormalQualityPart r;
  ICP_TRY_RC(evaluate_on_handle(h, d_src, n, T, d_idx, false, [&](const uint32_t *idx, unsigned k, NormalQualityPart *cur) {
    hipLaunchKernelGGL(k_plane_quality_terms, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                       (const double *)h->d_normals, (unsigned)h->m, r2, cur);
  }, &r));
  return normal_quality_result(n, r, out, &icp_plane_quality::plane_sum_r2, &icp_plane_quality::plane_rmse);
}

}  // namespace

extern "C" int icp_evaluate_point_to_plane_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                                  double max_dist, icp_plane_quality *out, uint32_t *d_idx) {
  bool done;
  const int rc = normal_evaluate_enter(h, d_src, n, T, max_dist, out, 3, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return plane_evaluate(h, d_src, n, *T, max_dist, out, d_idx);
}

extern "C" int icp_evaluate_point_to_plane(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                                           icp_plane_quality *out, uint32_t *idx) {
  bool done;
  const int rc = normal_evaluate_enter(h, src, n, T, max_dist, out, 3, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return evaluate_staged(h, src, n, idx, [&](const double *d_src, uint32_t *d_idx) {
    return plane_evaluate(h, d_src, n, *T, max_dist, out, d_idx);
  });
}
