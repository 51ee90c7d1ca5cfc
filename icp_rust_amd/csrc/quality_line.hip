// EXTENSION beyond the reference (include/icp_mi355x.h section 16): the quality of a pose under the point-to-LINE
// residual of section 14 -- fitness, inlier RMSE, line RMSE, error / huber_error of the line residual and the SE(2)
// information matrix that residual gives -- at a GIVEN pose, for a 2-D handle with current line normals, as a single
// call and as a batch.  Section 13 (quality_plane.hip) with the third coordinate removed: the terms, the level-1 body,
// the single calls' driver, the entries' decisions and the result's fields are written once for both, in
// quality_device.hpp.
//   k_line_quality_terms  one workgroup per 256 source points: a lane gathers src[i], idx[i], dst[j], nrm[j] once (52 B),
//                         forms the ten terms of section 16, and the group folds them by the tree of section 9
//                         (fold_device.hpp) into one 96-byte record; its body is normal_quality_level1<2>
//   k_fold_level<10>      the next level of the same tree: one workgroup per 256 records (as many launches as levels)
//   k_line_quality_batch  one workgroup per item of icp_batch_evaluate_point_to_line: the item's box, its targets sorted
//                         into LDS, their line normals (the sweep k_line_estimate_batch runs), the exact nearest
//                         neighbour of every moved source point (tiny_nearest), the same terms and the tree of a batch
//                         item, fold_workgroup, as k_quality_batch folds it (api_batch.hip drives it); its body is
//                         normal_batch_device.hpp: normal_quality_item<2>, its LDS plan
//                         normal_quality_plan<2>
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.
#include "normal_batch_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

__global__ __launch_bounds__(256) void k_line_quality_terms(const double *__restrict__ src, unsigned n, Pose T,
                                                            const uint32_t *__restrict__ idx,
                                                            const double *__restrict__ dst,
                                                            const double *__restrict__ nrm, unsigned m, double r2,
                                                            LineQualityPart *__restrict__ out) {
  normal_quality_level1<2>(src, n, T, idx, dst, nrm, m, r2, out);
}

__global__ __launch_bounds__(kNormalQualityThreads) void k_line_quality_batch(const double *__restrict__ src_all,
                                                                              const double *__restrict__ dst_all,
                                                                              const QualityBatchItem *__restrict__ items,
                                                                              double r2, int kk, unsigned L,
                                                                              unsigned shared_bytes,
                                                                              LineQualityPart *__restrict__ res) {
  normal_quality_item<2>(src_all, dst_all, items, r2, kk, L, shared_bytes, res);
}

template <>
hipError_t launch_normal_quality_batch<2>(unsigned m_max, const double *d_src, const double *d_dst,
                                          const QualityBatchItem *d_items, unsigned count, double r2, int k,
                                          NormalQualityPart *res, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;
  const NormalPlan plan = normal_quality_plan<2>(m_max);
  return launch_one_workgroup_batch(grant, &k_line_quality_batch, &k_line_quality_batch, kNormalQualityThreads, plan, count,
                                    stream, granted, d_src, d_dst, d_items, r2, k, plan.list_threads, plan.shared_bytes,
                                    res);
}

// The fields of section 16 from the root record, on the host (both entries and the batch share it: same bits).
int line_quality_result(size_t n, const LineQualityPart &p, icp_line_quality *q) {
  return normal_quality_result(n, p, q, &icp_line_quality::line_sum_r2, &icp_line_quality::line_rmse);
}

}  // namespace icp

namespace {

// The device part of both entries: the handle's exact 2-D search at T, then the terms and the tree.
int line_evaluate(icp_handle *h, const double *d_src, size_t n, const Pose &T, double max_dist, icp_line_quality *out,
                  uint32_t *d_idx) {
  const double r2 = max_dist * max_dist;
  LineQualityPart r;
  ICP_TRY_RC(evaluate_on_handle(h, d_src, n, T, d_idx, false, [&](const uint32_t *idx, unsigned k, LineQualityPart *cur) {
    hipLaunchKernelGGL(k_line_quality_terms, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                       (const double *)h->d_normals, (unsigned)h->m, r2, cur);
  }, &r));
  return line_quality_result(n, r, out);
}

}  // namespace

extern "C" int icp_evaluate_point_to_line_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                                 double max_dist, icp_line_quality *out, uint32_t *d_idx) {
  bool done;
  const int rc = normal_evaluate_enter(h, d_src, n, T, max_dist, out, 2, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return line_evaluate(h, d_src, n, *T, max_dist, out, d_idx);
}

extern "C" int icp_evaluate_point_to_line(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                                          icp_line_quality *out, uint32_t *idx) {
  bool done;
  const int rc = normal_evaluate_enter(h, src, n, T, max_dist, out, 2, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return evaluate_staged(h, src, n, idx, [&](const double *d_src, uint32_t *d_idx) {
    return line_evaluate(h, d_src, n, *T, max_dist, out, d_idx);
  });
}
