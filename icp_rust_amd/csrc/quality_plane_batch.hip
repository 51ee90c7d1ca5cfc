// EXTENSION beyond the reference (include/icp_mi355x.h section 20): the quality of many poses under the point-to-PLANE
// residual of section 13, one workgroup per 3-D item.  Item i's record is what icp_create(3, dst_i) +
// icp_compute_target_normals(k) + icp_evaluate_point_to_plane(src_i, T_i, max_dist) fold on a fresh handle, bit for bit,
// or the workgroup hands the item back (its record is left alone) and api_batch.hip serves it through exactly those
// entries.  Nothing crosses workgroups: no flag, no atomic; every loop has a static bound.
//   k_plane_quality_batch  the item's box (tiny_batch_box<3>), its targets sorted into LDS (tiny_sort_targets<3>), their
//                          plane normals (the rounds k_plane_estimate_batch runs), the exact nearest neighbour of every
//                          moved source point from a cold start (tiny_nearest<3>), the ten terms of section 13
//                          (normal_quality_terms<3>) and the tree of a batch item (fold_workgroup); its body is
//                          normal_batch_device.hpp: normal_quality_item<3>, which k_line_quality_batch (quality_line.hip)
//                          runs in two dimensions, its LDS plan normal_quality_plan<3>: none of
//                          the estimator's wave sums, totals, PairCtl and sort buffers are in it
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.
#include "normal_batch_device.hpp"

namespace icp {

__global__ __launch_bounds__(kNormalQualityThreads) void k_plane_quality_batch(const double *__restrict__ src_all,
                                                                               const double *__restrict__ dst_all,
                                                                               const QualityBatchItem *__restrict__ items,
                                                                               double r2, int kk, unsigned L,
                                                                               unsigned shared_bytes,
                                                                               NormalQualityPart *__restrict__ res) {
  normal_quality_item<3>(src_all, dst_all, items, r2, kk, L, shared_bytes, res);
}

template <>
hipError_t launch_normal_quality_batch<3>(unsigned m_max, const double *d_src, const double *d_dst,
                                          const QualityBatchItem *d_items, unsigned count, double r2, int k,
                                          NormalQualityPart *res, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;
  const NormalPlan plan = normal_quality_plan<3>(m_max);
  return launch_one_workgroup_batch(grant, &k_plane_quality_batch, &k_plane_quality_batch, kNormalQualityThreads, plan,
                                    count, stream, granted, d_src, d_dst, d_items, r2, k, plan.list_threads,
                                    plan.shared_bytes, res);
}

// The fields of section 13 from the root record, on the host (the batch's; the single calls form them with the same
// function, quality_plane.hip: same bits).
int plane_quality_result(size_t n, const NormalQualityPart &p, icp_plane_quality *q) {
  return normal_quality_result(n, p, q, &icp_plane_quality::plane_sum_r2, &icp_plane_quality::plane_rmse);
}

}  // namespace icp
