// EXTENSION beyond the reference (include/icp_mi355x.h section 15): batched point-to-LINE registration, one workgroup per
// item.  Item i's result is what icp_create(2, dst_i) + icp_compute_target_line_normals(k) + icp_estimate_point_to_line
// return on a fresh handle, bit for bit (section 14; p2plane.hip, api_normal.hip: p2pl_loop_on_pairs), or the
// workgroup hands the item back (TinyResult::status = -1) and api_batch.hip serves it through exactly those entries.
// Nothing crosses workgroups: no flag, no atomic, no barrier across them.  What a workgroup does is
// normal_batch_device.hpp: normal_estimate_item<2, B, GATED>, the body the plane kernels (p2plane_batch.hip) run with
// DIM = 3; the pieces it has in common with the point kernels (gn_fast.hip, tiny_estimate_body.inc) are shared with them,
// each one copy in tiny_device.hpp.
//   box        fmin / fmax over its own targets (tiny_batch_box)
//   targets    sorted by fl32(x - cx) into LDS, with the f32 screen records (tiny_sort_targets)
//   normals    per target the k best by (d^2, index) from a sweep outwards over the sorted targets (exact: the k-nearest
//              set under that order is unique), lists in LDS for as many targets per round as the grant allows, then
//              line_normal_of_neighbours, the statement k_line_normals evaluates (normals_of_sorted_targets<2>, which
//              quality_line.hip's batch kernel calls too)
//   outer      transform, exact nearest neighbour (tiny_nearest: sweep and prune), the pair of k_line_gather
//   inner      plane_residual, exact median and MAD of r from one bitonic sort of the keys (tiny_bitonic_sort, ranks on the
//              sorted keys, as k_tiny_eval's sorting path), the 13 sums of k_p2pl_accumulate in the tree of
//              reduce_geometry(n) -- one or two blocks of 512 folded as block_reduce_store, then k_final_reduce's fold
//              over the blocks -- solve_update, the
//              three break tests in p2pl_loop_on_pairs' order, transform_new with the restated sin / cos
//              (tiny_inner_decide); the composed pose and the fixed-point test (tiny_outer_tail)
// Hand-back reasons: a box that is not finite; a NaN target coordinate; a rotation update outside the restated range of
// sin / cos.  A NaN residual is the item's ICP_NAN_INPUT.
// Section 17, k_line_estimate_gated_batch: the same body with the gate of icp_estimate_point_to_line_gated between the
// search and the inner loop -- the pairs with d2 <= r^2 (gate_plane.hip: k_lngate_stage's expressions), compacted in thread
// order (NormalGate<2, B>: the moved point and the position of its match), and p2pl_loop_on_pairs on the `kept` of them
// in the tree of reduce_geometry(kept).
// The LDS plan of a launch (DESIGN.md sections 9j and 9l): normal_estimate_plan<2, GATED>.
#include "normal_batch_device.hpp"

namespace icp {

template <unsigned B>
__global__ __launch_bounds__(B) void k_line_estimate_batch(const double *__restrict__ src_all,
                                                           const double *__restrict__ dst_all,
                                                           const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                           int kk, unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                           uint32_t *inner_all, uint32_t *idx_all) {
  normal_estimate_item<2, B, false>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all,
                                    0., nullptr);
}

// section 17: r2 = max_dist^2; inl_all: count x max_iter inlier counts, or null
template <unsigned B>
__global__ __launch_bounds__(B) void k_line_estimate_gated_batch(const double *__restrict__ src_all,
                                                                 const double *__restrict__ dst_all,
                                                                 const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                                 int kk, unsigned L, unsigned shared_bytes, double r2,
                                                                 TinyResult *res_all, uint32_t *inner_all,
                                                                 uint32_t *idx_all, uint32_t *inl_all) {
  normal_estimate_item<2, B, true>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all, r2,
                                   inl_all);
}

template <>
hipError_t launch_normal_estimate_batch<2, false>(unsigned threads, unsigned m_max, const double *d_src,
                                                  const double *d_dst, const TinyBatchItem *d_items, unsigned count,
                                                  unsigned max_iter, int k, double, TinyResult *res, uint32_t *inner,
                                                  uint32_t *d_idx, uint32_t *, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;
  const NormalPlan plan = normal_estimate_plan<2, false>(threads, m_max);
  return launch_one_workgroup_batch(grant, &k_line_estimate_batch<512>, &k_line_estimate_batch<1024>, threads, plan, count,
                                    stream, granted, d_src, d_dst, d_items, max_iter, k, plan.list_threads,
                                    plan.shared_bytes, res, inner, d_idx);
}

template <>
hipError_t launch_normal_estimate_batch<2, true>(unsigned threads, unsigned m_max, const double *d_src,
                                                 const double *d_dst, const TinyBatchItem *d_items, unsigned count,
                                                 unsigned max_iter, int k, double r2, TinyResult *res, uint32_t *inner,
                                                 uint32_t *d_idx, uint32_t *inliers, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;  // (these kernels' own)
  const NormalPlan plan = normal_estimate_plan<2, true>(threads, m_max);
  return launch_one_workgroup_batch(grant, &k_line_estimate_gated_batch<512>, &k_line_estimate_gated_batch<1024>, threads,
                                    plan, count, stream, granted, d_src, d_dst, d_items, max_iter, k, plan.list_threads,
                                    plan.shared_bytes, r2, res, inner, d_idx, inliers);
}

}  // namespace icp
