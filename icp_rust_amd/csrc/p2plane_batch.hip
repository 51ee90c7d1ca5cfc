// EXTENSION beyond the reference (include/icp_mi355x.h section 18): batched point-to-PLANE registration, one workgroup per
// 3-D item.  Item i's result is what icp_create(3, dst_i) + icp_compute_target_normals(k) + icp_estimate_point_to_plane
// return on a fresh handle, bit for bit (p2plane.hip's header comment and api_normal.hip: p2pl_loop_on_pairs are the
// definition), or the workgroup hands the item back (TinyResult::status = -1) and api_batch.hip serves it through exactly
// those entries.  Nothing crosses workgroups: no flag, no atomic, no barrier across them; every loop has a static bound
// (the rounds of the normals, jacobi3's 12 sweeps, ICP_INNER_MAX_ITER, max_iter).  What a workgroup does is
// normal_batch_device.hpp: normal_estimate_item<3, B, GATED>, the body the line kernels (p2line_batch.hip) run with
// DIM = 2, each piece the one copy the other one-workgroup kernels run too:
//   box        fmin / fmax over its own targets (tiny_batch_box<3>)
//   targets    sorted by fl32(x - cx) into LDS, x | y | z with the f32 screen records (tiny_sort_targets<3>)
//   normals    per target the k best by (d^2, index), d^2 = (dx dx + dy dy) + dz dz, from a sweep outwards over the sorted
//              targets (tiny_k_best_of_target<3>), lists in LDS for as many targets per round as the grant allows, then
//              plane_normal_of_neighbours, the statement k_target_normals evaluates (normals_of_sorted_targets<3>, which
//              quality_plane_batch.hip: k_plane_quality_batch runs too)
//   outer      transform xy with z carried, exact nearest neighbour (tiny_nearest<3>, warm), the pair of k_p2pl_gather
//   inner      tiny_pair_loop (pair_loop_device.hpp): plane_residual, exact median and MAD, k_p2pl_accumulate's 13 sums in
//              the tree of reduce_geometry(n), solve_update and the break tests; then tiny_outer_tail
// Hand-back reasons: a box that is not finite; a NaN target coordinate; a rotation update outside the restated range of
// sin / cos.  A NaN residual is the item's ICP_NAN_INPUT.
// Section 19, k_plane_estimate_gated_batch: the same body with the gate of icp_estimate_point_to_plane_gated between the
// search and the inner loop -- the pairs with d2 <= r^2 (gate_plane.hip: k_plgate_stage's expressions, d2 = (ex ex + ey
// ey) + dz dz), compacted in thread order (NormalGate<3, B>: one word per kept pair), and p2pl_loop_on_pairs on the
// `kept` of them in the tree of reduce_geometry(kept).
// The LDS plan of a launch (DESIGN.md sections 9m and 9n): normal_estimate_plan<3, GATED>.
#include "normal_batch_device.hpp"

namespace icp {

template <unsigned B>
__global__ __launch_bounds__(B) void k_plane_estimate_batch(const double *__restrict__ src_all,
                                                            const double *__restrict__ dst_all,
                                                            const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                            int kk, unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                            uint32_t *inner_all, uint32_t *idx_all) {
  normal_estimate_item<3, B, false>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all,
                                    0., nullptr);
}

// section 19: r2 = max_dist^2; inl_all: count x max_iter inlier counts, or null
template <unsigned B>
__global__ __launch_bounds__(B) void k_plane_estimate_gated_batch(const double *__restrict__ src_all,
                                                                  const double *__restrict__ dst_all,
                                                                  const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                                  int kk, unsigned L, unsigned shared_bytes, double r2,
                                                                  TinyResult *res_all, uint32_t *inner_all,
                                                                  uint32_t *idx_all, uint32_t *inl_all) {
  normal_estimate_item<3, B, true>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all, r2,
                                   inl_all);
}

template <>
hipError_t launch_normal_estimate_batch<3, false>(unsigned threads, unsigned m_max, const double *d_src,
                                                  const double *d_dst, const TinyBatchItem *d_items, unsigned count,
                                                  unsigned max_iter, int k, double, TinyResult *res, uint32_t *inner,
                                                  uint32_t *d_idx, uint32_t *, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;
  const NormalPlan plan = normal_estimate_plan<3, false>(threads, m_max);
  return launch_one_workgroup_batch(grant, &k_plane_estimate_batch<512>, &k_plane_estimate_batch<1024>, threads, plan,
                                    count, stream, granted, d_src, d_dst, d_items, max_iter, k, plan.list_threads,
                                    plan.shared_bytes, res, inner, d_idx);
}

template <>
hipError_t launch_normal_estimate_batch<3, true>(unsigned threads, unsigned m_max, const double *d_src,
                                                 const double *d_dst, const TinyBatchItem *d_items, unsigned count,
                                                 unsigned max_iter, int k, double r2, TinyResult *res, uint32_t *inner,
                                                 uint32_t *d_idx, uint32_t *inliers, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;  // (these kernels' own)
  const NormalPlan plan = normal_estimate_plan<3, true>(threads, m_max);
  return launch_one_workgroup_batch(grant, &k_plane_estimate_gated_batch<512>, &k_plane_estimate_gated_batch<1024>, threads,
                                    plan, count, stream, granted, d_src, d_dst, d_items, max_iter, k, plan.list_threads,
                                    plan.shared_bytes, r2, res, inner, d_idx, inliers);
}

}  // namespace icp
