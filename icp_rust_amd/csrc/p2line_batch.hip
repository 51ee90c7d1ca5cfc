// EXTENSION beyond the reference (include/icp_mi355x.h section 15): batched point-to-LINE registration, one workgroup per
// item.  Item i's result is what icp_create(2, dst_i) + icp_compute_target_line_normals(k) + icp_estimate_point_to_line
// return on a fresh handle, bit for bit (section 14; p2line.hip, p2plane.hip, api_ext.hip: p2pl_loop_on_pairs), or the
// workgroup hands the item back (TinyResult::status = -1) and api_batch.hip serves it through exactly those entries.
// Nothing crosses workgroups: no flag, no atomic, no barrier across them.  What a workgroup does:
// The pieces it has in common with the point kernels (gn_fast.hip, tiny_estimate_body.inc) are shared with them, each
// one copy in tiny_device.hpp.
//   box        fmin / fmax over its own targets (tiny_batch_box)
//   targets    sorted by fl32(x - cx) into LDS, with the f32 screen records (tiny_sort_targets)
//   normals    per target the k best by (d^2, index) from a sweep outwards over the sorted targets (exact: the k-nearest
//              set under that order is unique), lists in LDS for as many targets per round as the grant allows, then
//              line_normal_of_neighbours, the statement k_line_normals evaluates (p2line_device.hpp:
//              line_normals_of_sorted_targets, which quality_line.hip's batch kernel calls too)
//   outer      transform, exact nearest neighbour (tiny_nearest: sweep and prune), the pair of k_line_gather
//   inner      plane_residual, exact median and MAD of r from one bitonic sort of the keys (tiny_bitonic_sort, ranks on the
//              sorted keys, as k_tiny_eval's sorting path), the 13 sums of k_p2pl_accumulate in the tree of
//              reduce_geometry(n) -- one or two blocks of 512 folded as block_reduce_store, then k_final_reduce's fold
//              over the blocks -- solve_update, the
//              three break tests in p2pl_loop_on_pairs' order, transform_new with the restated sin / cos
//              (tiny_inner_decide); the composed pose and the fixed-point test (tiny_outer_tail)
// Hand-back reasons: a box that is not finite; a NaN target coordinate; a rotation update outside the restated range of
// sin / cos.  A NaN residual is the item's ICP_NAN_INPUT.
// Section 17, k_line_estimate_gated_batch: the same body (line_estimate_item) with the gate of
// icp_estimate_point_to_line_gated between the search and the inner loop -- the pairs with d2 <= r^2 (p2line.hip:
// k_lngate_stage's expressions), compacted in thread order, and p2pl_loop_on_pairs on the `kept` of them in the tree of
// reduce_geometry(kept).
#include "common.hpp"
#include "gn_device.hpp"
#include "p2line_device.hpp"
#include "p2plane_device.hpp"
#include "pair_loop_device.hpp"
#include "tiny_device.hpp"

namespace icp {

constexpr int kLineSums = kPairSums;  // (the sums and the control block of the inner loop: pair_loop_device.hpp)
using LineCtl = PairCtl;

// ---- the LDS plan of a launch ----
// per workgroup, for its item's m targets (mp = m rounded up to 64): x | y (f64), the f32 screen records (+ 4 pads), the
// normals; then ONE shared region, sized by the launch; then the wave sums, the totals and LineCtl.  The shared region
// holds, one after the other: the target sort's keys (8 B x the next power of two of m), the k-best lists of the
// normals ((8 + 4) B x 16 per list-holding thread), the estimator's two sort buffers and sorted keys (3 x 8 B x B).
// Per-thread lists for every thread do not fit beside 2048 targets, so the normals run in rounds of `list_threads`
// targets: as many as the grant leaves room for, up to one per thread and per target.
constexpr size_t kLineListBytes = kLineKMax * (sizeof(double) + sizeof(uint32_t));
constexpr size_t line_fixed_bytes(unsigned m) {
  const size_t mp = (m + 63u) & ~63u;
  return mp * 2 * sizeof(double) + (mp + 4) * sizeof(float4) + mp * sizeof(double2) + sizeof(double) * 16 * kLineSums +
         sizeof(double) * 16 + 256;
}
static_assert(sizeof(LineCtl) <= 256, "LineCtl's share of the LDS");
static_assert(line_fixed_bytes(kLineBatchMaxM) + 3 * 1024 * 8 <= kTinyLdsGrant &&
                  (kTinyLdsGrant - line_fixed_bytes(kLineBatchMaxM)) / kLineListBytes >= 256,
              "2048 targets leave room for the sort buffers and for at least 256 lists");
struct LinePlan {
  unsigned list_threads, shared_bytes;
  size_t lds_bytes;
};
constexpr LinePlan line_batch_plan(unsigned threads, unsigned m_max) {
  const size_t fixed = line_fixed_bytes(m_max);
  size_t keys = 64;
  while (keys < m_max) keys <<= 1;
  const size_t fit = (kTinyLdsGrant - fixed) / kLineListBytes / 64 * 64;
  size_t lists = (m_max + 63u) & ~63u;  // (a list per target is all a round can use)
  lists = lists < threads ? lists : threads;
  lists = lists < fit ? lists : fit;
  size_t shared = lists * kLineListBytes;
  shared = shared > keys * 8 ? shared : keys * 8;
  shared = shared > (size_t)3 * threads * 8 ? shared : (size_t)3 * threads * 8;
  return LinePlan{(unsigned)lists, (unsigned)shared, fixed + shared};
}
// the plan at its corners: the smallest item, a golden scan (two rounds of 640), the largest item (rounds of 320)
static_assert(line_batch_plan(512, 1).list_threads == 64 && line_batch_plan(512, 1).shared_bytes == 3 * 512 * 8, "m = 1");
static_assert(line_batch_plan(1024, 668).list_threads == 640 && line_batch_plan(1024, 668).lds_bytes == 158784, "m = 668");
static_assert(line_batch_plan(512, kLineBatchMaxM).list_threads == 320 && line_batch_plan(1024, kLineBatchMaxM).list_threads == 320 &&
                  line_batch_plan(1024, kLineBatchMaxM).lds_bytes == 161856 &&
                  line_batch_plan(1024, kLineBatchMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048");

// ---- the gate's words (section 17) ----
// Behind the estimator's three sort buffers in the shared region, which the normals' lists have left by then: the moved
// point (x | y, f64) and the sorted position of its match for each kept pair, in pair order, and the 16 wave counts.
constexpr size_t line_gate_bytes(unsigned threads) {
  return (size_t)threads * (2 * sizeof(double) + sizeof(uint32_t)) + 16 * sizeof(uint32_t);
}
constexpr LinePlan line_gated_batch_plan(unsigned threads, unsigned m_max) {
  LinePlan plan = line_batch_plan(threads, m_max);  // (the same rounds of the normals: the lists decide them)
  const size_t need = (size_t)3 * threads * 8 + line_gate_bytes(threads);
  if (plan.shared_bytes < need) {
    plan.lds_bytes += need - plan.shared_bytes;
    plan.shared_bytes = (unsigned)need;
  }
  return plan;
}
static_assert(line_gated_batch_plan(512, 1).list_threads == 64 &&
                  line_gated_batch_plan(512, 1).shared_bytes == 3 * 512 * 8 + line_gate_bytes(512) &&
                  line_gated_batch_plan(1024, 1).shared_bytes == 3 * 1024 * 8 + line_gate_bytes(1024),
              "m = 1: the sort buffers and the gate's words");
static_assert(line_gated_batch_plan(1024, 668).list_threads == 640 && line_gated_batch_plan(1024, 668).lds_bytes == 158784,
              "m = 668: the gate's words lie where the lists were");
static_assert(line_gated_batch_plan(512, kLineBatchMaxM).list_threads == 320 &&
                  line_gated_batch_plan(1024, kLineBatchMaxM).list_threads == 320 &&
                  line_gated_batch_plan(512, kLineBatchMaxM).lds_bytes == 161856 &&
                  line_gated_batch_plan(1024, kLineBatchMaxM).lds_bytes == 161856 &&
                  line_fixed_bytes(kLineBatchMaxM) + 3 * 1024 * 8 + line_gate_bytes(1024) <= kTinyLdsGrant,
              "m = 2048: nothing on top of the ungated plan");

// One item of a batch, by the workgroup's B threads: what both kernels below run.  GATED: the gate between the search and
// the inner loop; r2, inl_all: the squared bound and the inlier counts (count x max_iter, or null).
template <unsigned B, bool GATED>
__device__ __forceinline__ void line_estimate_item(const double *__restrict__ src_all, const double *__restrict__ dst_all,
                                                   const TinyBatchItem *__restrict__ items, unsigned max_iter, int kk,
                                                   unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                   uint32_t *inner_all, uint32_t *idx_all, double r2, uint32_t *inl_all) {
  static_assert(B == 512 || B == 1024, "one or two blocks of the 512-thread fold tree, a power of two for the sort");
  extern __shared__ unsigned char lds_raw[];
  const TinyBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m;          // 1 <= n <= B, 1 <= m <= kLineBatchMaxM (api_batch.hip: line_fits)
  const double *__restrict__ src = src_all + item.src_first * 2;
  const double *__restrict__ dst = dst_all + item.dst_first * 2;
  TinyResult *res = res_all + item.slot;
  uint32_t *inner_out = inner_all ? inner_all + (size_t)item.slot * max_iter : nullptr;
  uint32_t *idx_out = idx_all ? idx_all + item.idx_first : nullptr;
  const unsigned tid = threadIdx.x;
  const int wave = tid >> 6;

  double cx, cy, cz, scale;  // (cz: +0.0 in two dimensions)
  if (!tiny_batch_box<2, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) {
    if (tid == 0) res->status = -1;
    return;
  }
  // ---- LDS carve-up ----  (targets are kept SORTED BY x: position j below is not the target's index)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  unsigned char *p = reinterpret_cast<unsigned char *>(ty + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y relative to the box centre as f32, -, original index}
  p += sizeof(float4) * (mp + 4);
  double2 *nrm = reinterpret_cast<double2 *>(p);  // the line normal of the target at sorted position j
  p += sizeof(double2) * mp;
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then the estimator's sort (line_batch_plan)
  p += shared_bytes;
  double(*sm)[kLineSums] = reinterpret_cast<double(*)[kLineSums]>(p);
  p += sizeof(double) * 16 * kLineSums;
  double *tot = reinterpret_cast<double *>(p);
  p += sizeof(double) * 16;
  LineCtl *C = reinterpret_cast<LineCtl *>(p);
  const TinyTargets tg = {tx, ty, nullptr, g4, m};

  if (tid == 0) {
    C->T = item.init;
    C->nan = C->bail = 0;
    C->evals = 0;
    C->pos0 = 0;
    C->mad[0][0] = C->mad[0][1] = 0.;
  }
  if (tid < 16) {  // (the wave sums of the waves a 512-thread workgroup does not have stay +0.0)
#pragma unroll
    for (int q = 0; q < kLineSums; ++q) sm[tid][q] = 0.;
  }
  tiny_sort_targets<2, B>(dst, cx, cy, cz, reinterpret_cast<unsigned long long *>(shared), tg,
                          [&](unsigned j, unsigned k, double x, double y) {
                            if (k == 0) C->pos0 = j;
                            if ((x != x) | (y != y)) C->bail = 1;  // a NaN target: the single call decides what such a cloud is
                          });
  if (C->bail) {  // (uniform)
    if (tid == 0) res->status = -1;
    return;
  }
  // ---- line normals: the k best by (d^2, index) of every target, L targets per round (p2line_device.hpp) ----
  line_normals_of_sorted_targets(tg, cx, cy, scale, kk, L, shared, nrm);
  unsigned long long(*sbuf)[1][B] = reinterpret_cast<unsigned long long(*)[1][B]>(shared);  // two sort buffers, then the sorted keys
  const bool has = tid < n;
  double px = 0., py = 0.;
  if (has) {
    px = src[(size_t)tid * 2];
    py = src[(size_t)tid * 2 + 1];
  }
  // the pairs the inner loop sees: all n, thread t its own; gated: the kept ones, thread t the t-th of them
  unsigned cnt = n;
  bool hasp = has;
  int blocks = n > 512u ? 2 : 1;  // reduce_geometry(cnt) for cnt <= 1024: 512-thread blocks
  // the gate's words, behind the sort buffers (line_gated_batch_plan)
  double *gqx = reinterpret_cast<double *>(shared + (size_t)3 * B * 8), *gqy = gqx + B;
  uint32_t *gnb = reinterpret_cast<uint32_t *>(gqy + B), *gcnt = gnb + B;
  uint32_t *inl_out = GATED && inl_all ? inl_all + (size_t)item.slot * max_iter : nullptr;
  unsigned bi = 0xffffffffu;
  for (unsigned it = 0; it < max_iter; ++it) {
    const Pose T = C->T;
    // ---- transform + exact nearest neighbour, the pair of k_line_gather ----
    PlanePair pr;
    pr.ax = pr.ay = pr.qx = pr.qy = pr.dz = pr.nx = pr.ny = pr.nz = 0.;
    auto pair_of = [&](double qx, double qy, unsigned nb) {
      const double2 nq = nrm[nb];
      pr.ax = qx;
      pr.ay = qy;
      pr.qx = tx[nb];
      pr.qy = ty[nb];
      pr.nx = nq.x;
      pr.ny = nq.y;
    };
    double qx = 0., qy = 0.;
    unsigned nb = 0;  // sorted position of the nearest target
    bool in = false;  // (gated) the pair passes the gate
    if (has) {
      qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      qy = (T.r10 * px + T.r11 * py) + T.ty;
      unsigned nbo;  // original index of the nearest target
      tiny_nearest<2>(tg, qx, qy, 0., cx, cy, cz, scale, bi, &nb, &nbo);
      bi = nb;
      if (nb == 0xffffffffu) {  // no finite distance (NaN query): index 0, as a scan from 0 would
        nb = C->pos0;
        nbo = 0;
      }
      if constexpr (GATED) {  // k_lngate_stage's expressions
        const double ex = qx - tx[nb], ey = qy - ty[nb];
        const double d2 = ex * ex + ey * ey;
        in = d2 <= r2;  // (false for a NaN d2)
      } else {
        pair_of(qx, qy, nb);
      }
      if (idx_out && it + 1 == max_iter) idx_out[tid] = nbo;
    }
    if constexpr (GATED) {
      // ---- the gate: the kept pairs in thread order (stable), pair t to thread t ----
      // rank = kept lanes before this one in its wave + the counts of the waves before it; the kept lanes of a wave
      // write consecutive words
      const unsigned long long bal = __ballot(in);
      unsigned rank = (unsigned)__popcll(bal & ((1ull << (tid & 63)) - 1ull));
      if ((tid & 63) == 0) gcnt[wave] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned kept = 0;
#pragma unroll
      for (int w = 0; w < (int)(B / 64); ++w) {
        const unsigned c = gcnt[w];
        rank += w < wave ? c : 0u;
        kept += c;
      }
      if (in) {
        gqx[rank] = qx;
        gqy[rank] = qy;
        gnb[rank] = nb;
      }
      cnt = (unsigned)__builtin_amdgcn_readfirstlane((int)kept);  // (the same in every thread)
      hasp = tid < cnt;
      blocks = cnt > 512u ? 2 : 1;
    }
    // ---- p2pl_loop_on_pairs (api_ext.hip) on the cnt pairs (pair_loop_device.hpp) ----
    tiny_pair_loop<B>(pr, hasp, cnt, blocks, C, sbuf, sm, tot, [&]() {
      if constexpr (GATED) {
        if (hasp) pair_of(gqx[tid], gqy[tid], gnb[tid]);
      }
    });
    if (tid == 0) {
      tiny_outer_tail(C, it, max_iter, inner_out);
      if constexpr (GATED) {
        // the iterations a fixed point skips repeat this one's search and gate: this one's count is theirs
        if (inl_out) {
          inl_out[it] = cnt;
          if (C->fixed && it + 2 < max_iter)
            for (unsigned k = it + 1; k + 1 < max_iter; ++k) inl_out[k] = cnt;
        }
      }
    }
    __syncthreads();
    if (C->nan | C->bail) break;
    if (C->fixed && it + 2 < max_iter) it = max_iter - 2;  // (uniform: the flag is the workgroup's)
  }
  if (tid == 0) {
    res->pose = C->T;
    res->evals = C->evals;
    res->sorted = C->evals;
    res->status = C->nan ? 3 : (C->bail ? -1 : 0);
  }
}

template <unsigned B>
__global__ __launch_bounds__(B) void k_line_estimate_batch(const double *__restrict__ src_all,
                                                           const double *__restrict__ dst_all,
                                                           const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                           int kk, unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                           uint32_t *inner_all, uint32_t *idx_all) {
  line_estimate_item<B, false>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all, 0.,
                               nullptr);
}

// section 17: r2 = max_dist^2; inl_all: count x max_iter inlier counts, or null
template <unsigned B>
__global__ __launch_bounds__(B) void k_line_estimate_gated_batch(const double *__restrict__ src_all,
                                                                 const double *__restrict__ dst_all,
                                                                 const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                                 int kk, unsigned L, unsigned shared_bytes, double r2,
                                                                 TinyResult *res_all, uint32_t *inner_all,
                                                                 uint32_t *idx_all, uint32_t *inl_all) {
  line_estimate_item<B, true>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all, r2,
                              inl_all);
}

hipError_t launch_line_estimate_batch(unsigned threads, unsigned m_max, const double *d_src, const double *d_dst,
                                      const TinyBatchItem *d_items, unsigned count, unsigned max_iter, int k,
                                      TinyResult *res, uint32_t *inner, uint32_t *d_idx, hipStream_t stream, bool *granted) {
  // the grant above 64 KB of dynamic LDS, asked for both kernels once per process; refused: nothing launches
  static TinyLdsGrant grant;
  *granted = grant.ask({reinterpret_cast<const void *>(&k_line_estimate_batch<512>),
                        reinterpret_cast<const void *>(&k_line_estimate_batch<1024>)},
                       kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const LinePlan plan = line_batch_plan(threads, m_max);
  if (threads == 512u)
    hipLaunchKernelGGL((k_line_estimate_batch<512>), dim3(count), dim3(512), plan.lds_bytes, stream, d_src, d_dst, d_items,
                       max_iter, k, plan.list_threads, plan.shared_bytes, res, inner, d_idx);
  else
    hipLaunchKernelGGL((k_line_estimate_batch<1024>), dim3(count), dim3(1024), plan.lds_bytes, stream, d_src, d_dst, d_items,
                       max_iter, k, plan.list_threads, plan.shared_bytes, res, inner, d_idx);
  return hipGetLastError();
}

hipError_t launch_line_estimate_gated_batch(unsigned threads, unsigned m_max, const double *d_src, const double *d_dst,
                                            const TinyBatchItem *d_items, unsigned count, unsigned max_iter, int k,
                                            double r2, TinyResult *res, uint32_t *inner, uint32_t *d_idx,
                                            uint32_t *inliers, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;  // (these kernels' own: refused, nothing launches)
  *granted = grant.ask({reinterpret_cast<const void *>(&k_line_estimate_gated_batch<512>),
                        reinterpret_cast<const void *>(&k_line_estimate_gated_batch<1024>)},
                       kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const LinePlan plan = line_gated_batch_plan(threads, m_max);
  if (threads == 512u)
    hipLaunchKernelGGL((k_line_estimate_gated_batch<512>), dim3(count), dim3(512), plan.lds_bytes, stream, d_src, d_dst,
                       d_items, max_iter, k, plan.list_threads, plan.shared_bytes, r2, res, inner, d_idx, inliers);
  else
    hipLaunchKernelGGL((k_line_estimate_gated_batch<1024>), dim3(count), dim3(1024), plan.lds_bytes, stream, d_src, d_dst,
                       d_items, max_iter, k, plan.list_threads, plan.shared_bytes, r2, res, inner, d_idx, inliers);
  return hipGetLastError();
}

}  // namespace icp
