// EXTENSION beyond the reference (include/icp_mi355x.h section 18): batched point-to-PLANE registration, one workgroup per
// 3-D item.  Item i's result is what icp_create(3, dst_i) + icp_compute_target_normals(k) + icp_estimate_point_to_plane
// return on a fresh handle, bit for bit (p2plane.hip's header comment and api_ext.hip: p2pl_loop_on_pairs are the
// definition), or the workgroup hands the item back (TinyResult::status = -1) and api_batch.hip serves it through exactly
// those entries.  Nothing crosses workgroups: no flag, no atomic, no barrier across them; every loop has a static bound
// (the rounds of the normals, jacobi3's 12 sweeps, ICP_INNER_MAX_ITER, max_iter).  What a workgroup does, each piece the
// one copy the other one-workgroup kernels run too:
//   box        fmin / fmax over its own targets (tiny_batch_box<3>)
//   targets    sorted by fl32(x - cx) into LDS, x | y | z with the f32 screen records (tiny_sort_targets<3>)
//   normals    per target the k best by (d^2, index), d^2 = (dx dx + dy dy) + dz dz, from a sweep outwards over the sorted
//              targets (tiny_k_best_of_target<3>), lists in LDS for as many targets per round as the grant allows, then
//              plane_normal_of_neighbours, the statement k_target_normals evaluates (p2plane_device.hpp)
//   outer      transform xy with z carried, exact nearest neighbour (tiny_nearest<3>, warm), the pair of k_p2pl_gather
//   inner      tiny_pair_loop (pair_loop_device.hpp): plane_residual, exact median and MAD, k_p2pl_accumulate's 13 sums in
//              the tree of reduce_geometry(n), solve_update and the break tests; then tiny_outer_tail
// Hand-back reasons: a box that is not finite; a NaN target coordinate; a rotation update outside the restated range of
// sin / cos.  A NaN residual is the item's ICP_NAN_INPUT.
// Section 19, k_plane_estimate_gated_batch: the same body (plane_estimate_item) with the gate of
// icp_estimate_point_to_plane_gated between the search and the inner loop -- the pairs with d2 <= r^2 (gate_plane.hip:
// k_plgate_stage's expressions, d2 = (ex ex + ey ey) + dz dz), compacted in thread order, and p2pl_loop_on_pairs on the
// `kept` of them in the tree of reduce_geometry(kept).
#include "common.hpp"
#include "gn_device.hpp"
#include "p2plane_device.hpp"
#include "pair_loop_device.hpp"
#include "tiny_device.hpp"

namespace icp {

// ---- the LDS plan of a launch ----
// per workgroup, for its item's m targets (mp = m rounded up to 64): x | y | z (f64), the f32 screen records (+ 4 pads),
// the normals by sorted position (3 x f64); then ONE shared region, sized by the launch; then the wave sums, the totals
// and PairCtl.  The shared region holds, one after the other: the target sort's keys (8 B x the next power of two of m),
// the k-best lists of the normals ((8 + 4) B x 16 per list-holding thread), the estimator's two sort buffers and sorted
// keys (3 x 8 B x B).  The normals run in rounds of `list_threads` targets: as many as the grant leaves room for, up to
// one per thread and per target -- 128 beside 2048 targets, sixteen rounds with most of the workgroup idle.
constexpr size_t kPlaneListBytes = kTinyKBestMax * (sizeof(double) + sizeof(uint32_t));
constexpr size_t plane_fixed_bytes(unsigned m) {
  const size_t mp = (m + 63u) & ~63u;
  return mp * 3 * sizeof(double) + (mp + 4) * sizeof(float4) + mp * 3 * sizeof(double) + sizeof(double) * 16 * kPairSums +
         sizeof(double) * 16 + 256;
}
static_assert(sizeof(PairCtl) <= 256, "PairCtl's share of the LDS");
static_assert(kPlaneListBytes == 192, "sixteen (d^2, index | position) entries");
static_assert(kPlaneBatchMaxM <= kTinyKBestMaxTargets, "(original index << 16) | sorted position: both below 2^16");
static_assert(1024 / 64 * 6 * sizeof(double) <= plane_fixed_bytes(1), "the box's wave minima");
constexpr PlanePlan plane_batch_plan(unsigned threads, unsigned m_max) {
  const size_t fixed = plane_fixed_bytes(m_max);
  size_t keys = 64;
  while (keys < m_max) keys <<= 1;
  const size_t fit = (kTinyLdsGrant - fixed) / kPlaneListBytes / 64 * 64;
  size_t lists = (m_max + 63u) & ~63u;  // (a list per target is all a round can use)
  lists = lists < threads ? lists : threads;
  lists = lists < fit ? lists : fit;
  size_t shared = lists * kPlaneListBytes;
  shared = shared > keys * 8 ? shared : keys * 8;
  shared = shared > (size_t)3 * threads * 8 ? shared : (size_t)3 * threads * 8;
  return PlanePlan{(unsigned)lists, (unsigned)shared, (unsigned)fixed, (unsigned)(fixed + shared)};
}
// the plan at its corners: the smallest item, 1024 targets (three rounds of 448), the largest item (sixteen rounds of 128)
static_assert(plane_batch_plan(512, 1).list_threads == 64 && plane_batch_plan(512, 1).shared_bytes == 3 * 512 * 8 &&
                  plane_batch_plan(1024, 1).shared_bytes == 3 * 1024 * 8 && plane_batch_plan(512, 1).fixed_bytes == 6208,
              "m = 1");
static_assert(plane_batch_plan(1024, 1024).fixed_bytes == 67648 && plane_batch_plan(1024, 1024).list_threads == 448 &&
                  plane_batch_plan(512, 1024).list_threads == 448 && plane_batch_plan(1024, 1024).shared_bytes == 448 * 192,
              "m = 1024");
static_assert(plane_batch_plan(1024, kPlaneBatchMaxM).fixed_bytes == 133184 &&
                  kTinyLdsGrant - plane_batch_plan(1024, kPlaneBatchMaxM).fixed_bytes == 30400 &&
                  plane_batch_plan(512, kPlaneBatchMaxM).list_threads == 128 &&
                  plane_batch_plan(1024, kPlaneBatchMaxM).list_threads == 128 &&
                  plane_batch_plan(1024, kPlaneBatchMaxM).shared_bytes == 3 * 1024 * 8 &&
                  plane_batch_plan(1024, kPlaneBatchMaxM).lds_bytes == 157760 &&
                  plane_batch_plan(1024, kPlaneBatchMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048: the sort buffers fit in what the fixed part leaves");
// ... and at every m between: at least one round's lists, and never more LDS than the grant
constexpr bool plane_batch_plan_fits_everywhere() {
  for (unsigned m = 1; m <= kPlaneBatchMaxM; ++m)
    for (unsigned threads = 512; threads <= 1024; threads += 512) {
      const PlanePlan plan = plane_batch_plan(threads, m);
      if (plan.list_threads < 64 || plan.list_threads > threads || plan.lds_bytes > kTinyLdsGrant) return false;
    }
  return true;
}
static_assert(plane_batch_plan_fits_everywhere(), "every launch's LDS is within the grant");

PlanePlan plane_batch_plan_of(unsigned threads, unsigned m_max) { return plane_batch_plan(threads, m_max); }

// ---- the gate's words (section 19) ----
// Behind the estimator's three sort buffers in the shared region, which the normals' lists have left by then: ONE word
// per kept pair, in pair order -- (source thread << 16) | sorted position of its match, both below 2^16 -- and the 16 wave
// counts.  The moved point is not kept: thread t reads the source row of pair t again and forms qx, qy with the
// expression and the pose the gate formed them with.  The record the line kernel keeps (x | y as f64 and the position,
// with z 28 B a pair: plane_gate_line_style_bytes) does not fit behind the sort buffers beyond 1664 targets.
constexpr size_t plane_gate_bytes(unsigned threads) {
  return (size_t)threads * sizeof(uint32_t) + 16 * sizeof(uint32_t);
}
constexpr size_t plane_gate_line_style_bytes(unsigned threads) {
  return (size_t)threads * (3 * sizeof(double) + sizeof(uint32_t)) + 16 * sizeof(uint32_t);
}
static_assert(kPlaneBatchMaxN <= 0x10000u && kPlaneBatchMaxM <= 0x10000u,
              "a source thread and a sorted position in 16 bits each");
constexpr PlanePlan plane_gated_batch_plan(unsigned threads, unsigned m_max) {
  PlanePlan plan = plane_batch_plan(threads, m_max);  // (the same rounds of the normals: the lists decide them)
  const size_t need = (size_t)3 * threads * 8 + plane_gate_bytes(threads);
  if (plan.shared_bytes < need) {
    plan.lds_bytes += (unsigned)(need - plan.shared_bytes);
    plan.shared_bytes = (unsigned)need;
  }
  return plan;
}
PlanePlan plane_gated_batch_plan_of(unsigned threads, unsigned m_max) { return plane_gated_batch_plan(threads, m_max); }
// the plan at its corners
static_assert(plane_gate_bytes(512) == 2112 && plane_gate_bytes(1024) == 4160 &&
                  plane_gate_line_style_bytes(512) == 14400 && plane_gate_line_style_bytes(1024) == 28736,
              "the gate's words, and what the line kernel's record would take");
// (what a 1024-thread workgroup of m targets would need with the line kernel's record behind its sort buffers)
constexpr size_t plane_line_style_lds(unsigned m) {
  return plane_fixed_bytes(m) + 3 * 1024 * 8 + plane_gate_line_style_bytes(1024);
}
static_assert(plane_gated_batch_plan(512, 1).list_threads == 64 && plane_gated_batch_plan(1024, 1).list_threads == 64 &&
                  plane_gated_batch_plan(512, 1).shared_bytes == 3 * 512 * 8 + 2112 &&
                  plane_gated_batch_plan(1024, 1).shared_bytes == 3 * 1024 * 8 + 4160 &&
                  plane_gated_batch_plan(512, 1).lds_bytes == 6208 + 14400 &&
                  plane_gated_batch_plan(1024, 1).lds_bytes == 6208 + 28736,
              "m = 1: the sort buffers and the gate's words");
static_assert(plane_gated_batch_plan(512, 1024).list_threads == 448 &&
                  plane_gated_batch_plan(1024, 1024).list_threads == 448 &&
                  plane_gated_batch_plan(512, 1024).lds_bytes == plane_batch_plan(512, 1024).lds_bytes &&
                  plane_gated_batch_plan(1024, 1024).lds_bytes == 67648 + 448 * 192,
              "m = 1024: the gate's words lie where the lists were");
static_assert(plane_fixed_bytes(1664) == 108608 && plane_line_style_lds(1664) == 161920 &&
                  plane_line_style_lds(1664) <= kTinyLdsGrant && plane_gated_batch_plan(512, 1664).list_threads == 256 &&
                  plane_gated_batch_plan(1024, 1664).list_threads == 256 &&
                  plane_gated_batch_plan(512, 1664).lds_bytes == 108608 + 256 * 192 &&
                  plane_gated_batch_plan(1024, 1664).lds_bytes == 108608 + 256 * 192,
              "m = 1664: the last m at which the line kernel's record would still fit; nothing on top of the ungated plan");
static_assert(plane_fixed_bytes(1665) == 112704 && plane_line_style_lds(1665) > kTinyLdsGrant &&
                  plane_gated_batch_plan(512, 1665).list_threads == 256 &&
                  plane_gated_batch_plan(1024, 1665).list_threads == 256 &&
                  plane_gated_batch_plan(512, 1665).lds_bytes == 112704 + 256 * 192 &&
                  plane_gated_batch_plan(1024, 1665).lds_bytes == 161856,
              "m = 1665: the line kernel's record overflows the grant, the one word per pair does not");
static_assert(plane_gated_batch_plan(512, kPlaneBatchMaxM).list_threads == 128 &&
                  plane_gated_batch_plan(1024, kPlaneBatchMaxM).list_threads == 128 &&
                  plane_gated_batch_plan(512, kPlaneBatchMaxM).lds_bytes == 157760 &&
                  plane_gated_batch_plan(1024, kPlaneBatchMaxM).shared_bytes == 3 * 1024 * 8 + 4160 &&
                  plane_gated_batch_plan(1024, kPlaneBatchMaxM).shared_bytes <= 30400 &&
                  plane_gated_batch_plan(1024, kPlaneBatchMaxM).lds_bytes == 133184 + 28736 &&
                  plane_gated_batch_plan(1024, kPlaneBatchMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048: 28 736 of the 30 400 bytes the fixed part leaves");
// ... and at every m between: within the grant, and the rounds of the normals those of the ungated plan
constexpr bool plane_gated_batch_plan_fits_everywhere() {
  for (unsigned m = 1; m <= kPlaneBatchMaxM; ++m)
    for (unsigned threads = 512; threads <= 1024; threads += 512) {
      const PlanePlan plan = plane_gated_batch_plan(threads, m);
      if (plan.list_threads < 64 || plan.list_threads > threads || plan.lds_bytes > kTinyLdsGrant) return false;
      if (plan.list_threads != plane_batch_plan(threads, m).list_threads) return false;
      if (plan.shared_bytes < 3 * threads * 8 + plane_gate_bytes(threads)) return false;
      if (plan.lds_bytes != plan.fixed_bytes + plan.shared_bytes) return false;
    }
  return true;
}
static_assert(plane_gated_batch_plan_fits_everywhere(), "every gated launch's LDS is within the grant");

// (the plane normals of a workgroup's own targets: p2plane_device.hpp, plane_normals_of_sorted_targets, which
// quality_plane_batch.hip: k_plane_quality_batch runs too)

// One item of a batch, by the workgroup's B threads: what both kernels below run.  GATED: the gate between the search and
// the inner loop; r2, inl_all: the squared bound and the inlier counts (count x max_iter, or null).
template <unsigned B, bool GATED>
__device__ __forceinline__ void plane_estimate_item(const double *__restrict__ src_all, const double *__restrict__ dst_all,
                                                    const TinyBatchItem *__restrict__ items, unsigned max_iter, int kk,
                                                    unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                    uint32_t *inner_all, uint32_t *idx_all, double r2, uint32_t *inl_all) {
  static_assert(B == 512 || B == 1024, "one or two blocks of the 512-thread fold tree, a power of two for the sort");
  extern __shared__ unsigned char lds_raw[];
  const TinyBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m;          // 1 <= n <= B, 1 <= m <= kPlaneBatchMaxM (api_batch.hip: plane_fits)
  const double *__restrict__ src = src_all + item.src_first * 3;
  const double *__restrict__ dst = dst_all + item.dst_first * 3;
  TinyResult *res = res_all + item.slot;
  uint32_t *inner_out = inner_all ? inner_all + (size_t)item.slot * max_iter : nullptr;
  uint32_t *idx_out = idx_all ? idx_all + item.idx_first : nullptr;
  const unsigned tid = threadIdx.x;

  double cx, cy, cz, scale;
  if (!tiny_batch_box<3, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) {
    if (tid == 0) res->status = -1;
    return;
  }
  // ---- LDS carve-up (plane_batch_plan) ----  (targets are kept SORTED BY x: position j below is not the target's index)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  double *tz = ty + mp;
  unsigned char *p = reinterpret_cast<unsigned char *>(tz + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y, z relative to the box centre as f32, original index}
  p += sizeof(float4) * (mp + 4);
  double *nrm = reinterpret_cast<double *>(p);  // the plane normal of the target at sorted position j, at [3 j]
  p += sizeof(double) * 3 * mp;
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then the estimator's sort
  p += shared_bytes;
  double(*sm)[kPairSums] = reinterpret_cast<double(*)[kPairSums]>(p);
  p += sizeof(double) * 16 * kPairSums;
  double *tot = reinterpret_cast<double *>(p);
  p += sizeof(double) * 16;
  PairCtl *C = reinterpret_cast<PairCtl *>(p);
  const TinyTargets tg = {tx, ty, tz, g4, m};

  if (tid == 0) {
    C->T = item.init;
    C->nan = C->bail = 0;
    C->evals = 0;
    C->pos0 = 0;
    C->mad[0][0] = C->mad[0][1] = 0.;
  }
  if (tid < 16) {  // (the wave sums of the waves a 512-thread workgroup does not have stay +0.0)
#pragma unroll
    for (int q = 0; q < kPairSums; ++q) sm[tid][q] = 0.;
  }
  tiny_sort_targets<3, B>(dst, cx, cy, cz, reinterpret_cast<unsigned long long *>(shared), tg,
                          [&](unsigned j, unsigned k, double x, double y) {
                            if (k == 0) C->pos0 = j;
                            const double z = tz[j];  // (this thread has just written it)
                            if ((x != x) | (y != y) | (z != z)) C->bail = 1;  // a NaN target: the single call decides
                          });
  if (C->bail) {  // (uniform)
    if (tid == 0) res->status = -1;
    return;
  }
  plane_normals_of_sorted_targets(tg, cx, cy, cz, scale, kk, L, shared, nrm);
  unsigned long long(*sbuf)[1][B] = reinterpret_cast<unsigned long long(*)[1][B]>(shared);  // two sort buffers, then the sorted keys
  const bool has = tid < n;
  double px = 0., py = 0., pz = 0.;
  if (has) {
    px = src[(size_t)tid * 3];
    py = src[(size_t)tid * 3 + 1];
    pz = src[(size_t)tid * 3 + 2];
  }
  // the pairs the inner loop sees: all n, thread t its own; gated: the kept ones, thread t the t-th of them
  unsigned cnt = n;
  bool hasp = has;
  int blocks = n > 512u ? 2 : 1;  // reduce_geometry(cnt) for cnt <= 1024: 512-thread blocks
  // the gate's words, behind the sort buffers (plane_gated_batch_plan)
  uint32_t *gw = reinterpret_cast<uint32_t *>(shared + (size_t)3 * B * 8), *gcnt = gw + B;
  uint32_t *inl_out = GATED && inl_all ? inl_all + (size_t)item.slot * max_iter : nullptr;
  unsigned bi = 0xffffffffu;
  for (unsigned it = 0; it < max_iter; ++it) {
    const Pose T = C->T;
    // ---- transform + exact nearest neighbour, the pair of k_p2pl_gather ----
    PlanePair pr;
    pr.ax = pr.ay = pr.qx = pr.qy = pr.dz = pr.nx = pr.ny = pr.nz = 0.;
    unsigned nb = 0;  // sorted position of the nearest target
    bool in = false;  // (gated) the pair passes the gate
    if (has) {
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24; z is carried
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      unsigned nbo;  // original index of the nearest target
      tiny_nearest<3>(tg, qx, qy, pz, cx, cy, cz, scale, bi, &nb, &nbo);
      bi = nb;
      if (nb == 0xffffffffu) {  // no finite distance (NaN query): index 0, as a scan from 0 would
        nb = C->pos0;
        nbo = 0;
      }
      if constexpr (GATED) {  // k_plgate_stage's expressions
        const double ex = qx - tx[nb], ey = qy - ty[nb], dz = pz - tz[nb];
        const double d2 = (ex * ex + ey * ey) + dz * dz;
        in = d2 <= r2;  // (false for a NaN d2)
      } else {
        pr.ax = qx;
        pr.ay = qy;
        pr.qx = tx[nb];
        pr.qy = ty[nb];
        pr.dz = pz - tz[nb];
        pr.nx = nrm[3 * nb];
        pr.ny = nrm[3 * nb + 1];
        pr.nz = nrm[3 * nb + 2];
      }
      if (idx_out && it + 1 == max_iter) idx_out[tid] = nbo;
    }
    if constexpr (GATED) {
      // ---- the gate: the kept pairs in thread order (stable), pair t to thread t ----
      // rank = kept lanes before this one in its wave + the counts of the waves before it; the kept lanes of a wave
      // write consecutive words
      const int wave = tid >> 6;
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
      if (in) gw[rank] = (tid << 16) | nb;  // (rank < kept <= n <= B; tid < 1024 and nb < m <= 2048: 16 bits each)
      cnt = (unsigned)__builtin_amdgcn_readfirstlane((int)kept);  // (the same in every thread)
      hasp = tid < cnt;
      blocks = cnt > 512u ? 2 : 1;
    }
    // ---- p2pl_loop_on_pairs (api_ext.hip) on the cnt pairs (pair_loop_device.hpp) ----
    tiny_pair_loop<B>(pr, hasp, cnt, blocks, C, sbuf, sm, tot, [&]() {
      if constexpr (GATED) {
        // pair t: its source row read again and moved by the pose the gate moved it by (C->T: thread 0 writes it next in
        // tiny_outer_tail, behind the loop) -- the same expressions, the same bits; the eight values k_plgate_stage writes
        if (hasp) {
          const unsigned w = gw[tid], s = w >> 16, g = w & 0xffffu;  // (s < n, g < m: written by the gate above)
          const double sx = src[(size_t)s * 3], sy = src[(size_t)s * 3 + 1], sz = src[(size_t)s * 3 + 2];
          const Pose G = C->T;
          pr.ax = (G.r00 * sx + G.r01 * sy) + G.tx;
          pr.ay = (G.r10 * sx + G.r11 * sy) + G.ty;
          pr.qx = tx[g];
          pr.qy = ty[g];
          pr.dz = sz - tz[g];
          pr.nx = nrm[3 * g];
          pr.ny = nrm[3 * g + 1];
          pr.nz = nrm[3 * g + 2];
        }
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
__global__ __launch_bounds__(B) void k_plane_estimate_batch(const double *__restrict__ src_all,
                                                            const double *__restrict__ dst_all,
                                                            const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                            int kk, unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                            uint32_t *inner_all, uint32_t *idx_all) {
  plane_estimate_item<B, false>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all, 0.,
                                nullptr);
}

// section 19: r2 = max_dist^2; inl_all: count x max_iter inlier counts, or null
template <unsigned B>
__global__ __launch_bounds__(B) void k_plane_estimate_gated_batch(const double *__restrict__ src_all,
                                                                  const double *__restrict__ dst_all,
                                                                  const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                                  int kk, unsigned L, unsigned shared_bytes, double r2,
                                                                  TinyResult *res_all, uint32_t *inner_all,
                                                                  uint32_t *idx_all, uint32_t *inl_all) {
  plane_estimate_item<B, true>(src_all, dst_all, items, max_iter, kk, L, shared_bytes, res_all, inner_all, idx_all, r2,
                               inl_all);
}

hipError_t launch_plane_estimate_batch(unsigned threads, unsigned m_max, const double *d_src, const double *d_dst,
                                       const TinyBatchItem *d_items, unsigned count, unsigned max_iter, int k,
                                       TinyResult *res, uint32_t *inner, uint32_t *d_idx, hipStream_t stream, bool *granted) {
  // the grant above 64 KB of dynamic LDS, asked for both kernels once per process; refused: nothing launches
  static TinyLdsGrant grant;
  *granted = grant.ask({reinterpret_cast<const void *>(&k_plane_estimate_batch<512>),
                        reinterpret_cast<const void *>(&k_plane_estimate_batch<1024>)},
                       kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const PlanePlan plan = plane_batch_plan(threads, m_max);
  if (threads == 512u)
    hipLaunchKernelGGL((k_plane_estimate_batch<512>), dim3(count), dim3(512), plan.lds_bytes, stream, d_src, d_dst, d_items,
                       max_iter, k, plan.list_threads, plan.shared_bytes, res, inner, d_idx);
  else
    hipLaunchKernelGGL((k_plane_estimate_batch<1024>), dim3(count), dim3(1024), plan.lds_bytes, stream, d_src, d_dst,
                       d_items, max_iter, k, plan.list_threads, plan.shared_bytes, res, inner, d_idx);
  return hipGetLastError();
}

hipError_t launch_plane_estimate_gated_batch(unsigned threads, unsigned m_max, const double *d_src, const double *d_dst,
                                             const TinyBatchItem *d_items, unsigned count, unsigned max_iter, int k,
                                             double r2, TinyResult *res, uint32_t *inner, uint32_t *d_idx,
                                             uint32_t *inliers, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;  // (these kernels' own: refused, nothing launches)
  *granted = grant.ask({reinterpret_cast<const void *>(&k_plane_estimate_gated_batch<512>),
                        reinterpret_cast<const void *>(&k_plane_estimate_gated_batch<1024>)},
                       kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const PlanePlan plan = plane_gated_batch_plan(threads, m_max);
  if (threads == 512u)
    hipLaunchKernelGGL((k_plane_estimate_gated_batch<512>), dim3(count), dim3(512), plan.lds_bytes, stream, d_src, d_dst,
                       d_items, max_iter, k, plan.list_threads, plan.shared_bytes, r2, res, inner, d_idx, inliers);
  else
    hipLaunchKernelGGL((k_plane_estimate_gated_batch<1024>), dim3(count), dim3(1024), plan.lds_bytes, stream, d_src, d_dst,
                       d_items, max_iter, k, plan.list_threads, plan.shared_bytes, r2, res, inner, d_idx, inliers);
  return hipGetLastError();
}

}  // namespace icp
