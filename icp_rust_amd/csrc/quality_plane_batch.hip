// EXTENSION beyond the reference (include/icp_mi355x.h section 20): the quality of many poses under the point-to-PLANE
// residual of section 13, one workgroup per 3-D item.  Item i's record is what icp_create(3, dst_i) +
// icp_compute_target_normals(k) + icp_evaluate_point_to_plane(src_i, T_i, max_dist) fold on a fresh handle, bit for bit,
// or the workgroup hands the item back (its record is left alone) and api_batch.hip serves it through exactly those
// entries.  Nothing crosses workgroups: no flag, no atomic; every loop has a static bound.
//   k_plane_quality_batch  the item's box (tiny_batch_box<3>), its targets sorted into LDS (tiny_sort_targets<3>), their
//                          plane normals (p2plane_device.hpp: the rounds k_plane_estimate_batch runs), the exact nearest
//                          neighbour of every moved source point from a cold start (tiny_nearest<3>), the ten terms of
//                          section 13 (normal_quality_terms<3>) and the tree of a batch item (fold_workgroup), as
//                          k_line_quality_batch (quality_line.hip) does in two dimensions
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.
#include "p2plane_device.hpp"
#include "quality_device.hpp"
#include "tiny_device.hpp"

using namespace icp;

namespace icp {

// ---- the LDS plan of a launch ----
// per workgroup, for its item's m targets (mp = m rounded up to 64): x | y | z (f64), the f32 screen records (+ 4 pads),
// the normals by sorted position (3 x f64); then ONE shared region, sized by the launch; then the control words.  The
// shared region holds, one after the other: the target sort's keys (8 B x the next power of two of m), the k-best lists
// of the normals ((8 + 4) B x 16 per list-holding thread), and then the fold's group (FoldLds<10>) with the four group
// records behind it: the fold aliases the lists, which are dead by then.  None of the estimator's wave sums, totals,
// PairCtl and sort buffers (plane_batch_plan) are here.  The rounds of the normals hold as many lists as the grant
// leaves room for: 448 at m = 1024, 128 at m = 2048, the estimate kernel's.
namespace {

constexpr unsigned kPlaneQualityThreads = 1024;
constexpr size_t kPlaneQualityListBytes = kTinyKBestMax * (sizeof(double) + sizeof(uint32_t));
constexpr size_t kPlaneQualityFoldBytes =
    sizeof(FoldLds<kNormalQualitySums>) + (kPlaneQualityMaxN / kFoldGroup) * sizeof(NormalQualityPart);
constexpr size_t kPlaneQualityCtlBytes = 256;
struct PlaneQualityCtl {
  unsigned pos0;  // the sorted position of the target of original index 0
  int bail;       // a NaN target: the single call decides what such a cloud is
};
static_assert(sizeof(PlaneQualityCtl) <= kPlaneQualityCtlBytes, "the control words' share of the LDS");
constexpr size_t plane_quality_fixed_bytes(unsigned m) {
  const size_t mp = (m + 63u) & ~63u;
  return mp * 3 * sizeof(double) + (mp + 4) * sizeof(float4) + mp * 3 * sizeof(double) + kPlaneQualityCtlBytes;
}
constexpr size_t plane_quality_keys_bytes(unsigned m) {
  size_t keys = 64;
  while (keys < m) keys <<= 1;
  return keys * 8;
}
constexpr PlanePlan plane_quality_plan(unsigned m_max) {
  const size_t fixed = plane_quality_fixed_bytes(m_max);
  const size_t keys = plane_quality_keys_bytes(m_max);
  const size_t fit = (kTinyLdsGrant - fixed) / kPlaneQualityListBytes / 64 * 64;
  size_t lists = (m_max + 63u) & ~63u;  // (a list per target is all a round can use)
  lists = lists < kPlaneQualityThreads ? lists : kPlaneQualityThreads;
  lists = lists < fit ? lists : fit;
  size_t shared = lists * kPlaneQualityListBytes;
  shared = shared > keys ? shared : keys;
  shared = shared > kPlaneQualityFoldBytes ? shared : kPlaneQualityFoldBytes;
  return PlanePlan{(unsigned)lists, (unsigned)shared, (unsigned)fixed, (unsigned)(fixed + shared)};
}
static_assert(kPlaneQualityListBytes == 192, "sixteen (d^2, index | position) entries");
static_assert(kPlaneQualityFoldBytes == 23936 && kPlaneQualityFoldBytes % 16 == 0, "a group of the tree and four records");
static_assert(kPlaneQualityMaxM <= kTinyKBestMaxTargets, "(original index << 16) | sorted position: both below 2^16");
static_assert(kPlaneQualityMaxN == kPlaneQualityThreads, "a thread per source point");
static_assert(kPlaneQualityMaxN >= kPlaneBatchMaxN && kPlaneQualityMaxM >= kPlaneBatchMaxM,
              "every item the estimate serves in a launch is served in a launch here");
// the plan at its corners: the smallest item (the fold sizes the region), 1024 targets (three rounds of 448), the
// largest item (sixteen rounds of 128: their lists are just above the fold's bytes)
static_assert(plane_quality_plan(1).fixed_bytes == 4416 && plane_quality_plan(1).list_threads == 64 &&
                  plane_quality_plan(1).shared_bytes == kPlaneQualityFoldBytes && plane_quality_plan(1).lds_bytes == 28352,
              "m = 1");
static_assert(plane_quality_plan(1024).fixed_bytes == 65856 && plane_quality_plan(1024).list_threads == 448 &&
                  plane_quality_plan(1024).shared_bytes == 448 * 192 && plane_quality_plan(1024).lds_bytes == 151872,
              "m = 1024");
static_assert(plane_quality_plan(kPlaneQualityMaxM).fixed_bytes == 131392 &&
                  plane_quality_plan(kPlaneQualityMaxM).list_threads == 128 &&
                  plane_quality_plan(kPlaneQualityMaxM).shared_bytes == 128 * 192 &&
                  plane_quality_plan(kPlaneQualityMaxM).shared_bytes >= kPlaneQualityFoldBytes &&
                  plane_quality_plan(kPlaneQualityMaxM).lds_bytes == 155968 &&
                  plane_quality_plan(kPlaneQualityMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048");
// ... and at every m between: within the grant, at least one round's lists and at most a list per thread, room for the
// fold and for the sort's keys in the shared region, room for the box's wave minima in front of it
constexpr bool plane_quality_plan_fits_everywhere() {
  for (unsigned m = 1; m <= kPlaneQualityMaxM; ++m) {
    const PlanePlan plan = plane_quality_plan(m);
    if (plan.lds_bytes > kTinyLdsGrant || plan.lds_bytes != plan.fixed_bytes + plan.shared_bytes) return false;
    if (plan.list_threads < 64 || plan.list_threads > kPlaneQualityThreads || plan.list_threads % 64 != 0) return false;
    if (plan.shared_bytes < plan.list_threads * kPlaneQualityListBytes) return false;
    if (plan.shared_bytes < kPlaneQualityFoldBytes || plan.shared_bytes < plane_quality_keys_bytes(m)) return false;
    if (kPlaneQualityThreads / 64 * 6 * sizeof(double) > plan.fixed_bytes - kPlaneQualityCtlBytes) return false;
  }
  return true;
}
static_assert(plane_quality_plan_fits_everywhere(), "every launch's LDS is within the grant");

}  // namespace

PlanePlan plane_quality_plan_of(unsigned m_max) { return plane_quality_plan(m_max); }

// One item per workgroup, a thread per source point (1 <= n <= 1024, 1 <= m <= 2048: api_batch.hip, PlaneQualityKind).
// Hand-backs (the item's record is left as the host preset it, pad != 0): a box that is not finite, a NaN target.
__global__ __launch_bounds__(kPlaneQualityThreads) void k_plane_quality_batch(const double *__restrict__ src_all,
                                                                              const double *__restrict__ dst_all,
                                                                              const QualityBatchItem *__restrict__ items,
                                                                              double r2, int kk, unsigned L,
                                                                              unsigned shared_bytes,
                                                                              NormalQualityPart *__restrict__ res) {
  constexpr unsigned B = kPlaneQualityThreads;
  extern __shared__ unsigned char lds_raw[];
  const QualityBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m, tid = threadIdx.x;
  const double *__restrict__ src = src_all + item.src_first * 3;
  const double *__restrict__ dst = dst_all + item.dst_first * 3;

  double cx, cy, cz, scale;
  if (!tiny_batch_box<3, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) return;
  // ---- LDS carve-up (plane_quality_plan) ----  (targets are kept SORTED BY x: position j below is not the target's index)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  double *tz = ty + mp;
  unsigned char *p = reinterpret_cast<unsigned char *>(tz + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y, z relative to the box centre as f32, original index}
  p += sizeof(float4) * (mp + 4);
  double *nrm = reinterpret_cast<double *>(p);  // the plane normal of the target at sorted position j, at [3 j]
  p += sizeof(double) * 3 * mp;
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then the fold
  p += shared_bytes;
  PlaneQualityCtl *C = reinterpret_cast<PlaneQualityCtl *>(p);
  const TinyTargets tg = {tx, ty, tz, g4, m};

  if (tid == 0) {
    C->pos0 = 0;
    C->bail = 0;
  }
  tiny_sort_targets<3, B>(dst, cx, cy, cz, reinterpret_cast<unsigned long long *>(shared), tg,
                          [&](unsigned j, unsigned k, double x, double y) {
                            if (k == 0) C->pos0 = j;
                            const double z = tz[j];  // (this thread has just written it)
                            if ((x != x) | (y != y) | (z != z)) C->bail = 1;
                          });
  if (C->bail) return;  // (uniform)
  plane_normals_of_sorted_targets(tg, cx, cy, cz, scale, kk, L, shared, nrm);

  // ---- transform with z carried, exact nearest neighbour from a cold start, the ten terms ----
  double v[kNormalQualitySums] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (tid < n) {
    const double px = src[(size_t)tid * 3], py = src[(size_t)tid * 3 + 1], pz = src[(size_t)tid * 3 + 2];
    const double qx = (item.T.r00 * px + item.T.r01 * py) + item.T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (item.T.r10 * px + item.T.r11 * py) + item.T.ty;
    unsigned nb, nbo;  // sorted position / original index of the nearest target
    tiny_nearest<3>(tg, qx, qy, pz, cx, cy, cz, scale, 0xffffffffu, &nb, &nbo);
    if (nb == 0xffffffffu) nb = C->pos0;  // no finite distance (NaN query): index 0, as a scan from 0 would
    const double q[3] = {qx, qy, pz}, b[3] = {tx[nb], ty[nb], tz[nb]};
    const double nn[3] = {nrm[3 * nb], nrm[3 * nb + 1], nrm[3 * nb + 2]};
    normal_quality_terms<3>(q, b, nn, r2, v, in, nan);
  }
  // ---- the tree of a batch item, k_quality_batch's ----
  // (the normals' lists are dead since the barrier behind their last round: the fold takes their place)
  FoldLds<kNormalQualitySums> &F = *reinterpret_cast<FoldLds<kNormalQualitySums> *>(shared);
  NormalQualityPart *grp = reinterpret_cast<NormalQualityPart *>(shared + sizeof(FoldLds<kNormalQualitySums>));
  fold_workgroup(F, grp, tid, n, v, in, nan, &res[item.slot]);
}

hipError_t launch_plane_quality_batch(unsigned m_max, const double *d_src, const double *d_dst,
                                      const QualityBatchItem *d_items, unsigned count, double r2, int k,
                                      NormalQualityPart *res, hipStream_t stream, bool *granted) {
  // the grant above 64 KB of dynamic LDS, asked once per process; refused: nothing launches
  static TinyLdsGrant grant;
  *granted = grant.ask({reinterpret_cast<const void *>(&k_plane_quality_batch)}, kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const PlanePlan plan = plane_quality_plan(m_max);
  hipLaunchKernelGGL(k_plane_quality_batch, dim3(count), dim3(kPlaneQualityThreads), plan.lds_bytes, stream, d_src, d_dst,
                     d_items, r2, k, plan.list_threads, plan.shared_bytes, res);
  return hipGetLastError();
}

// The fields of section 13 from the root record, on the host (the batch's; the single calls form them with the same
// function, quality_plane.hip: same bits).
int plane_quality_result(size_t n, const NormalQualityPart &p, icp_plane_quality *q) {
  return normal_quality_result(n, p, q, &icp_plane_quality::plane_sum_r2, &icp_plane_quality::plane_rmse);
}

}  // namespace icp
