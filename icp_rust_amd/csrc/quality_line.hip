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
//                         into LDS, their line normals (p2line_device.hpp: the sweep k_line_estimate_batch runs), the
//                         exact nearest neighbour of every moved source point (tiny_nearest), the same terms and the tree
//                         of a batch item, fold_workgroup, as k_quality_batch folds it (api_batch.hip drives it)
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.
#include "p2line_device.hpp"
#include "quality_device.hpp"
#include "tiny_device.hpp"

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

// ---- the LDS plan of a batch launch ----
// per workgroup, for its item's m targets (mp = m rounded up to 64): x | y (f64), the f32 screen records (+ 4 pads), the
// normals, as k_line_estimate_batch keeps them; then ONE shared region, sized by the launch; then the control words.
// The shared region holds, one after the other: the target sort's keys (8 B x the next power of two of m), the k-best
// lists of the normals ((8 + 4) B x 16 per list-holding thread), and then the fold's group (FoldLds<10>) with the four
// group records behind it: the fold aliases the lists, which are dead by then.  The rounds of the normals hold as many
// lists as the grant leaves room for: 640 at m = 668, 320 at m = 2048, the estimate kernel's.
namespace {

constexpr unsigned kLineQualityThreads = 1024;
constexpr size_t kLineQualityListBytes = kLineKMax * (sizeof(double) + sizeof(uint32_t));
constexpr size_t kLineQualityFoldBytes =
    sizeof(FoldLds<kNormalQualitySums>) + (kLineQualityMaxN / kFoldGroup) * sizeof(LineQualityPart);
constexpr size_t kLineQualityCtlBytes = 256;
struct LineQualityCtl {
  unsigned pos0;  // the sorted position of the target of original index 0
  int bail;       // a NaN target: the single call decides what such a cloud is
};
static_assert(sizeof(LineQualityCtl) <= kLineQualityCtlBytes, "the control words' share of the LDS");
constexpr size_t line_quality_fixed_bytes(unsigned m) {
  const size_t mp = (m + 63u) & ~63u;
  return mp * 2 * sizeof(double) + (mp + 4) * sizeof(float4) + mp * sizeof(double2) + kLineQualityCtlBytes;
}
struct LineQualityPlan {
  unsigned list_threads, shared_bytes;
  size_t lds_bytes;
};
constexpr LineQualityPlan line_quality_plan(unsigned m_max) {
  const size_t fixed = line_quality_fixed_bytes(m_max);
  size_t keys = 64;
  while (keys < m_max) keys <<= 1;
  const size_t fit = (kTinyLdsGrant - fixed) / kLineQualityListBytes / 64 * 64;
  size_t lists = (m_max + 63u) & ~63u;  // (a list per target is all a round can use)
  lists = lists < kLineQualityThreads ? lists : kLineQualityThreads;
  lists = lists < fit ? lists : fit;
  size_t shared = lists * kLineQualityListBytes;
  shared = shared > keys * 8 ? shared : keys * 8;
  shared = shared > kLineQualityFoldBytes ? shared : kLineQualityFoldBytes;
  return LineQualityPlan{(unsigned)lists, (unsigned)shared, fixed + shared};
}
static_assert(kLineQualityFoldBytes == 23936 && kLineQualityFoldBytes % 16 == 0, "a group of the tree and four records");
static_assert(kLineQualityThreads / 64 * 6 * sizeof(double) <= line_quality_fixed_bytes(1), "the box's wave minima");
// the plan at its corners: the smallest item (the fold sizes the region), a golden scan (two rounds of 640), the
// largest item (rounds of 320)
static_assert(line_quality_plan(1).list_threads == 64 && line_quality_plan(1).shared_bytes == kLineQualityFoldBytes, "m = 1");
static_assert(line_quality_plan(668).list_threads == 640 && line_quality_plan(668).shared_bytes == 640 * 192 &&
                  line_quality_plan(668).lds_bytes == 156992,
              "m = 668");
static_assert(line_quality_plan(kLineQualityMaxM).list_threads == 320 &&
                  line_quality_plan(kLineQualityMaxM).shared_bytes == 320 * 192 &&
                  line_quality_plan(kLineQualityMaxM).lds_bytes == 160064 &&
                  line_quality_plan(kLineQualityMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048");

}  // namespace

// One item per workgroup, a thread per source point (1 <= n <= 1024, 1 <= m <= 2048: api_batch.hip, LineQualityKind).
// Hand-backs (the item's record is left as the host preset it, pad != 0): a box that is not finite, a NaN target.
__global__ __launch_bounds__(kLineQualityThreads) void k_line_quality_batch(const double *__restrict__ src_all,
                                                                            const double *__restrict__ dst_all,
                                                                            const QualityBatchItem *__restrict__ items,
                                                                            double r2, int kk, unsigned L,
                                                                            unsigned shared_bytes,
                                                                            LineQualityPart *__restrict__ res) {
  constexpr unsigned B = kLineQualityThreads;
  extern __shared__ unsigned char lds_raw[];
  const QualityBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m, tid = threadIdx.x;
  const double *__restrict__ src = src_all + item.src_first * 2;
  const double *__restrict__ dst = dst_all + item.dst_first * 2;

  double cx, cy, cz, scale;  // (cz: +0.0 in two dimensions)
  if (!tiny_batch_box<2, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) return;
  // ---- LDS carve-up ----  (targets are kept SORTED BY x: position j below is not the target's index)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  unsigned char *p = reinterpret_cast<unsigned char *>(ty + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y relative to the box centre as f32, -, original index}
  p += sizeof(float4) * (mp + 4);
  double2 *nrm = reinterpret_cast<double2 *>(p);  // the line normal of the target at sorted position j
  p += sizeof(double2) * mp;
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then the fold (line_quality_plan)
  p += shared_bytes;
  LineQualityCtl *C = reinterpret_cast<LineQualityCtl *>(p);
  const TinyTargets tg = {tx, ty, nullptr, g4, m};

  if (tid == 0) {
    C->pos0 = 0;
    C->bail = 0;
  }
  tiny_sort_targets<2, B>(dst, cx, cy, cz, reinterpret_cast<unsigned long long *>(shared), tg,
                          [&](unsigned j, unsigned k, double x, double y) {
                            if (k == 0) C->pos0 = j;
                            if ((x != x) | (y != y)) C->bail = 1;
                          });
  if (C->bail) return;  // (uniform)
  line_normals_of_sorted_targets(tg, cx, cy, scale, kk, L, shared, nrm);

  // ---- transform, exact nearest neighbour from a cold start, the ten terms ----
  double v[kNormalQualitySums] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (tid < n) {
    const double px = src[(size_t)tid * 2], py = src[(size_t)tid * 2 + 1];
    const double qx = (item.T.r00 * px + item.T.r01 * py) + item.T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (item.T.r10 * px + item.T.r11 * py) + item.T.ty;
    unsigned nb, nbo;  // sorted position / original index of the nearest target
    tiny_nearest<2>(tg, qx, qy, 0., cx, cy, cz, scale, 0xffffffffu, &nb, &nbo);
    if (nb == 0xffffffffu) nb = C->pos0;  // no finite distance (NaN query): index 0, as a scan from 0 would
    const double2 nq = nrm[nb];
    const double q[2] = {qx, qy}, b[2] = {tx[nb], ty[nb]}, nn[2] = {nq.x, nq.y};
    normal_quality_terms<2>(q, b, nn, r2, v, in, nan);
  }
  // ---- the tree of a batch item, k_quality_batch's ----
  // (the normals' lists are dead since the barrier behind their last round: the fold takes their place)
  FoldLds<kNormalQualitySums> &F = *reinterpret_cast<FoldLds<kNormalQualitySums> *>(shared);
  LineQualityPart *grp = reinterpret_cast<LineQualityPart *>(shared + sizeof(FoldLds<kNormalQualitySums>));
  fold_workgroup(F, grp, tid, n, v, in, nan, &res[item.slot]);
}

hipError_t launch_line_quality_batch(unsigned m_max, const double *d_src, const double *d_dst,
                                     const QualityBatchItem *d_items, unsigned count, double r2, int k,
                                     LineQualityPart *res, hipStream_t stream, bool *granted) {
  // the grant above 64 KB of dynamic LDS, asked once per process; refused: nothing launches
  static TinyLdsGrant grant;
  *granted = grant.ask({reinterpret_cast<const void *>(&k_line_quality_batch)}, kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const LineQualityPlan plan = line_quality_plan(m_max);
  hipLaunchKernelGGL(k_line_quality_batch, dim3(count), dim3(kLineQualityThreads), plan.lds_bytes, stream, d_src, d_dst,
                     d_items, r2, k, plan.list_threads, plan.shared_bytes, res);
  return hipGetLastError();
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
