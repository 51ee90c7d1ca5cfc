// EXTENSION beyond the reference (include/icp_mi355x.h section 16): the quality of a pose under the point-to-LINE
// residual of section 14 -- fitness, inlier RMSE, line RMSE, error / huber_error of the line residual and the SE(2)
// information matrix that residual gives -- at a GIVEN pose, for a 2-D handle with current line normals, as a single
// call and as a batch.  Section 13 (quality_plane.hip) with the third coordinate removed.
//   k_line_quality_terms  one workgroup per 256 source points: a lane gathers src[i], idx[i], dst[j], nrm[j] once (52 B),
//                         forms the ten terms of section 16, and the group folds them by the tree of section 9
//                         (fold_device.hpp) into one 96-byte record
//   k_fold_level<10>      the next level of the same tree: one workgroup per 256 records (as many launches as levels)
//   k_line_quality_batch  one workgroup per item of icp_batch_evaluate_point_to_line: the item's box, its targets sorted
//                         into LDS, their line normals (p2line_device.hpp: the sweep k_line_estimate_batch runs), the
//                         exact nearest neighbour of every moved source point (tiny_nearest), the same terms and the same
//                         tree as k_quality_batch folds it (api_batch.hip drives it)
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.
#include <cmath>
#include <cstring>

#include "api_internal.hpp"
#include "fold_device.hpp"
#include "gn_device.hpp"
#include "p2line_device.hpp"
#include "tiny_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace {

static_assert(sizeof(LineQualityPart) == 96, "twelve doubles per record: ceil(n / 256) of them fit in max(n, 256)");

// A point's terms: the expressions of section 16 (the library is built with -ffp-contract=off: no FMA).  q is the moved
// source point, b the matched target, (nx, ny) its line normal.  plane_residual (p2plane_device.hpp) adds a trailing
// + nz dz = + 0.0 to rp; the square does not see it (it only turns a -0.0 into +0.0), so it is left out here.
__device__ __forceinline__ void line_quality_terms(double qx, double qy, double bx, double by, double nx, double ny,
                                                   double r2, double v[kLineQualitySums], unsigned &in, unsigned &nan) {
  const double ex = qx - bx, ey = qy - by;
  const double d2 = ex * ex + ey * ey;  // the 2-D icp_evaluate's d2
  const bool inl = d2 <= r2;            // (false for a NaN d2)
  const double rp = nx * ex + ny * ey;
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

}  // namespace

// level 1: the terms of source points [256 g, 256 g + 256), folded -> out[g].  n == 1: out[0] is the one point's terms
// (the fold of one value is the value: no +0.0 added, a -0.0 stays).  src and dst at a stride of 2; the normals at the
// stride of 3 they are stored with (nz = +0.0 is there and is not read).
__global__ __launch_bounds__(256) void k_line_quality_terms(const double *__restrict__ src, unsigned n, Pose T,
                                                            const uint32_t *__restrict__ idx,
                                                            const double *__restrict__ dst,
                                                            const double *__restrict__ nrm, unsigned m, double r2,
                                                            LineQualityPart *__restrict__ out) {
  __shared__ FoldLds<kLineQualitySums> L;
  const unsigned tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kFoldGroup + tid;
  double v[kLineQualitySums] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (i < n) {
    const double px = src[i * 2], py = src[i * 2 + 1];
    const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (T.r10 * px + T.r11 * py) + T.ty;
    uint32_t j = idx[i];
    if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the reads in bounds)
    const double *b = dst + (size_t)j * 2, *nj = nrm + (size_t)j * 3;
    line_quality_terms(qx, qy, b[0], b[1], nj[0], nj[1], r2, v, in, nan);
  }
  if (n == 1) {
    if (tid == 0) out[0] = fold_part(v, in, nan);
    return;
  }
  fold_put(L, tid, v, in, nan);
  fold_group(L, tid);
  if (tid == 0) out[blockIdx.x] = fold_take(L);
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
    sizeof(FoldLds<kLineQualitySums>) + (kLineQualityMaxN / kFoldGroup) * sizeof(LineQualityPart);
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

// One item per workgroup, a thread per source point (1 <= n <= 1024, 1 <= m <= 2048: api_batch.hip, line_quality_fits).
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
  double v[kLineQualitySums] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (tid < n) {
    const double px = src[(size_t)tid * 2], py = src[(size_t)tid * 2 + 1];
    const double qx = (item.T.r00 * px + item.T.r01 * py) + item.T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (item.T.r10 * px + item.T.r11 * py) + item.T.ty;
    unsigned nb, nbo;  // sorted position / original index of the nearest target
    tiny_nearest<2>(tg, qx, qy, 0., cx, cy, cz, scale, 0xffffffffu, &nb, &nbo);
    if (nb == 0xffffffffu) nb = C->pos0;  // no finite distance (NaN query): index 0, as a scan from 0 would
    const double2 nq = nrm[nb];
    line_quality_terms(qx, qy, tx[nb], ty[nb], nq.x, nq.y, r2, v, in, nan);
  }
  if (n == 1) {  // (uniform across the workgroup)
    if (tid == 0) res[item.slot] = fold_part(v, in, nan);
    return;
  }
  // ---- the tree over each group of 256 points, then over the (up to four) group records: k_quality_batch's ----
  // (the normals' lists are dead since the barrier behind their last round: the fold takes their place)
  FoldLds<kLineQualitySums> &F = *reinterpret_cast<FoldLds<kLineQualitySums> *>(shared);
  LineQualityPart *grp = reinterpret_cast<LineQualityPart *>(shared + sizeof(FoldLds<kLineQualitySums>));
  const unsigned groups = (n + kFoldGroup - 1) / kFoldGroup;
  for (unsigned g = 0; g < groups; ++g) {
    const unsigned lane = tid - g * kFoldGroup;  // (wraps for the threads below the group: never < kFoldGroup then)
    if (lane < kFoldGroup) fold_put(F, lane, v, in, nan);
    fold_group(F, tid);
    if (tid == 0) grp[g] = fold_take(F);
    __syncthreads();
  }
  if (groups == 1) {
    if (tid == 0) res[item.slot] = grp[0];
    return;
  }
  if (tid < kFoldGroup) {
    if (tid < groups) fold_put(F, tid, grp[tid].v, grp[tid].inliers, grp[tid].nan);
    else fold_put_zero(F, tid);
  }
  fold_group(F, tid);
  if (tid == 0) res[item.slot] = fold_take(F);
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

// n and zeros: what *out holds unless a result replaces it
void line_quality_clear(size_t n, icp_line_quality *q) {
  std::memset(q, 0, sizeof(*q));
  q->n = n;
}

// The fields of section 16 from the root record, on the host (both entries and the batch share it: same bits).
int line_quality_result(size_t n, const LineQualityPart &p, icp_line_quality *q) {
  line_quality_clear(n, q);
  if (n == 0) return ICP_OK;
  if (p.nan) return ICP_NAN_INPUT;  // (the estimator's rule: a NaN residual)
  q->inliers = p.inliers;
  q->fitness = (double)p.inliers / (double)n;
  q->inlier_sum_d2 = p.v[0];
  q->inlier_rmse = p.inliers ? std::sqrt(p.v[0] / (double)p.inliers) : 0.;
  q->line_sum_r2 = p.v[1];
  q->line_rmse = p.inliers ? std::sqrt(p.v[1] / (double)p.inliers) : 0.;
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

namespace {

// What both entries decide before any work, in the order section 16 gives: the arguments, n == 0, the device, and only
// then the handle.  *done: the status is final.
int line_evaluate_enter(icp_handle *h, const void *src, size_t n, const icp_pose *T, double max_dist,
                        icp_line_quality *out, bool *done) {
  *done = true;
  if (out) line_quality_clear(n, out);
  if (!sized_args_ok(h, src, n, T, max_dist, out)) return ICP_BAD_ARGUMENT;
  if (n == 0) return ICP_OK;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->dim != 2 || h->normals_m != h->m) return ICP_BAD_ARGUMENT;  // icp_compute_target_line_normals first (again after an append)
  if (h->m == 0) return ICP_EMPTY_DST;
  *done = false;
  return ICP_OK;
}

// The device part of both entries: the handle's search at T, then the terms and the tree.
int line_evaluate(icp_handle *h, const double *d_src, size_t n, const Pose &T, double max_dist, icp_line_quality *out,
                  uint32_t *d_idx) {
  Quiesce quiesce_on_exit{h};
  Workspace &w = h->ws;
  // (the level records live in the residual buffers: ceil(n / 256) records of 12 doubles fit in max(n, 256) doubles)
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  uint32_t *idx = d_idx ? d_idx : w.d_idx;
  ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &T));
  ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, nullptr, nullptr, idx));  // exact 2-D NN
  const double r2 = max_dist * max_dist;
  const unsigned k = (unsigned)((n + kFoldGroup - 1) / kFoldGroup);
  LineQualityPart *cur = reinterpret_cast<LineQualityPart *>(w.d_rx), *nxt = reinterpret_cast<LineQualityPart *>(w.d_ry);
  hipLaunchKernelGGL(k_line_quality_terms, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                     (const double *)h->d_normals, (unsigned)h->m, r2, cur);
  HIP_TRY(hipGetLastError());
  LineQualityPart r, *root;
  HIP_TRY(fold_levels(cur, nxt, k, h->stream, &root));
  HIP_TRY(hipMemcpyAsync(&r, root, sizeof(r), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return line_quality_result(n, r, out);
}

}  // namespace

extern "C" int icp_evaluate_point_to_line_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                                 double max_dist, icp_line_quality *out, uint32_t *d_idx) {
  bool done;
  const int rc = line_evaluate_enter(h, d_src, n, T, max_dist, out, &done);
  if (done) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return line_evaluate(h, d_src, n, *T, max_dist, out, d_idx);
}

extern "C" int icp_evaluate_point_to_line(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                                          icp_line_quality *out, uint32_t *idx) {
  bool done;
  const int erc = line_evaluate_enter(h, src, n, T, max_dist, out, &done);
  if (done) return erc;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int rc = line_evaluate(h, h->ws.d_src, n, *T, max_dist, out, h->ws.d_idx);
  if ((rc == ICP_OK || rc == ICP_NAN_INPUT) && idx) {  // (the search ran: its correspondences are there either way)
    HIP_TRY(hipMemcpyAsync(idx, h->ws.d_idx, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return rc;
}
