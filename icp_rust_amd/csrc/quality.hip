// EXTENSION beyond the reference (include/icp_mi355x.h section 9): the quality of a pose -- fitness, inlier RMSE, the
// reference's error / huber_error and the SE(2) information matrix at a GIVEN pose, with the handle's own exact search.
//   k_quality_terms<DIM>  one workgroup per 256 source points: each point's terms from src, T, idx and dst, folded by the
//                         tree of section 9 (fold_device.hpp) into one record per group
//   k_fold_level<6>       the next level of the same tree: one workgroup per 256 records (as many launches as levels)
//   k_quality_batch<DIM>  one workgroup per item of icp_batch_evaluate: the item's targets in LDS, exact brute-force
//                         nearest neighbour in f64, the same terms and the same tree (api_batch.hip drives it)
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.
#include <cmath>
#include <cstring>

#include "api_internal.hpp"
#include "fold_device.hpp"
#include "gn_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace {

// A point's terms: the expressions of section 9 (the library is built with -ffp-contract=off: no FMA).  b is the
// matched target; d2 is the search's distance expression, e2 its xy part.
template <int DIM>
__device__ __forceinline__ void quality_terms(double qx, double qy, double qz, double bx, double by, double bz, double r2,
                                              double v[kQualitySums], unsigned &in, unsigned &nan) {
  const double ex = qx - bx, ey = qy - by;
  const double e2 = ex * ex + ey * ey;
  double d2 = e2;
  if (DIM == 3) {
    const double dz = qz - bz;
    d2 = d2 + dz * dz;
  }
  const bool inl = d2 <= r2;  // (false for a NaN d2)
  v[0] = inl ? d2 : 0.;
  v[1] = e2;
  v[2] = huber_rho(e2);
  v[3] = inl ? qx : 0.;
  v[4] = inl ? qy : 0.;
  v[5] = inl ? qx * qx + qy * qy : 0.;
  in = inl ? 1u : 0u;
  nan = (e2 != e2) ? 1u : 0u;
}

}  // namespace

// level 1: the terms of source points [256 g, 256 g + 256), folded -> out[g].  n == 1: out[0] is the one point's terms
// (the fold of one value is the value: no +0.0 added, a -0.0 stays).
template <int DIM>
__global__ __launch_bounds__(256) void k_quality_terms(const double *__restrict__ src, unsigned n, Pose T,
                                                       const uint32_t *__restrict__ idx, const double *__restrict__ dst,
                                                       unsigned m, double r2, QualityPart *__restrict__ out) {
  __shared__ FoldLds<kQualitySums> L;
  const unsigned tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kFoldGroup + tid;
  double v[kQualitySums] = {0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (i < n) {
    const double px = src[i * DIM], py = src[i * DIM + 1];
    const double pz = DIM == 3 ? src[i * DIM + 2] : 0.;
    const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (T.r10 * px + T.r11 * py) + T.ty;
    uint32_t j = idx[i];
    if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the read in bounds)
    const double *b = dst + (size_t)j * DIM;
    quality_terms<DIM>(qx, qy, pz, b[0], b[1], DIM == 3 ? b[2] : 0., r2, v, in, nan);
  }
  if (n == 1) {
    if (tid == 0) out[0] = fold_part(v, in, nan);
    return;
  }
  fold_put(L, tid, v, in, nan);
  fold_group(L, tid);
  if (tid == 0) out[blockIdx.x] = fold_take(L);
}

// One item per workgroup, a thread per source point (n <= 1024): targets in LDS (SoA), the exact nearest neighbour by
// brute force in f64 with the handle's contract -- d2 = ((dx dx + dy dy) + dz dz), strictly smaller wins (ties -> the
// lowest index), a NaN distance never wins, no finite distance at all -> index 0 (as nn_brute.hip answers) -- then the
// terms, the tree over each group of 256 points, and the tree over the (up to four) group records.
template <int DIM>
__global__ __launch_bounds__(kQualityBatchThreads) void k_quality_batch(const double *__restrict__ src,
                                                                        const double *__restrict__ dst,
                                                                        const QualityBatchItem *__restrict__ items,
                                                                        double r2, QualityPart *__restrict__ res) {
  extern __shared__ double q_tgt[];  // x[m] | y[m] | z[m]
  __shared__ FoldLds<kQualitySums> L;
  __shared__ QualityPart grp[kQualityMaxN / kFoldGroup];
  const QualityBatchItem it = items[blockIdx.x];
  const unsigned n = it.n, m = it.m, tid = threadIdx.x;
  double *tx = q_tgt, *ty = tx + m, *tz = ty + m;
  const double *D = dst + it.dst_first * DIM;
  for (unsigned j = tid; j < m; j += kQualityBatchThreads) {
    tx[j] = D[(size_t)j * DIM];
    ty[j] = D[(size_t)j * DIM + 1];
    if (DIM == 3) tz[j] = D[(size_t)j * DIM + 2];
  }
  __syncthreads();
  double v[kQualitySums] = {0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (tid < n) {
    const double *p = src + (it.src_first + tid) * DIM;
    const double px = p[0], py = p[1], pz = DIM == 3 ? p[2] : 0.;
    const Pose T = it.T;
    const double qx = (T.r00 * px + T.r01 * py) + T.tx;
    const double qy = (T.r10 * px + T.r11 * py) + T.ty;
    double best = __builtin_huge_val();
    unsigned bi = 0xffffffffu;
    for (unsigned j = 0; j < m; ++j) {  // (every lane reads the same target: LDS broadcasts)
      const double dx = qx - tx[j], dy = qy - ty[j];
      double d = dx * dx + dy * dy;
      if (DIM == 3) {
        const double dz = pz - tz[j];
        d = d + dz * dz;
      }
      if (d < best) {
        best = d;
        bi = j;
      }
    }
    if (bi == 0xffffffffu) bi = 0;
    quality_terms<DIM>(qx, qy, pz, tx[bi], ty[bi], DIM == 3 ? tz[bi] : 0., r2, v, in, nan);
  }
  if (n == 1) {  // (uniform across the workgroup)
    if (tid == 0) res[it.slot] = fold_part(v, in, nan);
    return;
  }
  const unsigned groups = (n + kFoldGroup - 1) / kFoldGroup;
  for (unsigned g = 0; g < groups; ++g) {
    const unsigned lane = tid - g * kFoldGroup;  // (wraps for the threads below the group: never < kFoldGroup then)
    if (lane < kFoldGroup) fold_put(L, lane, v, in, nan);
    fold_group(L, tid);
    if (tid == 0) grp[g] = fold_take(L);
    __syncthreads();
  }
  if (groups == 1) {
    if (tid == 0) res[it.slot] = grp[0];
    return;
  }
  if (tid < kFoldGroup) {
    if (tid < groups) fold_put(L, tid, grp[tid].v, grp[tid].inliers, grp[tid].nan);
    else fold_put_zero(L, tid);
  }
  fold_group(L, tid);
  if (tid == 0) res[it.slot] = fold_take(L);
}

hipError_t launch_quality_batch(int dim, unsigned m_max, const double *d_src, const double *d_dst,
                                const QualityBatchItem *d_items, unsigned count, double r2, QualityPart *res,
                                hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const size_t lds = (size_t)m_max * (size_t)dim * sizeof(double);  // <= 48 KB; with the fold's 15 KB within 64 KB
  if (dim == 2)
    hipLaunchKernelGGL(k_quality_batch<2>, dim3(count), dim3(kQualityBatchThreads), lds, stream, d_src, d_dst, d_items,
                       r2, res);
  else
    hipLaunchKernelGGL(k_quality_batch<3>, dim3(count), dim3(kQualityBatchThreads), lds, stream, d_src, d_dst, d_items,
                       r2, res);
  return hipGetLastError();
}

// n and zeros: what *out holds unless a result replaces it
void quality_clear(size_t n, icp_quality *q) {
  std::memset(q, 0, sizeof(*q));
  q->n = n;
}

// The fields of section 9 from a folded record, on the host (both entries and the batch share it: same bits).
int quality_result(size_t n, const QualityPart &p, icp_quality *q) {
  quality_clear(n, q);
  if (n == 0) return ICP_OK;
  if (p.nan) return ICP_NAN_INPUT;  // (src/stats.rs:12's rule: a NaN residual)
  q->inliers = p.inliers;
  q->fitness = (double)p.inliers / (double)n;
  q->inlier_sum_d2 = p.v[0];
  q->inlier_rmse = p.inliers ? std::sqrt(p.v[0] / (double)p.inliers) : 0.;
  q->error = p.v[1];
  q->huber_error = p.v[2];
  const double c = (double)p.inliers, sx = p.v[3], sy = p.v[4], srr = p.v[5];
  const double info[9] = {c, 0., -sy, 0., c, sx, -sy, sx, srr};
  std::memcpy(q->information, info, sizeof(info));
  return ICP_OK;
}

}  // namespace icp

namespace {

// The device part of both entries: the handle's search at T, then the terms and the tree.
int evaluate(icp_handle *h, const double *d_src, size_t n, const Pose &T, double max_dist, icp_quality *out,
             uint32_t *d_idx) {
  Quiesce quiesce_on_exit{h};
  Workspace &w = h->ws;
  // (the level records live in the residual buffers: ceil(n / 256) records of 8 doubles fit in max(n, 256) doubles)
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  uint32_t *idx = d_idx ? d_idx : w.d_idx;
  ICP_TRY_RC(icp_prepare_source_device(h, d_src, n, &T));
  ICP_TRY_RC(icp_correspond_device(h, d_src, n, &T, w.d_a, w.d_b, idx));
  const double r2 = max_dist * max_dist;
  const unsigned k = (unsigned)((n + kFoldGroup - 1) / kFoldGroup);
  QualityPart *cur = reinterpret_cast<QualityPart *>(w.d_rx), *nxt = reinterpret_cast<QualityPart *>(w.d_ry);
  if (h->dim == 2)
    hipLaunchKernelGGL(k_quality_terms<2>, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                       (unsigned)h->m, r2, cur);
  else
    hipLaunchKernelGGL(k_quality_terms<3>, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                       (unsigned)h->m, r2, cur);
  HIP_TRY(hipGetLastError());
  QualityPart r, *root;
  HIP_TRY(fold_levels(cur, nxt, k, h->stream, &root));
  HIP_TRY(hipMemcpyAsync(&r, root, sizeof(r), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return quality_result(n, r, out);
}

}  // namespace

extern "C" int icp_evaluate_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T, double max_dist,
                                   icp_quality *out, uint32_t *d_idx) {
  if (!sized_args_ok(h, d_src, n, T, max_dist, out)) return ICP_BAD_ARGUMENT;
  quality_clear(n, out);
  if (n == 0) return ICP_OK;
  if (h->m == 0) return ICP_EMPTY_DST;  // index.unwrap() on an empty tree, src/lib.rs:122,165
  HIP_TRY(hipSetDevice(h->device));
  return evaluate(h, d_src, n, *T, max_dist, out, d_idx);
}

extern "C" int icp_evaluate(icp_handle *h, const double *src, size_t n, const icp_pose *T, double max_dist,
                            icp_quality *out, uint32_t *idx) {
  if (!sized_args_ok(h, src, n, T, max_dist, out)) return ICP_BAD_ARGUMENT;
  quality_clear(n, out);
  if (n == 0) return ICP_OK;
  if (h->m == 0) return ICP_EMPTY_DST;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), true));
  HIP_TRY(hipMemcpyAsync(h->ws.d_src, src, n * h->dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int rc = evaluate(h, h->ws.d_src, n, *T, max_dist, out, h->ws.d_idx);
  if ((rc == ICP_OK || rc == ICP_NAN_INPUT) && idx) {  // (the search ran: its correspondences are there either way)
    HIP_TRY(hipMemcpyAsync(idx, h->ws.d_idx, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return rc;
}
