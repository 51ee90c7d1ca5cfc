// EXTENSION beyond the reference (include/icp_mi355x.h section 9): the quality of a pose -- fitness, inlier RMSE, the
// reference's error / huber_error and the SE(2) information matrix at a GIVEN pose, with the handle's own exact search.
//   k_quality_terms<DIM>  one workgroup per 256 source points: each point's terms from src, T, idx and dst, folded by the
//                         tree of section 9 (fold_device.hpp) into one record per group; its body is the level 1 that
//                         all three qualities share (quality_device.hpp)
//   k_fold_level<6>       the next level of the same tree: one workgroup per 256 records (as many launches as levels)
//   k_quality_batch<DIM>  one workgroup per item of icp_batch_evaluate: the item's targets in LDS, exact brute-force
//                         nearest neighbour in f64, the same terms and the same tree (api_batch.hip drives it)
// Every sum is the fixed tree, so a result is a pure function of the inputs, whichever kernel computed it.  The single
// calls' driver, the staging of the host entry and the fields every quality shares: quality_device.hpp.
#include "quality_device.hpp"

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

// level 1 (quality_device.hpp: quality_level1) around the terms above
template <int DIM>
__global__ __launch_bounds__(256) void k_quality_terms(const double *__restrict__ src, unsigned n, Pose T,
                                                       const uint32_t *__restrict__ idx, const double *__restrict__ dst,
                                                       unsigned m, double r2, QualityPart *__restrict__ out) {
  quality_level1<DIM>(src, n, T, idx, m, out,
                      [=](const double *q, uint32_t j, double (&v)[kQualitySums], unsigned &in, unsigned &nan) {
                        const double *b = dst + (size_t)j * DIM;
                        quality_terms<DIM>(q[0], q[1], q[2], b[0], b[1], DIM == 3 ? b[2] : 0., r2, v, in, nan);
                      });
}

// One item per workgroup, a thread per source point (n <= 1024): targets in LDS (SoA), the exact nearest neighbour by
// brute force in f64 with the handle's contract -- d2 = ((dx dx + dy dy) + dz dz), strictly smaller wins (ties -> the
// lowest index), a NaN distance never wins, no finite distance at all -> index 0 (as nn_brute.hip answers) -- then the
// terms and the tree of a batch item (fold_device.hpp: fold_workgroup).
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
  fold_workgroup(L, grp, tid, n, v, in, nan, &res[it.slot]);
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

// The fields of section 9 from a folded record, on the host (both entries and the batch share it: same bits).
int quality_result(size_t n, const QualityPart &p, icp_quality *q) {
  int rc;
  if (!quality_head(n, p, q, &rc)) return rc;
  q->error = p.v[1];
  q->huber_error = p.v[2];
  const double c = (double)p.inliers, sx = p.v[3], sy = p.v[4], srr = p.v[5];
  const double info[9] = {c, 0., -sy, 0., c, sx, -sy, sx, srr};
  std::memcpy(q->information, info, sizeof(info));
  return ICP_OK;
}

}  // namespace icp

namespace {

// The device part of both entries: the handle's search at T (the pairs too), then the terms and the tree.
int evaluate(icp_handle *h, const double *d_src, size_t n, const Pose &T, double max_dist, icp_quality *out,
             uint32_t *d_idx) {
  const double r2 = max_dist * max_dist;
  QualityPart r;
  ICP_TRY_RC(evaluate_on_handle(h, d_src, n, T, d_idx, true, [&](const uint32_t *idx, unsigned k, QualityPart *cur) {
    if (h->dim == 2)
      hipLaunchKernelGGL(k_quality_terms<2>, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                         (unsigned)h->m, r2, cur);
    else
      hipLaunchKernelGGL(k_quality_terms<3>, dim3(k), dim3(kFoldGroup), 0, h->stream, d_src, (unsigned)n, T, idx, h->d_dst,
                         (unsigned)h->m, r2, cur);
  }, &r));
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
  return evaluate_staged(h, src, n, idx, [&](const double *d_src, uint32_t *d_idx) {
    return evaluate(h, d_src, n, *T, max_dist, out, d_idx);
  });
}
