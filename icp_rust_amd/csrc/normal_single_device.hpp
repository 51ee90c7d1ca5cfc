// What the single-handle kernels of the two normal residuals share -- point-to-plane on a 3-D handle (include/icp_mi355x.h
// section 7) and point-to-line on a 2-D one (section 14) -- beside normal_batch_device.hpp's NormalResidual<DIM> for the
// one-workgroup kernels: ONE body per piece, DIM = 2 or 3, so that the dimensions cannot drift apart.
//   grid_k_nearest<DIM, KMAX>     the ring search and the (d^2, index) insertion, shared with outlier.hip's lists
//   target_normals_by_grid<DIM>   k_target_normals / k_line_normals (p2plane.hip): one lane per target, its k nearest
//                                 targets through the grid, the normal from them
//   normal_gather<DIM>            k_p2pl_gather / k_line_gather (p2plane.hip): the pairs of all correspondences
//   normal_gate_stage<DIM>        k_plgate_stage / k_lngate_stage: in gate_plane.hip, beside the compaction it is built on
// The line definition is the plane's with the third coordinate removed: d^2 = dx dx + dy dy, one layer of cells, the
// 2 x 2 covariance (p2line_device.hpp), dz = nz = 0 in a pair.  The stored normal is m x 3 either way, nz = +0.0 in 2-D.
#pragma once
#include "common.hpp"
#include "p2line_device.hpp"
#include "p2plane_device.hpp"

namespace icp {

constexpr int kNormalKMax = kTinyKBestMax;  // the longest k-best list: the entries refuse k > 16
static_assert(kNormalKMax == 16, "icp_compute_target_normals / _line_normals accept 3 <= k <= 16");

// Where the kernels of the two dimensions differ in their GUARDS today (not in the definition).  Kept as they are --
// DESIGN.md section 9q lists them for a change of behaviour of its own.
template <int DIM>
struct NormalSingle {
  // a NaN d^2 is no neighbour (3-D); in 2-D it goes through the insertion like any other
  static constexpr bool kSkipNanDistance = DIM == 3;
  // a grid record's index >= m reads target 0, and k is held to the list length (2-D); neither in 3-D
  static constexpr bool kClampNeighbours = DIM == 2;
  // a correspondence j >= m gathers target 0 (2-D); not in 3-D.  (Both gate stages clamp.)
  static constexpr bool kClampGather = DIM == 2;
};

// The k nearest targets of the point p by (d^2, index), through the grid: Chebyshev rings of cells around p's own cell
// (x cells finer by fx; a 2-D grid has one layer, n[2] == 1) until the k-th distance is covered by the visited block.
// The running lists bd / bi (KMAX entries each, the caller's LDS row: dynamic indexing) end sorted; returns their
// length.  ONE body behind the normals kernels (KMAX = 16, guards of NormalSingle<DIM>) and the neighbour lists of
// section 23 (outlier.hip: KMAX = 16 or 32, the 3-D guards in both dimensions).  1 <= k <= min(KMAX, m) unless CLAMP.
template <int DIM, int KMAX, bool SKIP_NAN, bool CLAMP>
__device__ __forceinline__ int grid_k_nearest(const double *__restrict__ dst, unsigned m, const GridParams &g,
                                              const uint32_t *__restrict__ start, const GridPoint *__restrict__ pts,
                                              const double (&p)[DIM], int k, double *bd, uint32_t *bi) {
  int c[DIM];
  for (int d = 0; d < DIM; ++d) {
    double t = floor((p[d] - g.lo[d]) * g.inv_h[d]);
    t = fmin(fmax(t, 0.), (double)(g.n[d] - 1));
    c[d] = (int)t;
  }
  if (CLAMP) k = k < KMAX ? k : KMAX;  // (this only keeps the lists inside their rows)
  int cnt = 0;
  int rmax = max(g.n[0], g.n[1]);
  if (DIM == 3) rmax = max(rmax, g.n[2]);
  for (int r = 1; r <= rmax; ++r) {
    cnt = 0;
    const int x0 = max(c[0] - r * g.fx, 0), x1 = min(c[0] + r * g.fx, g.n[0] - 1);
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
    const int z0 = DIM == 3 ? max(c[DIM - 1] - r, 0) : 0, z1 = DIM == 3 ? min(c[DIM - 1] + r, g.n[2] - 1) : 0;
    for (int iz = z0; iz <= z1; ++iz)
      for (int iy = y0; iy <= y1; ++iy) {
        const uint32_t row = ((uint32_t)iz * g.n[1] + iy) * g.n[0];
        const uint32_t s = start[row + x0], e = start[row + x1 + 1];
        for (uint32_t j = s; j < e; ++j) {
          uint32_t ti = pts[j].idx;
          if (CLAMP && ti >= m) ti = 0;  // (a record's idx is always < m: this only keeps the reads in bounds)
          const double dx = p[0] - dst[(size_t)ti * DIM], dy = p[1] - dst[(size_t)ti * DIM + 1];
          double dd = dx * dx + dy * dy;
          if (DIM == 3) {
            const double dz = p[DIM - 1] - dst[(size_t)ti * DIM + 2];
            dd = dd + dz * dz;
          }
          // A NaN distance (a NaN coordinate in either target) is no neighbour: (d^2, index) does not order it, and a
          // list that took it in would depend on the order of the records inside a cell, which the grid's scatter
          // leaves to its atomics -- the normals of such a cloud would differ from one handle to the next.
          if (SKIP_NAN && dd != dd) continue;
          // insertion by (d^2, index) into the k best
          if (cnt == k && !(dd < bd[k - 1] || (dd == bd[k - 1] && ti < bi[k - 1]))) continue;
          int pos = cnt < k ? cnt : k - 1;
          while (pos > 0 && (dd < bd[pos - 1] || (dd == bd[pos - 1] && ti < bi[pos - 1]))) {
            bd[pos] = bd[pos - 1];
            bi[pos] = bi[pos - 1];
            --pos;
          }
          bd[pos] = dd;
          bi[pos] = ti;
          if (cnt < k) ++cnt;
        }
      }
    // is everything outside the visited block strictly farther than the k-th best?
    double cover = __builtin_huge_val();
    for (int d = 0; d < DIM; ++d) {
      const int w = d == 0 ? r * g.fx : r;
      if (c[d] - w > 0) cover = fmin(cover, p[d] - (g.lo[d] + (c[d] - w) * g.h[d]));
      if (c[d] + w < g.n[d] - 1) cover = fmin(cover, (g.lo[d] + (c[d] + w + 1) * g.h[d]) - p[d]);
    }
    if (cover == __builtin_huge_val()) break;  // the whole grid
    double mag = g.scale;
    for (int d = 0; d < DIM; ++d) mag = mag + fabs(p[d]);
    cover -= 1e-9 * mag;
    if (cnt == k && cover > 0. && bd[k - 1] < cover * cover) break;
  }
  return cnt;
}

// One lane per target: its k nearest targets through the grid (grid_k_nearest), then the covariance's smallest
// eigenvector.  The running k-best lists live in LDS (dynamic indexing).  Workgroups of 64.
template <int DIM>
__device__ __forceinline__ void target_normals_by_grid(const double *__restrict__ dst, unsigned m, const GridParams &g,
                                                       const uint32_t *__restrict__ start,
                                                       const GridPoint *__restrict__ pts, int kk,
                                                       double *__restrict__ normals, unsigned first) {
  using G = NormalSingle<DIM>;
  __shared__ double s_d[64][kNormalKMax];
  __shared__ uint32_t s_i[64][kNormalKMax];
  const unsigned i = first + blockIdx.x * 64 + threadIdx.x;  // (targets [first, m): all of them, or the appended ones)
  if (i >= m) return;
  double *bd = s_d[threadIdx.x];
  uint32_t *bi = s_i[threadIdx.x];
  double p[DIM];
  for (int d = 0; d < DIM; ++d) p[d] = dst[(size_t)i * DIM + d];
  const int k = kk < (int)m ? kk : (int)m;
  const int cnt = grid_k_nearest<DIM, kNormalKMax, G::kSkipNanDistance, G::kClampNeighbours>(dst, m, g, start, pts, p, k,
                                                                                             bd, bi);
  double nrm[3] = {0., 0., 0.};  // (the tails behind the k best: shared with the batch kernels)
  const auto coord = [&](int j, int d) { return dst[(size_t)bi[j] * DIM + d]; };
  if constexpr (DIM == 3)
    plane_normal_of_neighbours(cnt, coord, nrm);
  else
    line_normal_of_neighbours(cnt, coord, nrm);
  normals[(size_t)i * 3] = nrm[0];
  normals[(size_t)i * 3 + 1] = nrm[1];
  normals[(size_t)i * 3 + 2] = nrm[2];
}

// (PlanePair, the per-pair constants of an inner loop, and plane_residual: p2plane_device.hpp)
template <int DIM>
__device__ __forceinline__ void normal_gather(const double *__restrict__ src, unsigned n, const Pose &T,
                                              const uint32_t *__restrict__ idx, const double *__restrict__ dst, unsigned m,
                                              const double *__restrict__ normals, PlanePair *__restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = src[(size_t)i * DIM], y = src[(size_t)i * DIM + 1];
  uint32_t j = idx[i];
  if (NormalSingle<DIM>::kClampGather && j >= m) j = 0;  // (the search always answers j < m: this keeps the reads in bounds)
  PlanePair o;
  o.ax = (T.r00 * x + T.r01 * y) + T.tx;  // Transform::transform, src/transform.rs:22-24
  o.ay = (T.r10 * x + T.r11 * y) + T.ty;
  o.qx = dst[(size_t)j * DIM];
  o.qy = dst[(size_t)j * DIM + 1];
  o.dz = 0.;
  if (DIM == 3) o.dz = src[(size_t)i * DIM + 2] - dst[(size_t)j * DIM + 2];
  o.nx = normals[(size_t)j * 3];
  o.ny = normals[(size_t)j * 3 + 1];
  o.nz = DIM == 3 ? normals[(size_t)j * 3 + 2] : 0.;
  out[i] = o;
}

}  // namespace icp
