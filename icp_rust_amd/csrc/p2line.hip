// EXTENSION beyond the reference (include/icp_mi355x.h section 14): point-to-LINE residuals for 2-D handles, the planar
// counterpart of p2plane.hip ("PLICP").  tier4/icp_rust is point-to-point only, so NOTHING here has a reference
// counterpart and no parity claim is made.  The definition is p2plane.hip's with the third coordinate removed:
//   normal of a target q   = unit eigenvector of the smaller eigenvalue of the 2 x 2 covariance of the k targets nearest
//                            to q in the xy plane (q itself included; ordered by (d^2, index), d^2 = dx dx + dy dy), one
//                            Jacobi rotation of the pair (0, 1) in f64 (jacobi3's update sequence; skipped when
//                            a[0][1] == 0), the smaller diagonal (a tie: column 0), normalised by sqrt(n0 n0 + n1 n1),
//                            sign: first non-zero of (n_y, n_x) positive; fewer than 3 neighbours or zero length: zero;
//   residual of a pair     = n_q . (T p - q): ONE scalar per pair.
// The normals live in the handle's d_normals with a stride of 3 and nz = +0.0, the pairs are the PlanePair of
// p2plane_device.hpp with dz = 0, nz = 0: weights, Jacobian row, Huber error and the inner loop are p2plane.hip's own
// kernels (launch_p2pl_eval), untouched.  An independent numpy statement of the normals: tests/test_line_abi.py.
//   k_line_normals   one lane per target, Chebyshev rings of the 2-D grid (n[2] == 1, x cells finer by fx), k-best in LDS
//   k_line_gather    the pairs of all correspondences (src and dst with a stride of 2)
//   k_lngate_stage   the gate's first launch (gate_plane.hip's k_plgate_stage for a stride of 2); the place launch is
//                    gate_plane.hip's k_plgate_place itself
#include "api_internal.hpp"
#include "compact_device.hpp"
#include "p2line_device.hpp"
#include "p2plane_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

// (gate_plane.hip)
__global__ __launch_bounds__(kCompactThreads) void k_plgate_place(const double2 *__restrict__ st_pairs,
                                                                  const uint32_t *__restrict__ st_pos,
                                                                  const uint32_t *__restrict__ cnt,
                                                                  const uint32_t *__restrict__ sums, unsigned tiles,
                                                                  double2 *__restrict__ out_pairs,
                                                                  uint32_t *__restrict__ out_pos,
                                                                  unsigned *__restrict__ h_total);

constexpr unsigned kLinePairWords = sizeof(PlanePair) / sizeof(double2);
static_assert(sizeof(PlanePair) == 64 && kLinePairWords == 4, "a pair is four 16-byte words");

__global__ __launch_bounds__(64) void k_line_normals(const double *__restrict__ dst, unsigned m, GridParams g,
                                                     const uint32_t *__restrict__ start,
                                                     const GridPoint *__restrict__ pts, int kk,
                                                     double *__restrict__ normals, unsigned first) {
  __shared__ double s_d[64][kLineKMax];
  __shared__ uint32_t s_i[64][kLineKMax];
  const unsigned i = first + blockIdx.x * 64 + threadIdx.x;  // (targets [first, m): all of them, or the appended ones)
  if (i >= m) return;
  double *bd = s_d[threadIdx.x];
  uint32_t *bi = s_i[threadIdx.x];
  const double p[2] = {dst[(size_t)i * 2], dst[(size_t)i * 2 + 1]};
  int c[2];
  for (int d = 0; d < 2; ++d) {
    double t = floor((p[d] - g.lo[d]) * g.inv_h[d]);
    t = fmin(fmax(t, 0.), (double)(g.n[d] - 1));
    c[d] = (int)t;
  }
  int k = kk < (int)m ? kk : (int)m;
  k = k < kLineKMax ? k : kLineKMax;  // (the entries refuse k > 16: this only keeps the lists inside their rows)
  int cnt = 0;
  const int rmax = max(g.n[0], g.n[1]);
  for (int r = 1; r <= rmax; ++r) {
    cnt = 0;
    const int x0 = max(c[0] - r * g.fx, 0), x1 = min(c[0] + r * g.fx, g.n[0] - 1);
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.n[1] - 1);
    for (int iy = y0; iy <= y1; ++iy) {
      const uint32_t row = (uint32_t)iy * g.n[0];  // (a 2-D grid has one layer of cells: iz == 0)
      const uint32_t s = start[row + x0], e = start[row + x1 + 1];
      for (uint32_t j = s; j < e; ++j) {
        uint32_t ti = pts[j].idx;
        if (ti >= m) ti = 0;  // (a record's idx is always < m: this only keeps the reads in bounds)
        const double dx = p[0] - dst[(size_t)ti * 2], dy = p[1] - dst[(size_t)ti * 2 + 1];
        const double dd = dx * dx + dy * dy;
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
    for (int d = 0; d < 2; ++d) {
      const int w = d == 0 ? r * g.fx : r;
      if (c[d] - w > 0) cover = fmin(cover, p[d] - (g.lo[d] + (c[d] - w) * g.h[d]));
      if (c[d] + w < g.n[d] - 1) cover = fmin(cover, (g.lo[d] + (c[d] + w + 1) * g.h[d]) - p[d]);
    }
    if (cover == __builtin_huge_val()) break;  // the whole grid
    cover -= 1e-9 * (g.scale + fabs(p[0]) + fabs(p[1]));
    if (cnt == k && cover > 0. && bd[k - 1] < cover * cover) break;
  }
  double nrm[2];  // (the tail behind the k best: p2line_device.hpp, shared with the batch kernel)
  line_normal_of_neighbours(cnt, [&](int j, int d) { return dst[(size_t)bi[j] * 2 + d]; }, nrm);
  normals[(size_t)i * 3] = nrm[0];
  normals[(size_t)i * 3 + 1] = nrm[1];
  normals[(size_t)i * 3 + 2] = 0.;
}

__global__ void k_line_gather(const double *__restrict__ src, unsigned n, Pose T, const uint32_t *__restrict__ idx,
                              const double *__restrict__ dst, unsigned m, const double *__restrict__ normals,
                              PlanePair *__restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = src[(size_t)i * 2], y = src[(size_t)i * 2 + 1];
  uint32_t j = idx[i];
  if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the reads in bounds)
  PlanePair o;
  o.ax = (T.r00 * x + T.r01 * y) + T.tx;  // Transform::transform, src/transform.rs:22-24
  o.ay = (T.r10 * x + T.r11 * y) + T.ty;
  o.qx = dst[(size_t)j * 2];
  o.qy = dst[(size_t)j * 2 + 1];
  o.dz = 0.;
  o.nx = normals[(size_t)j * 3];
  o.ny = normals[(size_t)j * 3 + 1];
  o.nz = 0.;
  out[i] = o;
}

// gate_plane.hip's k_plgate_stage with the clouds read at a stride of 2: d2 = ex ex + ey ey (section 9's rule in the
// plane), dz = 0, nz = 0
__global__ __launch_bounds__(kCompactThreads) void k_lngate_stage(const double *__restrict__ src, unsigned n, Pose T,
                                                                  const uint32_t *__restrict__ idx,
                                                                  const double *__restrict__ dst, unsigned m,
                                                                  const double *__restrict__ normals, double r2,
                                                                  double2 *__restrict__ st_pairs,
                                                                  uint32_t *__restrict__ st_pos,
                                                                  uint32_t *__restrict__ cnt) {
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  const unsigned tid = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  double2 w0[kCompactRounds], w1[kCompactRounds], w2[kCompactRounds];
  unsigned rank[kCompactRounds];
  bool keep[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + tid;
    bool in = false;
    w0[k] = w1[k] = w2[k] = make_double2(0., 0.);
    if (i < n) {
      const double px = src[i * 2], py = src[i * 2 + 1];
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      uint32_t j = idx[i];
      if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the reads in bounds)
      const double *t = dst + (size_t)j * 2, *nj = normals + (size_t)j * 3;
      const double bx = t[0], by = t[1];
      const double ex = qx - bx, ey = qy - by;
      const double d2 = ex * ex + ey * ey;
      in = d2 <= r2;  // (false for a NaN d2)
      w0[k] = make_double2(qx, qy);  // PlanePair: ax, ay | qx, qy | dz, nx | ny, nz
      w1[k] = make_double2(bx, by);
      w2[k] = make_double2(nj[0], nj[1]);
    }
    rank[k] = compact_wave_rank(__ballot(in), wcnt[k]);
    keep[k] = in;
  }
  __syncthreads();
  unsigned total = 0;
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    unsigned before = 0;
    compact_round_offset(before, wcnt[k], total);
    if (!keep[k]) continue;
    const size_t at = first + before + rank[k];  // (< first + the tile's points: inside the tile's own segment)
    double2 *o = st_pairs + at * kLinePairWords;
    o[0] = w0[k];
    o[1] = w1[k];
    o[2] = make_double2(0., w2[k].x);
    o[3] = make_double2(w2[k].y, 0.);
    if (st_pos) st_pos[at] = (uint32_t)(first + k * kCompactThreads + tid);
  }
  if (tid == 0) cnt[blockIdx.x] = total;
}

hipError_t launch_line_normals(icp_handle *h, int k, double *d_normals, size_t first) {
  const unsigned m = (unsigned)h->m;
  if (first >= h->m) return hipSuccess;
  hipLaunchKernelGGL(k_line_normals, dim3((m - (unsigned)first + 63) / 64), dim3(64), 0, h->stream, h->d_dst, m, h->grid.p,
                     (const uint32_t *)h->grid.d_start, (const GridPoint *)h->grid.d_pts, k, d_normals, (unsigned)first);
  return hipGetLastError();
}

hipError_t launch_line_gather(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx,
                              const double *d_normals, void *d_pairs) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_line_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_src, (unsigned)n, T, d_idx,
                     h->d_dst, (unsigned)h->m, d_normals, (PlanePair *)d_pairs);
  return hipGetLastError();
}

namespace api {

// launch_gate_plane (gate_plane.hip) for a 2-D handle: same scratch, same place launch, same count (gate_count)
hipError_t launch_gate_line(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx, double r2,
                            void *d_pairs, uint32_t *d_kept) {
  Workspace &w = h->ws;
  w.h_res->pad = 0;
  if (n == 0) return hipSuccess;
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  // (cap_n >= 256 doubles per residual buffer: tiles + chunks words fit -- a word per 1 024 points and one per 2^23)
  uint32_t *cnt = reinterpret_cast<uint32_t *>(w.d_ry), *sums = cnt + tiles;
  uint32_t *st_pos = d_kept ? reinterpret_cast<uint32_t *>(w.d_rx) : nullptr;
  double2 *st = reinterpret_cast<double2 *>(h->d_plane_stage);
  hipLaunchKernelGGL(k_lngate_stage, dim3(tiles), dim3(kCompactThreads), 0, h->stream, d_src, (unsigned)n, T, d_idx,
                     h->d_dst, (unsigned)h->m, (const double *)h->d_normals, r2, st, st_pos, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (chunks > 1 && (e = launch_compact_chunks(cnt, tiles, sums, h->stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_plgate_place, dim3(tiles), dim3(kCompactThreads), 0, h->stream, (const double2 *)st,
                     (const uint32_t *)st_pos, (const uint32_t *)cnt, (const uint32_t *)sums, tiles,
                     reinterpret_cast<double2 *>(d_pairs), d_kept, &w.h_res->pad);
  return hipGetLastError();
}

}  // namespace api
}  // namespace icp
