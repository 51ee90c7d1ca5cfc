// What the kernels that compute line normals share (p2line.hip: k_line_normals, through the target grid;
// p2line_batch.hip: k_line_estimate_batch and quality_line.hip: k_line_quality_batch, a sweep over the workgroup's own
// targets): everything behind the k best neighbours -- ONE statement of include/icp_mi355x.h section 14's mean,
// covariance, Jacobi rotation, column choice, normalisation and sign, so that they cannot drift apart -- and, for the
// two one-workgroup kernels, the sweep itself.
#pragma once
#include "common.hpp"
#include "tiny_device.hpp"

namespace icp {

constexpr int kLineKMax = 16;

// The line normal from the `cnt` neighbours found, in their (d^2, index) order: coord(j, d) is coordinate d of the j-th.
// Fewer than 3 neighbours, or a zero-length eigenvector: the zero vector.
template <class Coord>
__device__ __forceinline__ void line_normal_of_neighbours(int cnt, Coord coord, double nrm[2]) {
  nrm[0] = nrm[1] = 0.;
  if (cnt < 3) return;
  double mean[2] = {0., 0.};
  for (int j = 0; j < cnt; ++j)
    for (int d = 0; d < 2; ++d) mean[d] = mean[d] + coord(j, d);
  for (int d = 0; d < 2; ++d) mean[d] = mean[d] / (double)cnt;
  double a[2][2] = {{0., 0.}, {0., 0.}};
  for (int j = 0; j < cnt; ++j) {
    double e[2];
    for (int d = 0; d < 2; ++d) e[d] = coord(j, d) - mean[d];
    for (int r = 0; r < 2; ++r)
      for (int s = 0; s < 2; ++s) a[r][s] = a[r][s] + e[r] * e[s];
  }
  double v[2][2] = {{1., 0.}, {0., 1.}};
  if (a[0][1] != 0.) {  // jacobi3's rotation of the pair (p, q) = (0, 1): it diagonalises a 2 x 2
    const double theta = (a[1][1] - a[0][0]) / (2. * a[0][1]);
    const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
    const double cs = 1. / sqrt(t * t + 1.), sn = t * cs;
    for (int q = 0; q < 2; ++q) {  // A <- A J (columns 0, 1)
      const double a0 = a[q][0], a1 = a[q][1];
      a[q][0] = cs * a0 - sn * a1;
      a[q][1] = sn * a0 + cs * a1;
    }
    for (int q = 0; q < 2; ++q) {  // A <- J^T A (rows 0, 1)
      const double a0 = a[0][q], a1 = a[1][q];
      a[0][q] = cs * a0 - sn * a1;
      a[1][q] = sn * a0 + cs * a1;
    }
    for (int q = 0; q < 2; ++q) {
      const double v0 = v[q][0], v1 = v[q][1];
      v[q][0] = cs * v0 - sn * v1;
      v[q][1] = sn * v0 + cs * v1;
    }
  }
  const int col = a[1][1] < a[0][0] ? 1 : 0;  // the smaller eigenvalue; a tie: column 0
  double n0 = v[0][col], n1 = v[1][col];
  const double len = sqrt(n0 * n0 + n1 * n1);
  if (len > 0.) {
    n0 = n0 / len;
    n1 = n1 / len;
    const double lead = n1 != 0. ? n1 : n0;
    if (lead < 0.) {
      n0 = -n0;
      n1 = -n1;
    }
    nrm[0] = n0;
    nrm[1] = n1;
  }
}

// ---- the line normals of a workgroup's own targets (the one-workgroup kernels: k_line_estimate_batch,
// k_line_quality_batch) ----
// Per target the k best by (d^2, index) from a sweep outwards over the targets SORTED BY x in LDS (tiny_sort_targets;
// exact: the k-nearest set under that order is unique), L targets per round with their lists in `shared` ((8 + 4) B x
// kLineKMax x L, free again on return), then line_normal_of_neighbours -> nrm[sorted position].  kk: the entries' k,
// clamped here to m.  Every thread of the workgroup calls it; it ends with a barrier.
__device__ __forceinline__ void line_normals_of_sorted_targets(const TinyTargets &tg, double cx, double cy, double scale,
                                                               int kk, unsigned L, unsigned char *shared, double2 *nrm) {
  const unsigned tid = threadIdx.x, m = tg.m;
  const double *tx = tg.tx, *ty = tg.ty;
  const float4 *g4 = tg.g4;
  double *ld = reinterpret_cast<double *>(shared);                // [kLineKMax][L]: d^2
  uint32_t *li = reinterpret_cast<uint32_t *>(ld + kLineKMax * L);  // [kLineKMax][L]: (index << 16) | sorted position
  int k = kk < (int)m ? kk : (int)m;
  k = k < kLineKMax ? k : kLineKMax;  // (the entries refuse k > 16: this only keeps the lists inside their rows)
  for (unsigned base = 0; base < m; base += L) {
    const unsigned j = base + tid;
    if (tid < L && j < m) {
      double *bd = ld + tid;
      uint32_t *bi = li + tid;
      const double x = tx[j], y = ty[j];
      const float4 own = g4[j];
      const double ec = tiny_screen_margin(x - cx, y - cy, 0., scale);
      // The k best are kept UNORDERED while the sweep runs, with the worst of them -- its (d^2, index) and its slot --
      // in registers: a candidate is refused without touching the list, an accepted one replaces the worst and the
      // new worst is found by k independent reads (a sorted insertion is a chain of dependent LDS accesses as long as
      // the deepest insertion among the wave's 64 lanes).  They are ordered once, after the sweep.
      float thr = __builtin_huge_valf();  // the screen's bound: the worst kept distance once k are kept
      double wd = __builtin_huge_val();
      uint32_t wi = 0xffffffffu;
      int wq = 0, cnt = 0;
      auto offer = [&](unsigned jj, unsigned orig) {
        const double dx = x - tx[jj], dy = y - ty[jj];
        const double dd = dx * dx + dy * dy;
        const uint32_t ti = (orig << 16) | jj;  // (index and position below 2^16: ordered as the indices are)
        if (cnt == k && !(dd < wd || (dd == wd && ti < wi))) return;
        const int at = cnt < k ? cnt : wq;
        bd[at * L] = dd;
        bi[at * L] = ti;
        if (cnt < k) ++cnt;
        if (cnt == k) {
          wd = bd[0];
          wi = bi[0];
          wq = 0;
          for (int q = 1; q < k; ++q) {
            const double dq = bd[q * L];
            const uint32_t iq = bi[q * L];
            if (dq > wd || (dq == wd && iq > wi)) {
              wd = dq;
              wi = iq;
              wq = q;
            }
          }
          thr = tiny_screen_bound(wd, ec);
        }
      };
      // outwards from the target's own position while a target's x alone does not rule it out: the f32 difference is
      // within ec of the true one and thr carries that margin, so fx^2 > thr  =>  strictly farther than the k-th best.
      // Four targets per step, their LDS reads in flight together (as tiny_nearest); unlike a nearest-neighbour
      // search a list must not be offered a target twice, so a step's slots past either end are masked, not repeated.
      auto visit = [&](const float4 g, unsigned jj, bool valid) {
        const float fx = own.x - g.x, fy = own.y - g.y;
        if (valid && !(__builtin_fmaf(fy, fy, fx * fx) > thr)) offer(jj, __float_as_uint(g.w));
      };
      offer(j, __float_as_uint(own.w));
      for (unsigned jj = j + 1; jj < m; jj += 4) {  // (g4 carries four +inf pads past mp)
        const float4 g0 = g4[jj], g1 = g4[jj + 1], g2 = g4[jj + 2], g3 = g4[jj + 3];
        const float f0 = own.x - g0.x;
        if (f0 * f0 > thr) break;  // sorted by x: everything further right is farther still
        visit(g0, jj, true);
        visit(g1, jj + 1, jj + 1 < m);
        visit(g2, jj + 2, jj + 2 < m);
        visit(g3, jj + 3, jj + 3 < m);
      }
      for (unsigned jj = j; jj > 0;) {
        const unsigned j0 = jj - 1, j1 = jj > 1 ? jj - 2 : 0, j2 = jj > 2 ? jj - 3 : 0, j3 = jj > 3 ? jj - 4 : 0;
        const float4 g0 = g4[j0], g1 = g4[j1], g2 = g4[j2], g3 = g4[j3];
        const float f0 = own.x - g0.x;
        if (f0 * f0 > thr) break;
        visit(g0, j0, true);
        visit(g1, j1, jj > 1);
        visit(g2, j2, jj > 2);
        visit(g3, j3, jj > 3);
        jj = j3;
      }
      // the (d^2, index) order: entry q's rank is the number of entries before it (the pairs are distinct); its
      // sorted position then goes where its d^2 was, at slot `rank` (every rank is known before the first is written)
      unsigned long long ranks = 0;
      for (int q = 0; q < cnt; ++q) {
        const double dq = bd[q * L];
        const uint32_t iq = bi[q * L];
        unsigned r = 0;
        for (int u = 0; u < cnt; ++u) {
          const double du = bd[u * L];
          const uint32_t iu = bi[u * L];
          r += (du < dq || (du == dq && iu < iq)) ? 1u : 0u;
        }
        ranks |= (unsigned long long)r << (4 * q);
      }
      for (int q = 0; q < cnt; ++q)
        bd[((ranks >> (4 * q)) & 15u) * L] = __longlong_as_double((long long)(bi[q * L] & 0xffffu));
      double nv[2];
      line_normal_of_neighbours(cnt, [&](int q, int d) {
        const unsigned pos = (unsigned)__double_as_longlong(bd[q * L]);
        return d == 0 ? tx[pos] : ty[pos];
      }, nv);
      nrm[j] = make_double2(nv[0], nv[1]);
    }
  }
  __syncthreads();
}

}  // namespace icp
