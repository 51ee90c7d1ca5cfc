// What the kernels that compute line normals share (p2plane.hip: k_line_normals, through the target grid;
// p2line_batch.hip: k_line_estimate_batch and quality_line.hip: k_line_quality_batch, a sweep over the workgroup's own
// targets, normal_batch_device.hpp: normals_of_sorted_targets<2>): everything behind the k best neighbours -- ONE
// statement of include/icp_mi355x.h section 14's mean, covariance, Jacobi rotation, column choice, normalisation and
// sign, so that they cannot drift apart.
#pragma once
#include "common.hpp"
#include "tiny_device.hpp"

namespace icp {

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

}  // namespace icp
