// What the point-to-plane kernels share (p2plane.hip: gather, residual, accumulate; gate_plane.hip: the gate that writes
// the same pairs for the inliers only): the per-pair constants of an inner loop and the residual over them.
// Also: everything behind the k best neighbours of a target (the rounds that find them among a workgroup's own targets,
// for the one-workgroup kernels of p2plane_batch.hip and quality_plane_batch.hip, are normal_batch_device.hpp:
// normals_of_sorted_targets<3>).
#pragma once
#include "common.hpp"
#include "tiny_device.hpp"

namespace icp {

// per pair: everything the inner loop needs that does not change with the inner pose
struct PlanePair {
  double ax, ay;        // xy(T_outer p)
  double qx, qy, dz;    // matched target xy, p_z - q_z
  double nx, ny, nz;    // its normal
};

__device__ __forceinline__ double plane_residual(const PlanePair &p, const Pose &T) {
  const double rx = ((T.r00 * p.ax + T.r01 * p.ay) + T.tx) - p.qx;
  const double ry = ((T.r10 * p.ax + T.r11 * p.ay) + T.ty) - p.qy;
  return (p.nx * rx + p.ny * ry) + p.nz * p.dz;
}

// ---- everything behind the k best neighbours of a target (p2plane.hip: k_target_normals, through the target grid;
// p2plane_batch.hip: k_plane_estimate_batch, a sweep over the workgroup's own targets): ONE statement of the mean, the
// covariance, the Jacobi sweeps, the column choice, the normalisation and the sign, so that the two cannot drift apart.

// cyclic Jacobi on a symmetric 3x3 (a: upper triangle used, row-major full), eigenvectors in the
// columns of v.  Fixed operation order (the CPU restatement runs the same sequence).
__device__ inline void jacobi3(double a[3][3], double v[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1. : 0.;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = (a[0][1] * a[0][1] + a[0][2] * a[0][2]) + a[1][2] * a[1][2];
    if (off == 0.) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.) continue;
        const double theta = (a[q][q] - a[p][p]) / (2. * a[p][q]);
        const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
        const double c = 1. / sqrt(t * t + 1.), s = t * c;
        for (int k = 0; k < 3; ++k) {  // A <- A J (columns p, q)
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {  // A <- J^T A (rows p, q)
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// The plane normal from the `cnt` neighbours found, in their (d^2, index) order: coord(j, d) is coordinate d of the j-th.
// Fewer than 3 neighbours, or a zero-length eigenvector: the zero vector.
template <class Coord>
__device__ __forceinline__ void plane_normal_of_neighbours(int cnt, Coord coord, double nrm[3]) {
  nrm[0] = nrm[1] = nrm[2] = 0.;
  if (cnt >= 3) {
    double mean[3] = {0., 0., 0.};
    for (int j = 0; j < cnt; ++j)
      for (int d = 0; d < 3; ++d) mean[d] = mean[d] + coord(j, d);
    for (int d = 0; d < 3; ++d) mean[d] = mean[d] / (double)cnt;
    double a[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
    for (int j = 0; j < cnt; ++j) {
      double e[3];
      for (int d = 0; d < 3; ++d) e[d] = coord(j, d) - mean[d];
      for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s) a[r][s] = a[r][s] + e[r] * e[s];
    }
    double v[3][3];
    jacobi3(a, v);
    int col = 0;  // smallest eigenvalue; ties -> lowest column
    if (a[1][1] < a[0][0]) col = 1;
    if (a[2][2] < (col == 1 ? a[1][1] : a[0][0])) col = 2;
    // (column `col` of v by selects: indexed by a variable, v would live in scratch memory)
    double n0 = col == 2 ? v[0][2] : (col == 1 ? v[0][1] : v[0][0]);
    double n1 = col == 2 ? v[1][2] : (col == 1 ? v[1][1] : v[1][0]);
    double n2 = col == 2 ? v[2][2] : (col == 1 ? v[2][1] : v[2][0]);
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (len > 0.) {
      n0 = n0 / len;
      n1 = n1 / len;
      n2 = n2 / len;
      const double lead = n2 != 0. ? n2 : (n1 != 0. ? n1 : n0);
      if (lead < 0.) {
        n0 = -n0;
        n1 = -n1;
        n2 = -n2;
      }
      nrm[0] = n0;
      nrm[1] = n1;
      nrm[2] = n2;
    }
  }
}

}  // namespace icp
