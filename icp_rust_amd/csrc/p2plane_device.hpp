// What the point-to-plane kernels share (p2plane.hip: gather, residual, accumulate; gate_plane.hip: the gate that writes
// the same pairs for the inliers only): the per-pair constants of an inner loop and the residual over them.
#pragma once
#include "common.hpp"

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

}  // namespace icp
