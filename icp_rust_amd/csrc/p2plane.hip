// EXTENSION beyond the reference (BASELINE.json configs[4]): point-to-plane
// residuals.  tier4/icp_rust is point-to-point only -- there is no normal, no plane, no neighbourhood
// anywhere in src/ (src/lib.rs:218-261) -- so NOTHING here has a reference counterpart and no parity
// claim is made.  What is kept from the reference is everything around the residual: the SE(2) pose on
// the xy-plane with z carried through (src/lib.rs:52-57), the exact nearest neighbour in 3-D
// (:161-167), the Huber / MAD weighting with the same constants and the same inner loop with its two
// break tests (:59-84, :218-261, src/huber.rs, src/stats.rs), the 3x3 adjugate solve and Transform::new.
// Definition (an independent CPU statement of it is the checker of tests/test_p2plane.py):
//   normal of a target q   = unit eigenvector of the smallest eigenvalue of the covariance of the k
//                            targets nearest to q (q itself included; ties by lowest index), cyclic
//                            Jacobi in f64, sign: first non-zero of (n_z, n_y, n_x) positive;
//   residual of a pair     = n_q . (T p - q), T p = (R p_xy + t, p_z): ONE scalar per pair;
//   weights                = sigma = 1.4826 MAD(r), g = 1 / sigma, w = drho(r^2, 1.345), skipped when
//                            sigma == 0, exactly as the reference treats each of its two rows;
//   Jacobian row           = n_xy^T [R | R (-a_y, a_x)^T] with the reference's jacobian() (:176-184);
//   Huber error            = sum rho(r^2).
// Point-to-LINE residuals for 2-D handles (include/icp_mi355x.h section 14, "PLICP") are the same definition with the
// third coordinate removed:
//   normal of a target q   = unit eigenvector of the smaller eigenvalue of the 2 x 2 covariance of the k targets nearest
//                            to q in the xy plane (q itself included; ordered by (d^2, index), d^2 = dx dx + dy dy), one
//                            Jacobi rotation of the pair (0, 1) in f64 (jacobi3's update sequence; skipped when
//                            a[0][1] == 0), the smaller diagonal (a tie: column 0), normalised by sqrt(n0 n0 + n1 n1),
//                            sign: first non-zero of (n_y, n_x) positive; fewer than 3 neighbours or zero length: zero.
// The normals live in the handle's d_normals with a stride of 3 and nz = +0.0, the pairs are the PlanePair of
// p2plane_device.hpp with dz = 0, nz = 0: weights, Jacobian row, Huber error and the inner loop are the kernels below
// (launch_p2pl_eval), which do not know the dimension.  An independent numpy statement of the line normals:
// tests/test_line_abi.py.
//   k_target_normals / k_line_normals   one lane per target, Chebyshev rings of the grid, k-best in LDS
//   k_p2pl_gather / k_line_gather       the pairs of all correspondences (src and dst with a stride of 3 / 2)
// One body behind each pair of kernels: normal_single_device.hpp.
#include "common.hpp"
#include "gn_device.hpp"
#include "normal_single_device.hpp"
#include "p2plane_device.hpp"

namespace icp {
__global__ void k_final_reduce(const double *__restrict__ partials, int blocks, int nacc,
                               const GnScalars *__restrict__ scal, GnResult *__restrict__ res);

// (jacobi3 and everything behind the k best neighbours: p2plane_device.hpp, plane_normal_of_neighbours; the 2-D twin:
// p2line_device.hpp, line_normal_of_neighbours; the bodies of the four kernels below: normal_single_device.hpp)

__global__ __launch_bounds__(64) void k_target_normals(const double *__restrict__ dst, unsigned m, GridParams g,
                                                       const uint32_t *__restrict__ start,
                                                       const GridPoint *__restrict__ pts, int kk,
                                                       double *__restrict__ normals, unsigned first) {
  target_normals_by_grid<3>(dst, m, g, start, pts, kk, normals, first);
}

__global__ __launch_bounds__(64) void k_line_normals(const double *__restrict__ dst, unsigned m, GridParams g,
                                                     const uint32_t *__restrict__ start,
                                                     const GridPoint *__restrict__ pts, int kk,
                                                     double *__restrict__ normals, unsigned first) {
  target_normals_by_grid<2>(dst, m, g, start, pts, kk, normals, first);
}

__global__ void k_p2pl_gather(const double *__restrict__ src, unsigned n, Pose T, const uint32_t *__restrict__ idx,
                              const double *__restrict__ dst, const double *__restrict__ normals,
                              PlanePair *__restrict__ out) {
  normal_gather<3>(src, n, T, idx, dst, 0u, normals, out);  // (m: only the 2-D gather clamps by it)
}

__global__ void k_line_gather(const double *__restrict__ src, unsigned n, Pose T, const uint32_t *__restrict__ idx,
                              const double *__restrict__ dst, unsigned m, const double *__restrict__ normals,
                              PlanePair *__restrict__ out) {
  normal_gather<2>(src, n, T, idx, dst, m, normals, out);
}

// residuals as the pairs ((r, 0), (0, 0)): launch_stddevs (gn_pull.hip, the full key) under the identity pose then
// selects the exact median and MAD of r (dimension 0); dimension 1 is all zeros
__global__ void k_p2pl_residual(const PlanePair *__restrict__ pp, unsigned n, Pose T, double2 *__restrict__ fa,
                                double2 *__restrict__ fb) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fa[i] = make_double2(plane_residual(pp[i], T), 0.);
  fb[i] = make_double2(0., 0.);
}

__global__ __launch_bounds__(kReduceThreads) void k_p2pl_accumulate(const PlanePair *__restrict__ pp, unsigned n, Pose T,
                                                                    const GnScalars *__restrict__ scal,
                                                                    double *__restrict__ partials) {
  double acc[kNAcc];
#pragma unroll
  for (int k = 0; k < kNAcc; ++k) acc[k] = 0.;
  const double sigma = scal->sigma[0];
  const double gw = 1. / sigma;
  const unsigned G = gridDim.x * kReduceThreads;
  for (unsigned i = blockIdx.x * kReduceThreads + threadIdx.x; i < n; i += G) {
    const PlanePair p = pp[i];
    const double r = plane_residual(p, T);
    const double e = r * r;
    if (sigma != 0.) {  // src/lib.rs:243-245
      const double a0 = -p.ay, a1 = p.ax;  // jacobian(), src/lib.rs:176-184
      const double b0 = T.r00 * a0 + T.r01 * a1;
      const double b1 = T.r10 * a0 + T.r11 * a1;
      const double J[3] = {p.nx * T.r00 + p.ny * T.r10, p.nx * T.r01 + p.ny * T.r11, p.nx * b0 + p.ny * b1};
      const double wg = huber_drho(e) * gw;
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[9 + k] = acc[9 + k] + (wg * J[k]) * r;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[3 * a + b] = acc[3 * a + b] + (wg * J[a]) * J[b];
    }
    acc[12] = acc[12] + huber_rho(e);
  }
  block_reduce_store<kNAcc>(acc, partials + (size_t)blockIdx.x * (kNAcc + 1));
}

// the normals of the targets [first, m) with the kernel of the handle's dimension (m x 3 either way)
hipError_t launch_normals(icp_handle *h, int k, double *d_normals, size_t first) {
  const unsigned m = (unsigned)h->m;
  if (first >= h->m) return hipSuccess;
  hipLaunchKernelGGL(h->dim == 3 ? k_target_normals : k_line_normals, dim3((m - (unsigned)first + 63) / 64), dim3(64), 0,
                     h->stream, h->d_dst, m, h->grid.p, (const uint32_t *)h->grid.d_start, (const GridPoint *)h->grid.d_pts, k,
                     d_normals, (unsigned)first);
  return hipGetLastError();
}

hipError_t launch_normal_gather(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx,
                                const double *d_normals, void *d_pairs) {
  if (n == 0) return hipSuccess;  // (an empty scan: no pair, and a grid of no workgroups is not a launch)
  const dim3 blocks((unsigned)((n + 255) / 256));
  if (h->dim == 3)
    hipLaunchKernelGGL(k_p2pl_gather, blocks, dim3(256), 0, h->stream, d_src, (unsigned)n, T, d_idx, h->d_dst, d_normals,
                       (PlanePair *)d_pairs);
  else
    hipLaunchKernelGGL(k_line_gather, blocks, dim3(256), 0, h->stream, d_src, (unsigned)n, T, d_idx, h->d_dst,
                       (unsigned)h->m, d_normals, (PlanePair *)d_pairs);
  return hipGetLastError();
}

// one evaluation: result in h->ws.h_res after the stream is synchronised (acc[0..8] jtj, [9..11] jtr, [12] error)
hipError_t launch_p2pl_eval(icp_handle *h, const void *d_pairs, size_t n_, const Pose &T, double *d_fa, double *d_fb) {
  Workspace &w = h->ws;
  const unsigned n = (unsigned)n_;
  hipError_t e;
  hipLaunchKernelGGL(k_p2pl_residual, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const PlanePair *)d_pairs, n, T,
                     (double2 *)d_fa, (double2 *)d_fb);
  if (w.gn_dirty) {  // (first use, or a NaN left its flag behind: the caller sets it when it reads one)
    if ((e = launch_sel_init(h, n_)) != hipSuccess) return e;
    w.gn_dirty = false;
  }
  // (the full key: dimension 1 is n equal keys, which no candidate list holds)
  if ((e = launch_stddevs(h, d_fa, d_fb, n_, transform_identity())) != hipSuccess) return e;
  int blocks, threads;
  reduce_geometry(n_, &blocks, &threads);
  hipLaunchKernelGGL(k_p2pl_accumulate, dim3(blocks), dim3(threads), 0, h->stream, (const PlanePair *)d_pairs, n, T,
                     (const GnScalars *)w.d_scal, w.d_partials);
  hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(kReduceThreads), 0, h->stream, (const double *)w.d_partials, blocks,
                     kNAcc, (const GnScalars *)w.d_scal, w.h_res);
  return hipGetLastError();
}

size_t p2pl_pair_bytes() { return sizeof(PlanePair); }

}  // namespace icp
