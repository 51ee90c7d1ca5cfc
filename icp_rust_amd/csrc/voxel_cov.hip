// EXTENSION beyond the reference (include/icp_mi355x.h section 26): voxel covariances -- per occupied voxel the mean of its
// points and the second moments about that mean, packed xx, xy, yy / xx, xy, xz, yy, yz, zz, with section 25's count,
// lowest index and point-to-voxel map.  Membership, order and the means' bits are section 25's (voxel_mean.hip runs the
// chain up to the sort; this file takes the sorted members from there); a second moment is the fold tree of section 9 over
// the products (x_a - m_a) (x_b - m_b) of the members in ascending index, divided once by c - ddof.
//   k_vc_fold<DIM>   k_vm_fold's body with the second moments switched on (voxel_fold_device.hpp): for a voxel up to 32
//                    members the members stay in the lanes of its group, the mean comes back from the group's lane 0, and
//                    the products run through the same narrow tree; 33 .. 256: the wave reads the members a second time,
//                    now less the mean; above: the same work lists, no second moments yet
//   k_vm_items, k_vm_top (voxel_mean.hip's, by its launcher)  the means of the voxels above 256 members
//   k_vc_items<DIM>  the items again, read-only now: the products of the deviations from the finished mean, two levels of
//                    the tree per workgroup; a voxel of one item is done, a larger one leaves a record of NS sums
//   k_vc_top<DIM>    a workgroup per voxel above 65 536 members: two more levels over its records
// The records of the means are read by k_vm_top before k_vc_items overwrites them (one stream).  No float atomics.
#include "voxel_device.hpp"
#include "voxel_fold_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vc_fold(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                                        const uint32_t *__restrict__ start, uint32_t *__restrict__ ctr,
                                                        double *__restrict__ mean, uint32_t *__restrict__ count,
                                                        uint4 *__restrict__ items, uint4 *__restrict__ bigs,
                                                        double *__restrict__ cov, uint32_t ddof) {
  vm_fold_body<DIM, vm_pairs(DIM)>(pts, perm, start, ctr, mean, count, items, bigs, cov, ddof);
}

template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vc_items(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ start, const uint32_t *__restrict__ ctr,
                                                         const uint4 *__restrict__ items, const double *__restrict__ mean,
                                                         double *__restrict__ cov, double *__restrict__ rec, uint32_t ddof) {
  __shared__ double part[vm_pairs(DIM)][kFoldGroup];  // (3-D: 12 KB)
  vm_items_body<DIM, vm_pairs(DIM)>(part, pts, perm, start, ctr, items, mean, cov, rec, ddof);
}

template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vc_top(const uint32_t *__restrict__ start, const uint32_t *__restrict__ ctr,
                                                       const uint4 *__restrict__ bigs, const double *__restrict__ rec,
                                                       double *__restrict__ cov, uint32_t ddof) {
  __shared__ double part[vm_pairs(DIM)][kFoldGroup];
  vm_top_body<vm_pairs(DIM)>(part, start, ctr, bigs, rec, cov, ddof);
}

namespace {

template <int DIM>
hipError_t covariance_chain(VoxelWs &W, const double *d_pts, size_t n, uint32_t ddof, double *d_cov, double *d_mean,
                            uint32_t *d_count, hipStream_t s) {
  hipError_t e = launch_vm_starts(W, n, s);
  if (e != hipSuccess) return e;
  const unsigned fold_blocks = (unsigned)((n + kVmWaves * 64 - 1) / (kVmWaves * 64));
  hipLaunchKernelGGL(k_vc_fold<DIM>, dim3(fold_blocks), dim3(kVmThreads), 0, s, d_pts, (const uint32_t *)W.perm,
                     (const uint32_t *)W.start, W.ctr, d_mean, d_count, W.items, W.bigs, d_cov, ddof);
  if ((e = hipGetLastError()) != hipSuccess || n <= kFoldGroup) return e;  // (no voxel above 256 members)
  if ((e = launch_vm_large_means(W, DIM, d_pts, n, d_mean, s)) != hipSuccess) return e;
  const size_t most = n / (kFoldGroup + 1) + n / kVmChunk + 1;
  hipLaunchKernelGGL(k_vc_items<DIM>, dim3((unsigned)(most < kVmItemBlocks ? most : kVmItemBlocks)), dim3(kVmThreads), 0, s,
                     d_pts, (const uint32_t *)W.perm, (const uint32_t *)W.start, (const uint32_t *)W.ctr,
                     (const uint4 *)W.items, (const double *)d_mean, d_cov, W.rec, ddof);
  if ((e = hipGetLastError()) != hipSuccess || n <= kVmChunk) return e;
  const size_t most_bigs = n / kVmChunk;
  hipLaunchKernelGGL(k_vc_top<DIM>, dim3((unsigned)(most_bigs < kVmTopBlocks ? most_bigs : kVmTopBlocks)), dim3(kVmThreads),
                     0, s, (const uint32_t *)W.start, (const uint32_t *)W.ctr, (const uint4 *)W.bigs,
                     (const double *)W.rec, d_cov, ddof);
  return hipGetLastError();
}

// the arguments of both entries, all decided before the device is touched (a refused call writes nothing)
bool covariance_args_ok(int dim, const void *pts, size_t n, double v, int ddof, const void *cov, const size_t *voxels,
                        int device) {
  return voxel_args_ok(dim, pts, n, v, voxels) && device >= -1 && (ddof == 0 || ddof == 1) && cov && n <= kVmMaxPoints;
}

}  // namespace

hipError_t launch_covariance_chain(VoxelWs &W, int dim, const double *d_pts, size_t n, int ddof, double *d_cov,
                                   double *d_mean, uint32_t *d_count, hipStream_t s) {
  return dim == 3 ? covariance_chain<3>(W, d_pts, n, (uint32_t)ddof, d_cov, d_mean, d_count, s)
                  : covariance_chain<2>(W, d_pts, n, (uint32_t)ddof, d_cov, d_mean, d_count, s);
}

}  // namespace icp

extern "C" int icp_voxel_covariances_device(int dim, const double *d_pts, size_t n, double voxel, int ddof, double *d_cov,
                                            double *d_mean, uint32_t *d_count, uint32_t *d_first_index,
                                            uint32_t *d_voxel_of, size_t *voxels, int device, void *hip_stream) {
  if (!covariance_args_ok(dim, d_pts, n, voxel, ddof, d_cov, voxels, device)) return ICP_BAD_ARGUMENT;
  *voxels = 0;
  ICP_TRY_RC(voxel_device(&device));
  if (n == 0) return ICP_OK;
  std::lock_guard<std::mutex> lk(voxel_mutex());
  VoxelWs &W = voxel_ws(device);
  if (!d_mean) {  // the second moments are about the means: into the workspace
    HIP_TRY(reserve(W.out, W.cap_out, n * dim));
    d_mean = W.out;
  }
  return voxel_centroids_on(W, dim, d_pts, n, voxel, d_mean, d_count, d_first_index, d_voxel_of, voxels,
                            (hipStream_t)hip_stream, d_cov, ddof);
}

extern "C" int icp_voxel_covariances(int dim, const double *pts, size_t n, double voxel, int ddof, double *cov, double *mean,
                                     uint32_t *count, uint32_t *first_index, uint32_t *voxel_of, size_t *voxels,
                                     int device) {
  if (!covariance_args_ok(dim, pts, n, voxel, ddof, cov, voxels, device)) return ICP_BAD_ARGUMENT;
  *voxels = 0;
  ICP_TRY_RC(voxel_device(&device));
  if (n == 0) return ICP_OK;
  std::lock_guard<std::mutex> lk(voxel_mutex());
  VoxelWs &W = voxel_ws(device);
  const size_t ns = (size_t)vm_pairs(dim);
  if (!W.stream) HIP_TRY(hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking));
  HIP_TRY(reserve(W.in, W.cap_in, n * dim));
  HIP_TRY(reserve(W.out, W.cap_out, n * dim));
  HIP_TRY(reserve(W.cov, W.cap_cov, n * ns));
  if (count) HIP_TRY(reserve(W.count, W.cap_count, n));
  if (first_index) HIP_TRY(reserve(W.idx, W.cap_idx, n));
  if (voxel_of) HIP_TRY(reserve(W.of, W.cap_of, n));
  HIP_TRY(hipMemcpyAsync(W.in, pts, n * dim * sizeof(double), hipMemcpyHostToDevice, W.stream));
  ICP_TRY_RC(voxel_centroids_on(W, dim, W.in, n, voxel, W.out, count ? W.count : nullptr, first_index ? W.idx : nullptr,
                                voxel_of ? W.of : nullptr, voxels, W.stream, W.cov, ddof));
  const size_t k = *voxels;
  if (k) HIP_TRY(hipMemcpyAsync(cov, W.cov, k * ns * sizeof(double), hipMemcpyDeviceToHost, W.stream));
  if (mean && k) HIP_TRY(hipMemcpyAsync(mean, W.out, k * dim * sizeof(double), hipMemcpyDeviceToHost, W.stream));
  if (count && k) HIP_TRY(hipMemcpyAsync(count, W.count, k * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  if (first_index && k) HIP_TRY(hipMemcpyAsync(first_index, W.idx, k * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  if (voxel_of) HIP_TRY(hipMemcpyAsync(voxel_of, W.of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  HIP_TRY(hipStreamSynchronize(W.stream));
  return ICP_OK;
}
