// EXTENSION beyond the reference (include/icp_mi355x.h section 25): voxel centroids -- per occupied voxel the mean of its
// points, their number, the lowest index, and per point the rank of its voxel.  Membership and order are voxel
// thinning's (section 22, voxel_device.hpp); a sum's bits are the fold tree of section 9 over the members in ascending
// index, so a result is a pure function of the input.
//   the chain  k_voxel_insert, k_voxel_mark, k_compact_chunks       as the thinning runs them (voxel.hip:
//                                                                   launch_voxel_front): w[i] = 0 for a voxel's lowest
//                                                                   index, cnt[tile]
//              k_vm_place       leader i of rank r: first_index[r] = i, w[i] = r (the marks become the leaders' ranks);
//                               compact_device.hpp's compact_place_tile with this rule
//              k_vm_key<DIM>    point i walks the table read-only to its leader: key[i] = voxel_of[i] = w[leader]; a
//                               dropped point: key n (sorts last), voxel_of 0xffffffff
//              stable_sort_cells (qsort.hip)  perm: the points by (rank, index) -- a voxel's members contiguous, ascending
//              k_vm_starts      where the key changes in sorted order: start[r]; start[voxels] = the finite points
//              k_vm_fold<DIM>   a lane per voxel reads its count; then by count: 1 -> the point's bytes; 2 .. 32 -> a
//                               group of 8, 16 or 32 lanes per voxel (several voxels of a wave at once); 33 .. 256 -> the
//                               wave; above -> a work item per 65 536 members (an integer atomic hands out list slots:
//                               the list's order varies, no value does)
//              k_vm_items<DIM>  a workgroup per item: its waves fold the groups of 256, wave 0 the group results; a voxel
//                               of one item is done, a larger one leaves a record per item
//              k_vm_top         a workgroup per voxel above 65 536 members: two more levels over its records
// The tree and the bodies of the three folding kernels are voxel_fold_device.hpp's: voxel_cov.hip (section 26) instantiates
// them with the second moments beside the means, and its entries run this file's chain (voxel_centroids_on) with its own
// folding launches in place of launch_centroid_chain.  No float atomics.
#include "api_internal.hpp"
#include "compact_device.hpp"
#include "voxel_device.hpp"
#include "voxel_fold_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

// leader i of rank r: first_index[r] = i (nullable), w[i] = r
__global__ __launch_bounds__(kCompactThreads) void k_vm_place(size_t n, uint32_t *__restrict__ w,
                                                              const uint32_t *__restrict__ cnt,
                                                              const uint32_t *__restrict__ sums,
                                                              uint32_t *__restrict__ first_index) {
  compact_place_tile(
      n, cnt, sums, [=](size_t i) { return w[i] != kCropGone; },
      [=](size_t i, size_t at, bool in) {
        if (!in) return;  // (a leader's at: < the voxels in all, which are <= n)
        if (first_index) first_index[at] = (uint32_t)i;
        w[i] = (uint32_t)at;
      });
}

// key[i] = the rank of point i's voxel (n for a point in none); voxel_of (nullable): the same, 0xffffffff for none
template <int DIM>
__global__ __launch_bounds__(kVoxelThreads) void k_vm_key(const double *__restrict__ pts, size_t n, double v,
                                                          const uint32_t *__restrict__ tab, size_t mask,
                                                          const uint32_t *__restrict__ w, uint32_t *__restrict__ key,
                                                          uint32_t *__restrict__ voxel_of) {
  const size_t i = (size_t)blockIdx.x * kVoxelThreads + threadIdx.x;
  if (i >= n) return;
  double c[3];
  uint32_t r = kCropGone;
  if (voxel_cell<DIM>(pts, i, v, c)) {
    const uint32_t leader = voxel_leader<DIM>(pts, n, v, tab, mask, i, c);
    if (leader < n) r = w[leader];
  }
  key[i] = r < n ? r : (uint32_t)n;
  if (voxel_of) voxel_of[i] = r < n ? r : kCropGone;
}

// start[r] = the sorted position of voxel r's first member, start[voxels] = the points that are in a voxel; ctr[kVmVoxels]
__global__ __launch_bounds__(kVoxelThreads) void k_vm_starts(const uint32_t *__restrict__ key,
                                                             const uint32_t *__restrict__ perm, size_t n,
                                                             uint32_t *__restrict__ start, uint32_t *__restrict__ ctr) {
  const size_t k = (size_t)blockIdx.x * kVoxelThreads + threadIdx.x;
  if (k >= n) return;
  const uint32_t gone = (uint32_t)n;
  const uint32_t kk = key[perm[k]];
  const uint32_t prev = k > 0 ? key[perm[k - 1]] : gone;
  if (kk < gone) {
    if (k == 0 || kk != prev) start[kk] = (uint32_t)k;
    if (k == n - 1) {
      start[kk + 1] = (uint32_t)n;  // (kk + 1 <= n: start has n + 1 words)
      ctr[kVmVoxels] = kk + 1;
    }
  } else if (k == 0 || prev != gone) {  // the first point that is in no voxel
    const uint32_t voxels = k == 0 ? 0u : prev + 1u;
    start[voxels] = (uint32_t)k;
    ctr[kVmVoxels] = voxels;
  }
}

// mean and count (each nullable) of the voxels up to 256 members; the work lists of the others
template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vm_fold(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                                        const uint32_t *__restrict__ start, uint32_t *__restrict__ ctr,
                                                        double *__restrict__ mean, uint32_t *__restrict__ count,
                                                        uint4 *__restrict__ items, uint4 *__restrict__ bigs) {
  vm_fold_body<DIM, 0>(pts, perm, start, ctr, mean, count, items, bigs, nullptr, 0u);
}

// an item: members [kVmChunk j, kVmChunk (j + 1)) of its voxel -> the voxel's mean (one item) or the item's record
template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vm_items(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ start, const uint32_t *__restrict__ ctr,
                                                         const uint4 *__restrict__ items, double *__restrict__ mean,
                                                         double *__restrict__ rec) {
  __shared__ double part[DIM][kFoldGroup];
  vm_items_body<DIM, 0>(part, pts, perm, start, ctr, items, nullptr, mean, rec, 0u);
}

// a voxel above kVmChunk members: the tree's third and fourth level over its at most 65 536 records
template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vm_top(const uint32_t *__restrict__ start, const uint32_t *__restrict__ ctr,
                                                       const uint4 *__restrict__ bigs, const double *__restrict__ rec,
                                                       double *__restrict__ mean) {
  __shared__ double part[DIM][kFoldGroup];
  vm_top_body<DIM>(part, start, ctr, bigs, rec, mean, 0u);
}

namespace {

// the arguments of both entries, all decided before the device is touched (a refused call writes nothing)
bool centroid_args_ok(int dim, const void *pts, size_t n, double v, const void *mean, const void *count, const size_t *voxels,
                      int device) {
  return voxel_args_ok(dim, pts, n, v, voxels) && device >= -1 && !((mean || count) && n > kVmMaxPoints);
}

unsigned bit_width(size_t x) {
  unsigned b = 0;
  while (x) {
    ++b;
    x >>= 1;
  }
  return b;
}

// the means of the voxels above 256 members, from the lists k_vm_fold (or voxel_cov.hip's k_vc_fold) left
template <int DIM>
hipError_t launch_large_means(VoxelWs &W, const double *d_pts, size_t n, double *d_mean, hipStream_t s) {
  if (n <= kFoldGroup) return hipSuccess;  // (no voxel above 256 members)
  hipError_t e;
  const size_t most = n / (kFoldGroup + 1) + n / kVmChunk + 1;
  hipLaunchKernelGGL(k_vm_items<DIM>, dim3((unsigned)(most < kVmItemBlocks ? most : kVmItemBlocks)), dim3(kVmThreads), 0, s,
                     d_pts, (const uint32_t *)W.perm, (const uint32_t *)W.start, (const uint32_t *)W.ctr,
                     (const uint4 *)W.items, d_mean, W.rec);
  if ((e = hipGetLastError()) != hipSuccess || n <= kVmChunk) return e;
  const size_t most_bigs = n / kVmChunk;
  hipLaunchKernelGGL(k_vm_top<DIM>, dim3((unsigned)(most_bigs < kVmTopBlocks ? most_bigs : kVmTopBlocks)), dim3(kVmThreads),
                     0, s, (const uint32_t *)W.start, (const uint32_t *)W.ctr, (const uint4 *)W.bigs,
                     (const double *)W.rec, d_mean);
  return hipGetLastError();
}

template <int DIM>
hipError_t launch_centroid_chain(VoxelWs &W, const double *d_pts, size_t n, double *d_mean, uint32_t *d_count, hipStream_t s) {
  hipError_t e = launch_vm_starts(W, n, s);
  if (e != hipSuccess) return e;
  const unsigned fold_blocks = (unsigned)((n + kVmWaves * 64 - 1) / (kVmWaves * 64));
  hipLaunchKernelGGL(k_vm_fold<DIM>, dim3(fold_blocks), dim3(kVmThreads), 0, s, d_pts, (const uint32_t *)W.perm,
                     (const uint32_t *)W.start, W.ctr, d_mean, d_count, W.items, W.bigs);
  if ((e = hipGetLastError()) != hipSuccess || !d_mean) return e;
  return launch_large_means<DIM>(W, d_pts, n, d_mean, s);
}

}  // namespace

hipError_t launch_vm_starts(VoxelWs &W, size_t n, hipStream_t s) {
  const unsigned blocks = (unsigned)((n + kVoxelThreads - 1) / kVoxelThreads);
  hipLaunchKernelGGL(k_vm_starts, dim3(blocks), dim3(kVoxelThreads), 0, s, (const uint32_t *)W.key,
                     (const uint32_t *)W.perm, n, W.start, W.ctr);
  return hipGetLastError();
}

hipError_t launch_vm_large_means(VoxelWs &W, int dim, const double *d_pts, size_t n, double *d_mean, hipStream_t s) {
  return dim == 3 ? launch_large_means<3>(W, d_pts, n, d_mean, s) : launch_large_means<2>(W, d_pts, n, d_mean, s);
}

// the call on device buffers (voxel_mutex() held, the device current): everything on `s`, which is waited for once.
// d_cov (nullable; d_mean is required with it): the second moments beside the means, by voxel_cov.hip's launches
int voxel_centroids_on(VoxelWs &W, int dim, const double *d_pts, size_t n, double v, double *d_mean, uint32_t *d_count,
                       uint32_t *d_first_index, uint32_t *d_voxel_of, size_t *voxels, hipStream_t s, double *d_cov,
                       int ddof) {
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  const bool members = d_mean || d_count || d_voxel_of;  // (first_index and the number of voxels need no sort)
  if (members) {
    HIP_TRY(reserve(W.key, W.cap_key, n));  // (the sort's keys; voxel_of alone needs the launch that writes them)
    if (d_mean || d_count) {
      HIP_TRY(reserve(W.perm, W.cap_perm, n));
      HIP_TRY(reserve(W.start, W.cap_start, n + 1));
      HIP_TRY(reserve(W.ctr, W.cap_ctr, (size_t)kVmCtrWords));
      // an item per voxel above 256 members and per further kVmChunk of one; a record per item of a voxel with several
      HIP_TRY(reserve(W.items, W.cap_items, n / (kFoldGroup + 1) + n / kVmChunk + 2));
      HIP_TRY(reserve(W.bigs, W.cap_bigs, n / kVmChunk + 1));
      HIP_TRY(reserve(W.rec, W.cap_rec, (2 * (n / kVmChunk) + 2) * (d_cov ? 6 : 3)));  // (a record: the sums of an item)
    }
  }
  size_t mask = 0;
  uint32_t *sums = nullptr;
  HIP_TRY(launch_voxel_front(W, dim, d_pts, n, v, s, &mask, &sums));
  if (members || d_first_index) {
    hipLaunchKernelGGL(k_vm_place, dim3(tiles), dim3(kCompactThreads), 0, s, n, W.w, (const uint32_t *)W.cnt,
                       (const uint32_t *)sums, d_first_index);
    HIP_TRY(hipGetLastError());
  }
  if (members) {
    const unsigned blocks = (unsigned)((n + kVoxelThreads - 1) / kVoxelThreads);
    if (dim == 3)
      hipLaunchKernelGGL(k_vm_key<3>, dim3(blocks), dim3(kVoxelThreads), 0, s, d_pts, n, v, (const uint32_t *)W.tab, mask,
                         (const uint32_t *)W.w, W.key, d_voxel_of);
    else
      hipLaunchKernelGGL(k_vm_key<2>, dim3(blocks), dim3(kVoxelThreads), 0, s, d_pts, n, v, (const uint32_t *)W.tab, mask,
                         (const uint32_t *)W.w, W.key, d_voxel_of);
    HIP_TRY(hipGetLastError());
  }
  if (d_mean || d_count) {
    HIP_TRY(hipMemsetAsync(W.ctr, 0, kVmCtrWords * sizeof(uint32_t), s));
    HIP_TRY(stable_sort_cells(W.key, W.perm, (unsigned)n, bit_width(n), W.sort_tmp, W.cap_sort, s));  // (keys 0 .. n)
    if (d_cov) HIP_TRY(launch_covariance_chain(W, dim, d_pts, n, ddof, d_cov, d_mean, d_count, s));
    else if (dim == 3) HIP_TRY(launch_centroid_chain<3>(W, d_pts, n, d_mean, d_count, s));
    else HIP_TRY(launch_centroid_chain<2>(W, d_pts, n, d_mean, d_count, s));
  }
  HIP_TRY(compact_total(sums, chunks, s, voxels));
  return ICP_OK;
}

}  // namespace icp

extern "C" int icp_voxel_centroids_device(int dim, const double *d_pts, size_t n, double voxel, double *d_mean,
                                          uint32_t *d_count, uint32_t *d_first_index, uint32_t *d_voxel_of, size_t *voxels,
                                          int device, void *hip_stream) {
  if (!centroid_args_ok(dim, d_pts, n, voxel, d_mean, d_count, voxels, device)) return ICP_BAD_ARGUMENT;
  *voxels = 0;
  ICP_TRY_RC(voxel_device(&device));
  if (n == 0) return ICP_OK;
  std::lock_guard<std::mutex> lk(voxel_mutex());
  return voxel_centroids_on(voxel_ws(device), dim, d_pts, n, voxel, d_mean, d_count, d_first_index, d_voxel_of, voxels,
                            (hipStream_t)hip_stream, nullptr, 0);
}

extern "C" int icp_voxel_centroids(int dim, const double *pts, size_t n, double voxel, double *mean, uint32_t *count,
                                   uint32_t *first_index, uint32_t *voxel_of, size_t *voxels, int device) {
  if (!centroid_args_ok(dim, pts, n, voxel, mean, count, voxels, device)) return ICP_BAD_ARGUMENT;
  *voxels = 0;
  ICP_TRY_RC(voxel_device(&device));
  if (n == 0) return ICP_OK;
  std::lock_guard<std::mutex> lk(voxel_mutex());
  VoxelWs &W = voxel_ws(device);
  if (!W.stream) HIP_TRY(hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking));
  HIP_TRY(reserve(W.in, W.cap_in, n * dim));
  if (mean) HIP_TRY(reserve(W.out, W.cap_out, n * dim));
  if (count) HIP_TRY(reserve(W.count, W.cap_count, n));
  if (first_index) HIP_TRY(reserve(W.idx, W.cap_idx, n));
  if (voxel_of) HIP_TRY(reserve(W.of, W.cap_of, n));
  HIP_TRY(hipMemcpyAsync(W.in, pts, n * dim * sizeof(double), hipMemcpyHostToDevice, W.stream));
  ICP_TRY_RC(voxel_centroids_on(W, dim, W.in, n, voxel, mean ? W.out : nullptr, count ? W.count : nullptr,
                                first_index ? W.idx : nullptr, voxel_of ? W.of : nullptr, voxels, W.stream, nullptr, 0));
  const size_t k = *voxels;
  if (mean && k) HIP_TRY(hipMemcpyAsync(mean, W.out, k * dim * sizeof(double), hipMemcpyDeviceToHost, W.stream));
  if (count && k) HIP_TRY(hipMemcpyAsync(count, W.count, k * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  if (first_index && k) HIP_TRY(hipMemcpyAsync(first_index, W.idx, k * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  if (voxel_of) HIP_TRY(hipMemcpyAsync(voxel_of, W.of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  HIP_TRY(hipStreamSynchronize(W.stream));
  return ICP_OK;
}
