// What voxel thinning (voxel.hip, include/icp_mi355x.h section 22), voxel centroids (voxel_mean.hip, section 25) and
// voxel covariances (voxel_cov.hip, section 26) share: the cell of a point, the equality of cells, the hash that starts a walk, the read-only walk of the table to a
// voxel's lowest index, and -- host side -- the per-device workspace with the launches that fill the table and the
// marks.  One copy of the rule: both features decide membership with exactly these functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <mutex>

namespace icp {

constexpr uint32_t kVoxelEmpty = 0xffffffffu;
constexpr unsigned kVoxelThreads = 256;

// the cell of point i (2-D: the third coordinate is +0.0); false: a coordinate is NaN or infinite
template <int DIM>
__device__ __forceinline__ bool voxel_cell(const double *__restrict__ pts, size_t i, double v, double (&c)[3]) {
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (a < DIM) {
      const double p = pts[i * DIM + a];
      finite = finite && fabs(p) <= DBL_MAX;  // (false for a NaN)
      c[a] = floor(p / v) + 0.0;
    } else {
      c[a] = 0.0;
    }
  }
  return finite;
}

__device__ __forceinline__ bool voxel_same(const double (&a)[3], const double (&b)[3]) {
  return a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
}

// where the walk of a cell starts: a 64-bit mix of the three bit patterns (canonical: no -0.0, no NaN)
__device__ __forceinline__ unsigned long long voxel_hash(const double (&c)[3]) {
  unsigned long long h = (unsigned long long)__double_as_longlong(c[0]) * 0x9e3779b97f4a7c15ull;
  h ^= h >> 32;
  h = (h ^ (unsigned long long)__double_as_longlong(c[1])) * 0xc2b2ae3d27d4eb4full;
  h ^= h >> 29;
  h = (h ^ (unsigned long long)__double_as_longlong(c[2])) * 0x165667b19e3779f9ull;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;
}

// The walk of the finished table, read-only: the word of the slot that the voxel of point i (finite, cell c) owns, which
// is the voxel's lowest index.  kVoxelEmpty: the walk met an empty slot (cannot be for an inserted point).
template <int DIM>
__device__ __forceinline__ uint32_t voxel_leader(const double *__restrict__ pts, size_t n, double v,
                                                 const uint32_t *__restrict__ tab, size_t mask, size_t i,
                                                 const double (&c)[3]) {
  double o[3];
  size_t s = (size_t)voxel_hash(c) & mask;
  for (size_t probe = 0; probe <= mask; ++probe) {
    const uint32_t cur = tab[s];
    if (cur == (uint32_t)i) return cur;
    if (cur >= n) return kVoxelEmpty;
    (void)voxel_cell<DIM>(pts, cur, v, o);
    if (voxel_same(c, o)) return cur;  // its voxel's slot, and a lower index has it
    s = (s + 1) & mask;
  }
  return kVoxelEmpty;
}

// ---- host side (voxel.hip defines them) ----
// What the calls keep between them, per device: the table, the marks, the tile counts and chunk sums, the host entries'
// staging buffers, and what the centroids add (sort keys and order, segment starts, work lists, the sort's temporary).
// One call at a time (voxel_mutex() is held for the length of a call).
struct VoxelWs {
  uint32_t *tab = nullptr, *w = nullptr, *cnt = nullptr, *idx = nullptr;
  double *in = nullptr, *out = nullptr, *cov = nullptr;  // (cov: voxel_cov.hip's host entry)
  size_t cap_tab = 0, cap_w = 0, cap_cnt = 0, cap_idx = 0, cap_in = 0, cap_out = 0, cap_cov = 0;
  // voxel_mean.hip
  uint32_t *key = nullptr, *perm = nullptr, *start = nullptr, *ctr = nullptr, *count = nullptr, *of = nullptr;
  uint4 *items = nullptr, *bigs = nullptr;
  double *rec = nullptr;
  void *sort_tmp = nullptr;
  size_t cap_key = 0, cap_perm = 0, cap_start = 0, cap_ctr = 0, cap_count = 0, cap_of = 0, cap_items = 0, cap_bigs = 0,
         cap_rec = 0, cap_sort = 0;
  hipStream_t stream = nullptr;  // the host entries'
};
std::mutex &voxel_mutex();
VoxelWs &voxel_ws(int device);  // (voxel_mutex() held)
bool voxel_size_ok(double v);
// the arguments every stand-alone entry checks before the device is touched
bool voxel_args_ok(int dim, const void *pts, size_t n, double v, const size_t *out_count);
// ICP_NO_DEVICE without one; -1 -> the current device; makes *device current
int voxel_device(int *device);
// the table for n points, preset on `s` (a table grows to the next power of two: geometric by construction)
hipError_t voxel_table(VoxelWs &W, size_t n, hipStream_t s, size_t *mask);
// the insert and the mark launch on `s`: w[i] (0 = its voxel's lowest index, kCropGone otherwise) and cnt[tile] for the
// n > 0 points of d_pts
hipError_t launch_voxel_marks(int dim, const double *d_pts, size_t n, double v, uint32_t *tab, size_t mask, uint32_t *w,
                              uint32_t *cnt, hipStream_t s);
// the front half of a stand-alone call: voxel_table, W.w and W.cnt reserved for the n > 0 points of d_pts, then
// launch_voxel_marks and the chunk sums on `s`; *sums = the chunk sums (behind the tile counts in W.cnt)
hipError_t launch_voxel_front(VoxelWs &W, int dim, const double *d_pts, size_t n, double v, hipStream_t s, size_t *mask,
                              uint32_t **sums);

// ---- the members of a voxel (voxel_mean.hip defines them; voxel_cov.hip runs the same chain) ----
constexpr size_t kVmMaxPoints = (size_t)1 << 27;  // what the sort of the members takes
// The call on device buffers (voxel_mutex() held, the device current): everything on `s`, which is waited for once.
// Every output is nullable.  d_cov == nullptr: the centroids.  Otherwise (d_mean required, ddof 0 or 1) the sorted members
// are folded by launch_covariance_chain, the second moments beside the means.
int voxel_centroids_on(VoxelWs &W, int dim, const double *d_pts, size_t n, double v, double *d_mean, uint32_t *d_count,
                       uint32_t *d_first_index, uint32_t *d_voxel_of, size_t *voxels, hipStream_t s, double *d_cov,
                       int ddof);
// start[] and the number of voxels from the sorted keys
hipError_t launch_vm_starts(VoxelWs &W, size_t n, hipStream_t s);
// the means of the voxels above 256 members, from the work lists a folding launch left in W
hipError_t launch_vm_large_means(VoxelWs &W, int dim, const double *d_pts, size_t n, double *d_mean, hipStream_t s);
// voxel_cov.hip: behind the sort, on `s` -- start[], the means and second moments of the voxels up to 256 members, the
// means of the larger ones, then their second moments over the same work lists
hipError_t launch_covariance_chain(VoxelWs &W, int dim, const double *d_pts, size_t n, int ddof, double *d_cov,
                                   double *d_mean, uint32_t *d_count, hipStream_t s);

}  // namespace icp
