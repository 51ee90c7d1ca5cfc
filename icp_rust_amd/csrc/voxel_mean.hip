// EXTENSION beyond the reference (include/icp_mi355x.h section 25): voxel centroids -- per occupied voxel the mean of its
// points, their number, the lowest index, and per point the rank of its voxel.  Membership and order are voxel
// thinning's (section 22, voxel_device.hpp); a sum's bits are the fold tree of section 9 over the members in ascending
// index, so a result is a pure function of the input.
//   the chain  k_voxel_insert, k_voxel_mark, k_compact_chunks       as the thinning runs them: w[i] = 0 for a voxel's lowest
//                                                                   index, cnt[tile]
//              k_vm_place       leader i of rank r: first_index[r] = i, w[i] = r (the marks become the leaders' ranks)
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
// Why a narrow group gives the tree's bits: with the c <= 2^k values of a voxel in lanes [0, 2^k) of a group of 256, the
// steps s >= 2^k only add +0.0 to each of them, and x + 0.0 + 0.0 = x + 0.0: one addition of +0.0 (it turns a -0.0 into
// +0.0, as the rule says), then the steps s < 2^k.  No float atomics.
#include <vector>

#include "api_internal.hpp"
#include "compact_device.hpp"
#include "fold_device.hpp"
#include "voxel_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

constexpr unsigned kVmChunk = kFoldGroup * kFoldGroup;  // members of a work item: 256 groups of the tree
constexpr unsigned kVmThreads = 256, kVmWaves = kVmThreads / 64;
constexpr unsigned kVmItemBlocks = 2048, kVmTopBlocks = 256;
// ctr: [0] voxels, [1] items, [2] voxels above kVmChunk members, [3] their records
enum { kVmVoxels = 0, kVmItems = 1, kVmBigs = 2, kVmRecs = 3, kVmCtrWords = 4 };

// leader i of rank r: first_index[r] = i (nullable), w[i] = r
__global__ __launch_bounds__(kCompactThreads) void k_vm_place(size_t n, uint32_t *__restrict__ w,
                                                              const uint32_t *__restrict__ cnt,
                                                              const uint32_t *__restrict__ sums,
                                                              uint32_t *__restrict__ first_index) {
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  __shared__ unsigned lds[kCompactWaves];
  const unsigned base = compact_tile_base(cnt, sums, blockIdx.x, lds);
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  bool in[kCompactRounds];
  unsigned rank[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + threadIdx.x;
    in[k] = i < n && w[i] != kCropGone;
  }
  (void)compact_tile_ranks(in, rank, wcnt);
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + threadIdx.x;
    if (!in[k]) continue;
    const uint32_t at = base + rank[k];  // (< the voxels in all, which are <= n)
    if (first_index) first_index[at] = (uint32_t)i;
    w[i] = at;
  }
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

// ---- the tree ----
// g[i] += g[i + s] for s = W / 2 ... 1 over the W lanes of a group (W <= 64 consecutive lanes): the group's lane 0 ends with the fold
template <int DIM, int W>
__device__ __forceinline__ void vm_lanes_tree(double (&x)[DIM]) {
#pragma unroll
  for (int s = W / 2; s > 0; s >>= 1) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) x[a] = x[a] + __shfl_down(x[a], s, W);
  }
}

// One group of the tree, by a wave: value i < k (k <= 256) is load(i), +0.0 beyond; lane l holds values l, l + 64,
// l + 128, l + 192, so the steps 128 and 64 are additions inside the lane.  Lane 0 returns the group's fold.
template <int DIM, typename Load>
__device__ __forceinline__ void vm_wave_group(unsigned lane, unsigned k, Load load, double (&x)[DIM]) {
  double q[4][DIM];
#pragma unroll
  for (unsigned u = 0; u < 4; ++u) {
    const unsigned i = lane + 64u * u;
#pragma unroll
    for (int a = 0; a < DIM; ++a) q[u][a] = 0.0;
    if (i < k) load(i, q[u]);
  }
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double lo = q[0][a] + q[2][a], hi = q[1][a] + q[3][a];  // s = 128
    x[a] = lo + hi;                                               // s = 64
  }
  vm_lanes_tree<DIM, 64>(x);
}

// the voxels of this wave (lane l: count c, first sorted position s0) with W / 2 < c <= W (W = 8: 2 <= c), 64 / W at a time
template <int DIM, int W>
__device__ __forceinline__ void vm_fold_narrow(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                               unsigned lane, uint32_t r0, uint32_t c, uint32_t s0,
                                               double *__restrict__ mean) {
  constexpr unsigned kPer = 64 / W;
  const bool mine = c <= (uint32_t)W && c > (W == 8 ? 1u : (uint32_t)W / 2);
  const unsigned long long todo = __ballot(mine);
  if (todo == 0ull) return;
  const unsigned g = lane / W, j = lane % W;
  for (unsigned t = 0; t < (unsigned)W; ++t) {
    if (((todo >> (t * kPer)) & ((1ull << kPer) - 1ull)) == 0ull) continue;  // (uniform across the wave)
    const unsigned vl = t * kPer + g;
    const uint32_t cv = __shfl(c, vl, 64), sv = __shfl(s0, vl, 64);
    const bool on = (todo >> vl) & 1ull;
    double x[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) x[a] = 0.0;
    if (on && j < cv) {
      const size_t i = perm[(size_t)sv + j];
#pragma unroll
      for (int a = 0; a < DIM; ++a) x[a] = pts[i * DIM + a];
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) x[a] = x[a] + 0.0;  // the steps s >= W of the group of 256
    vm_lanes_tree<DIM, W>(x);
    if (on && j == 0) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) mean[(size_t)(r0 + vl) * DIM + a] = x[a] / (double)cv;
    }
  }
}

// mean and count (each nullable) of the voxels up to 256 members; the work lists of the others
template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vm_fold(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                                        const uint32_t *__restrict__ start, uint32_t *__restrict__ ctr,
                                                        double *__restrict__ mean, uint32_t *__restrict__ count,
                                                        uint4 *__restrict__ items, uint4 *__restrict__ bigs) {
  const uint32_t voxels = ctr[kVmVoxels];
  const unsigned lane = threadIdx.x & 63u;
  const size_t wave0 = ((size_t)blockIdx.x * kVmWaves + (threadIdx.x >> 6)) * 64u;
  if (wave0 >= voxels) return;  // (uniform across the wave)
  const uint32_t r0 = (uint32_t)wave0, r = r0 + lane;
  uint32_t s0 = 0, c = 0;
  if (r < voxels) {
    s0 = start[r];
    c = start[r + 1] - s0;
    if (count) count[r] = c;
  }
  if (!mean) return;
  if (c == 1) {  // the fold of one value is the value
    const size_t i = perm[s0];
#pragma unroll
    for (int a = 0; a < DIM; ++a) mean[(size_t)r * DIM + a] = pts[i * DIM + a];
  }
  vm_fold_narrow<DIM, 8>(pts, perm, lane, r0, c, s0, mean);
  vm_fold_narrow<DIM, 16>(pts, perm, lane, r0, c, s0, mean);
  vm_fold_narrow<DIM, 32>(pts, perm, lane, r0, c, s0, mean);
  unsigned long long todo = __ballot(c > 32u && c <= kFoldGroup);
  while (todo) {  // the wave per voxel
    const unsigned vl = (unsigned)__ffsll((long long)todo) - 1u;
    todo &= todo - 1ull;
    const uint32_t cv = __shfl(c, vl, 64), sv = __shfl(s0, vl, 64);
    double x[DIM];
    vm_wave_group<DIM>(lane, cv, [&](unsigned i, double(&o)[DIM]) {
      const size_t p = perm[(size_t)sv + i];
#pragma unroll
      for (int a = 0; a < DIM; ++a) o[a] = pts[p * DIM + a];
    }, x);
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) mean[(size_t)(r0 + vl) * DIM + a] = x[a] / (double)cv;
    }
  }
  if (c > kFoldGroup) {  // an item per kVmChunk members: {voxel, item of the voxel, where its record goes, items of the voxel}
    const uint32_t parts = (uint32_t)(((unsigned long long)c + kVmChunk - 1) / kVmChunk);
    const uint32_t at = atomicAdd(&ctr[kVmItems], parts);
    uint32_t rec = kCropGone;
    if (parts > 1) {
      rec = atomicAdd(&ctr[kVmRecs], parts);
      bigs[atomicAdd(&ctr[kVmBigs], 1u)] = make_uint4(r, rec, parts, 0u);
    }
    for (uint32_t j = 0; j < parts; ++j) items[(size_t)at + j] = make_uint4(r, j, rec, parts);
  }
}

// Two levels of the tree by a workgroup: the k <= kVmChunk values load(0 .. k - 1) in groups of 256, a wave per group,
// then the group results (+0.0 up to 256) by wave 0.  One group: with `more` (the values are a part of a larger level,
// so the group's result meets the padding of the next level's group: + 0.0) or without (it is the tree's root).
// Thread 0 returns the fold.  Every thread calls it (barriers; k is uniform).
template <int DIM, typename Load>
__device__ __forceinline__ void vm_block_levels(double (*part)[kFoldGroup], unsigned k, bool more, Load load,
                                                double (&x)[DIM]) {
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned groups = (k + kFoldGroup - 1) / kFoldGroup;
  __syncthreads();  // (part may still be read from an earlier call)
  if (threadIdx.x >= groups && threadIdx.x < kFoldGroup) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) part[a][threadIdx.x] = 0.0;
  }
  for (unsigned g = wave; g < groups; g += kVmWaves) {
    const unsigned first = g * kFoldGroup, len = k - first < kFoldGroup ? k - first : kFoldGroup;
    vm_wave_group<DIM>(lane, len, [&](unsigned i, double(&o)[DIM]) { load(first + i, o); }, x);
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) part[a][g] = x[a];
    }
  }
  __syncthreads();
  if (wave == 0) {
    if (groups == 1) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) x[a] = more ? part[a][0] + 0.0 : part[a][0];
    } else {
      vm_wave_group<DIM>(lane, kFoldGroup, [&](unsigned i, double(&o)[DIM]) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) o[a] = part[a][i];
      }, x);
    }
  }
}

// an item: members [kVmChunk j, kVmChunk (j + 1)) of its voxel -> the voxel's mean (one item) or the item's record
template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vm_items(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ start, const uint32_t *__restrict__ ctr,
                                                         const uint4 *__restrict__ items, double *__restrict__ mean,
                                                         double *__restrict__ rec) {
  __shared__ double part[DIM][kFoldGroup];
  const uint32_t n_items = ctr[kVmItems];
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint4 item = items[it];
    const uint32_t s0 = start[item.x], c = start[item.x + 1] - s0;
    const size_t first = (size_t)s0 + (size_t)item.y * kVmChunk;
    const unsigned long long left = (unsigned long long)c - (unsigned long long)item.y * kVmChunk;
    const unsigned k = left < kVmChunk ? (unsigned)left : kVmChunk;
    double x[DIM];
    vm_block_levels<DIM>(part, k, true, [&](unsigned i, double(&o)[DIM]) {
      const size_t p = perm[first + i];
#pragma unroll
      for (int a = 0; a < DIM; ++a) o[a] = pts[p * DIM + a];
    }, x);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        if (item.w == 1u) mean[(size_t)item.x * DIM + a] = x[a] / (double)c;
        else rec[((size_t)item.z + item.y) * DIM + a] = x[a];
      }
    }
  }
}

// a voxel above kVmChunk members: the tree's third and fourth level over its at most 65 536 records
template <int DIM>
__global__ __launch_bounds__(kVmThreads) void k_vm_top(const uint32_t *__restrict__ start, const uint32_t *__restrict__ ctr,
                                                       const uint4 *__restrict__ bigs, const double *__restrict__ rec,
                                                       double *__restrict__ mean) {
  __shared__ double part[DIM][kFoldGroup];
  const uint32_t n_bigs = ctr[kVmBigs];
  for (uint32_t b = blockIdx.x; b < n_bigs; b += gridDim.x) {
    const uint4 big = bigs[b];
    const uint32_t c = start[big.x + 1] - start[big.x];
    double x[DIM];
    vm_block_levels<DIM>(part, big.z, false, [&](unsigned i, double(&o)[DIM]) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) o[a] = rec[((size_t)big.y + i) * DIM + a];
    }, x);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) mean[(size_t)big.x * DIM + a] = x[a] / (double)c;
    }
  }
}

namespace {

constexpr size_t kVmMaxPoints = (size_t)1 << 27;  // what stable_sort_cells takes

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

template <int DIM>
hipError_t launch_centroid_chain(VoxelWs &W, const double *d_pts, size_t n, double *d_mean, uint32_t *d_count, hipStream_t s) {
  const unsigned blocks = (unsigned)((n + kVoxelThreads - 1) / kVoxelThreads);
  hipLaunchKernelGGL(k_vm_starts, dim3(blocks), dim3(kVoxelThreads), 0, s, (const uint32_t *)W.key,
                     (const uint32_t *)W.perm, n, W.start, W.ctr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned fold_blocks = (unsigned)((n + kVmWaves * 64 - 1) / (kVmWaves * 64));
  hipLaunchKernelGGL(k_vm_fold<DIM>, dim3(fold_blocks), dim3(kVmThreads), 0, s, d_pts, (const uint32_t *)W.perm,
                     (const uint32_t *)W.start, W.ctr, d_mean, d_count, W.items, W.bigs);
  if ((e = hipGetLastError()) != hipSuccess || !d_mean || n <= kFoldGroup) return e;  // (no voxel above 256 members)
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

// the call on device buffers (voxel_mutex() held, the device current): everything on `s`, which is waited for once
int voxel_centroids_on(VoxelWs &W, int dim, const double *d_pts, size_t n, double v, double *d_mean, uint32_t *d_count,
                       uint32_t *d_first_index, uint32_t *d_voxel_of, size_t *voxels, hipStream_t s) {
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  const bool members = d_mean || d_count || d_voxel_of;  // (first_index and the number of voxels need no sort)
  size_t mask = 0;
  HIP_TRY(voxel_table(W, n, s, &mask));
  HIP_TRY(reserve(W.w, W.cap_w, n));
  HIP_TRY(reserve(W.cnt, W.cap_cnt, (size_t)tiles + chunks));
  if (members) {
    HIP_TRY(reserve(W.key, W.cap_key, n));  // (the sort's keys; voxel_of alone needs the launch that writes them)
    if (d_mean || d_count) {
      HIP_TRY(reserve(W.perm, W.cap_perm, n));
      HIP_TRY(reserve(W.start, W.cap_start, n + 1));
      HIP_TRY(reserve(W.ctr, W.cap_ctr, (size_t)kVmCtrWords));
      // an item per voxel above 256 members and per further kVmChunk of one; a record per item of a voxel with several
      HIP_TRY(reserve(W.items, W.cap_items, n / (kFoldGroup + 1) + n / kVmChunk + 2));
      HIP_TRY(reserve(W.bigs, W.cap_bigs, n / kVmChunk + 1));
      HIP_TRY(reserve(W.rec, W.cap_rec, (2 * (n / kVmChunk) + 2) * 3));
    }
  }
  uint32_t *sums = W.cnt + tiles;
  HIP_TRY(launch_voxel_marks(dim, d_pts, n, v, W.tab, mask, W.w, W.cnt, s));
  HIP_TRY(launch_compact_chunks(W.cnt, tiles, sums, s));
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
    if (dim == 3) HIP_TRY(launch_centroid_chain<3>(W, d_pts, n, d_mean, d_count, s));
    else HIP_TRY(launch_centroid_chain<2>(W, d_pts, n, d_mean, d_count, s));
  }
  std::vector<uint32_t> host(chunks);
  HIP_TRY(hipMemcpyAsync(host.data(), sums, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  size_t total = 0;
  for (unsigned c = 0; c < chunks; ++c) total += host[c];
  *voxels = total;
  return ICP_OK;
}

}  // namespace
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
                            (hipStream_t)hip_stream);
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
                                first_index ? W.idx : nullptr, voxel_of ? W.of : nullptr, voxels, W.stream));
  const size_t k = *voxels;
  if (mean && k) HIP_TRY(hipMemcpyAsync(mean, W.out, k * dim * sizeof(double), hipMemcpyDeviceToHost, W.stream));
  if (count && k) HIP_TRY(hipMemcpyAsync(count, W.count, k * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  if (first_index && k) HIP_TRY(hipMemcpyAsync(first_index, W.idx, k * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  if (voxel_of) HIP_TRY(hipMemcpyAsync(voxel_of, W.of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  HIP_TRY(hipStreamSynchronize(W.stream));
  return ICP_OK;
}
