// What voxel centroids (voxel_mean.hip, include/icp_mi355x.h section 25) and voxel covariances (voxel_cov.hip, section 26)
// share on the device: the fold tree over a voxel's members in sorted order -- in a group of lanes, in a wave, in a
// workgroup -- and the bodies of the three folding kernels.  One copy of the tree: a body takes the number of second
// moments NS as a template parameter, 0 for the centroids (the kernels of voxel_mean.hip: what they compiled to before
// the parameter existed), dim (dim + 1) / 2 for the covariances (the kernels of voxel_cov.hip).
// Why a narrow group gives the tree's bits: with the c <= 2^k values of a voxel in lanes [0, 2^k) of a group of 256, the
// steps s >= 2^k only add +0.0 to each of them, and x + 0.0 + 0.0 = x + 0.0: one addition of +0.0 (it turns a -0.0 into
// +0.0, as the rule says), then the steps s < 2^k.  That holds per sum, for a product sum as for a coordinate sum.
#pragma once
#include <hip/hip_runtime.h>

#include "api_internal.hpp"
#include "fold_device.hpp"

namespace icp {

constexpr unsigned kVmChunk = kFoldGroup * kFoldGroup;  // members of a work item: 256 groups of the tree
constexpr unsigned kVmThreads = 256, kVmWaves = kVmThreads / 64;
constexpr unsigned kVmItemBlocks = 2048, kVmTopBlocks = 256;
// ctr: [0] voxels, [1] items, [2] voxels above kVmChunk members, [3] their records
enum { kVmVoxels = 0, kVmItems = 1, kVmBigs = 2, kVmRecs = 3, kVmCtrWords = 4 };

// the second moments of dim axes, packed: the pairs (a, b), a <= b, in the order xx, xy, yy / xx, xy, xz, yy, yz, zz
constexpr int vm_pairs(int dim) { return dim * (dim + 1) / 2; }

// o[ab] = d[a] d[b]: one multiplication each (the build has -ffp-contract=off: never fused with an addition behind it)
template <int DIM>
__device__ __forceinline__ void vm_products(const double (&d)[DIM], double (&o)[vm_pairs(DIM)]) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
#pragma unroll
    for (int b = a; b < DIM; ++b) o[k++] = d[a] * d[b];
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

// the voxels of this wave (lane l: count c, first sorted position s0) with W / 2 < c <= W (W = 8: 2 <= c), 64 / W at a
// time.  NS > 0: the members stay in the lanes; the mean comes back from the group's lane 0, and the products of the
// deviations go through the same tree (a lane past the voxel's members holds +0.0, not a deviation).
template <int DIM, int W, int NS>
__device__ __forceinline__ void vm_fold_narrow(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                               unsigned lane, uint32_t r0, uint32_t c, uint32_t s0,
                                               double *__restrict__ mean, double *__restrict__ cov, uint32_t ddof) {
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
    if constexpr (NS == 0) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) x[a] = x[a] + 0.0;  // the steps s >= W of the group of 256
      vm_lanes_tree<DIM, W>(x);
      if (on && j == 0) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) mean[(size_t)(r0 + vl) * DIM + a] = x[a] / (double)cv;
      }
    } else {
      double d[DIM], q[NS];
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        d[a] = x[a];
        x[a] = x[a] + 0.0;  // the steps s >= W of the group of 256
      }
      vm_lanes_tree<DIM, W>(x);
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        const double m = __shfl(x[a] / (double)cv, 0, W);  // (the group's lane 0 has the sum)
        d[a] = d[a] - m;
        if (on && j == 0) mean[(size_t)(r0 + vl) * DIM + a] = m;
      }
      vm_products<DIM>(d, q);
#pragma unroll
      for (int k = 0; k < NS; ++k) q[k] = (on && j < cv ? q[k] : 0.0) + 0.0;
      vm_lanes_tree<NS, W>(q);
      if (on && j == 0) {  // (cv >= 2 > ddof)
#pragma unroll
        for (int k = 0; k < NS; ++k) cov[(size_t)(r0 + vl) * NS + k] = q[k] / (double)(cv - ddof);
      }
    }
  }
}

// The body of k_vm_fold<DIM> (NS == 0) and k_vc_fold<DIM> (NS == vm_pairs(DIM)): mean and count (each nullable) of the
// voxels up to 256 members, and the work lists of the others.  NS > 0: cov of the same voxels as well (a voxel of one
// member: +0.0, the fold of the one product (x - x)^2, or the rule's +0.0 for c <= ddof); mean is required then.
template <int DIM, int NS>
__device__ __forceinline__ void vm_fold_body(const double *__restrict__ pts, const uint32_t *__restrict__ perm,
                                             const uint32_t *__restrict__ start, uint32_t *__restrict__ ctr,
                                             double *__restrict__ mean, uint32_t *__restrict__ count,
                                             uint4 *__restrict__ items, uint4 *__restrict__ bigs,
                                             double *__restrict__ cov, uint32_t ddof) {
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
    if constexpr (NS > 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) cov[(size_t)r * NS + k] = 0.0;
    }
  }
  vm_fold_narrow<DIM, 8, NS>(pts, perm, lane, r0, c, s0, mean, cov, ddof);
  vm_fold_narrow<DIM, 16, NS>(pts, perm, lane, r0, c, s0, mean, cov, ddof);
  vm_fold_narrow<DIM, 32, NS>(pts, perm, lane, r0, c, s0, mean, cov, ddof);
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
    if constexpr (NS == 0) {
      if (lane == 0) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) mean[(size_t)(r0 + vl) * DIM + a] = x[a] / (double)cv;
      }
    } else {  // the members again (from the cache this time), less the mean of lane 0
      double m[DIM], q[NS];
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        m[a] = __shfl(x[a] / (double)cv, 0, 64);
        if (lane == 0) mean[(size_t)(r0 + vl) * DIM + a] = m[a];
      }
      vm_wave_group<NS>(lane, cv, [&](unsigned i, double(&o)[NS]) {
        const size_t p = perm[(size_t)sv + i];
        double d[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) d[a] = pts[p * DIM + a] - m[a];
        vm_products<DIM>(d, o);
      }, q);
      if (lane == 0) {  // (cv > 32 > ddof)
#pragma unroll
        for (int k = 0; k < NS; ++k) cov[(size_t)(r0 + vl) * NS + k] = q[k] / (double)(cv - ddof);
      }
    }
  }
  if (c > kFoldGroup) {  // an item per kVmChunk members: {voxel, item of the voxel, where its record goes, items of the voxel}
    const uint32_t parts = (uint32_t)(((unsigned long long)c + kVmChunk - 1) / kVmChunk);
    const uint32_t at = atomicAdd(&ctr[kVmItems], parts);
    uint32_t rec = api::kCropGone;
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

// The body of k_vm_items<DIM> (NS == 0) and k_vc_items<DIM>: an item is members [kVmChunk j, kVmChunk (j + 1)) of its
// voxel -> the voxel's result (one item) or the item's record.  NS == 0: the sums of the coordinates, out = mean, K =
// DIM.  NS > 0: the sums of the products of the deviations from mean_of[voxel] (finished by an earlier launch), out =
// cov, K = NS, the divisor c - ddof (c > 256 > ddof).  part: K rows of LDS.
template <int DIM, int NS>
__device__ __forceinline__ void vm_items_body(double (*part)[kFoldGroup], const double *__restrict__ pts,
                                              const uint32_t *__restrict__ perm, const uint32_t *__restrict__ start,
                                              const uint32_t *__restrict__ ctr, const uint4 *__restrict__ items,
                                              const double *__restrict__ mean_of, double *__restrict__ out,
                                              double *__restrict__ rec, uint32_t ddof) {
  constexpr int K = NS > 0 ? NS : DIM;
  const uint32_t n_items = ctr[kVmItems];
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    const uint4 item = items[it];
    const uint32_t s0 = start[item.x], c = start[item.x + 1] - s0;
    const size_t first = (size_t)s0 + (size_t)item.y * kVmChunk;
    const unsigned long long left = (unsigned long long)c - (unsigned long long)item.y * kVmChunk;
    const unsigned k = left < kVmChunk ? (unsigned)left : kVmChunk;
    double x[K];
    if constexpr (NS == 0) {
      vm_block_levels<K>(part, k, true, [&](unsigned i, double(&o)[K]) {
        const size_t p = perm[first + i];
#pragma unroll
        for (int a = 0; a < DIM; ++a) o[a] = pts[p * DIM + a];
      }, x);
    } else {
      double m[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) m[a] = mean_of[(size_t)item.x * DIM + a];
      vm_block_levels<K>(part, k, true, [&](unsigned i, double(&o)[K]) {
        const size_t p = perm[first + i];
        double d[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) d[a] = pts[p * DIM + a] - m[a];
        vm_products<DIM>(d, o);
      }, x);
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int a = 0; a < K; ++a) {
        if (item.w == 1u) out[(size_t)item.x * K + a] = x[a] / (double)(c - ddof);
        else rec[((size_t)item.z + item.y) * K + a] = x[a];
      }
    }
  }
}

// The body of k_vm_top<DIM> and k_vc_top<DIM>: a voxel above kVmChunk members, the tree's third and fourth level over
// its at most 65 536 records of K sums; out[voxel] = the root / (c - ddof)
template <int K>
__device__ __forceinline__ void vm_top_body(double (*part)[kFoldGroup], const uint32_t *__restrict__ start,
                                            const uint32_t *__restrict__ ctr, const uint4 *__restrict__ bigs,
                                            const double *__restrict__ rec, double *__restrict__ out, uint32_t ddof) {
  const uint32_t n_bigs = ctr[kVmBigs];
  for (uint32_t b = blockIdx.x; b < n_bigs; b += gridDim.x) {
    const uint4 big = bigs[b];
    const uint32_t c = start[big.x + 1] - start[big.x];
    double x[K];
    vm_block_levels<K>(part, big.z, false, [&](unsigned i, double(&o)[K]) {
#pragma unroll
      for (int a = 0; a < K; ++a) o[a] = rec[((size_t)big.y + i) * K + a];
    }, x);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int a = 0; a < K; ++a) out[(size_t)big.x * K + a] = x[a] / (double)(c - ddof);
    }
  }
}

}  // namespace icp
