// The fixed fold tree of include/icp_mi355x.h section 9, shared by the three pose qualities: point (quality.hip, six
// sums), point-to-plane (quality_plane.hip, ten) and point-to-line (quality_line.hip, ten), single calls and batches.
// Groups of kFoldGroup values, g[i] += g[i + s] for s = 128, 64, ..., 1 inside a group, the inlier counts added and the
// NaN flags or-ed beside the sums, one record (common.hpp: FoldPart) per group, level after level down to one.  This
// tree IS the definition of a result's bits: nothing crosses workgroups inside a launch and no sum uses atomics, so a
// result is a pure function of the inputs.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

#include "common.hpp"

namespace icp {

constexpr unsigned kFoldGroup = 256;  // values per group of the tree

// one group of the tree in LDS
template <int SUMS>
struct FoldLds {
  double v[SUMS][kFoldGroup];
  unsigned long long c[kFoldGroup];
  unsigned f[kFoldGroup];
};
// (below the 64 KB every kernel has without a grant, k_quality_batch's 48 KB of targets included)
static_assert(sizeof(FoldLds<6>) == 15360 && sizeof(FoldLds<10>) == 23552, "the LDS of a group");

template <int SUMS>
__device__ __forceinline__ void fold_put(FoldLds<SUMS> &L, unsigned lane, const double (&v)[SUMS], unsigned long long c,
                                         unsigned f) {
#pragma unroll
  for (int k = 0; k < SUMS; ++k) L.v[k][lane] = v[k];
  L.c[lane] = c;
  L.f[lane] = f;
}

template <int SUMS>
__device__ __forceinline__ void fold_put_zero(FoldLds<SUMS> &L, unsigned lane) {
#pragma unroll
  for (int k = 0; k < SUMS; ++k) L.v[k][lane] = 0.;
  L.c[lane] = 0;
  L.f[lane] = 0;
}

template <int SUMS>
__device__ __forceinline__ FoldPart<SUMS> fold_part(const double (&v)[SUMS], unsigned long long c, unsigned f) {
  FoldPart<SUMS> p;
#pragma unroll
  for (int k = 0; k < SUMS; ++k) p.v[k] = v[k];
  p.inliers = c;
  p.nan = f;
  p.pad = 0;
  return p;
}

// The tree over one group: lanes [0, 256) hold the values (+0.0 where the group has none).  Every thread of the
// workgroup calls it (barriers); afterwards lane 0 holds the group's fold.
template <int SUMS>
__device__ __forceinline__ void fold_group(FoldLds<SUMS> &L, unsigned tid) {
  for (unsigned s = kFoldGroup / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < SUMS; ++k) L.v[k][tid] = L.v[k][tid] + L.v[k][tid + s];
      L.c[tid] += L.c[tid + s];
      L.f[tid] |= L.f[tid + s];
    }
  }
  __syncthreads();
}

template <int SUMS>
__device__ __forceinline__ FoldPart<SUMS> fold_take(const FoldLds<SUMS> &L) {
  double v[SUMS];
#pragma unroll
  for (int k = 0; k < SUMS; ++k) v[k] = L.v[k][0];
  return fold_part(v, L.c[0], L.f[0]);
}

// The whole tree of one batch item inside its workgroup: thread tid < n holds a point's terms (the others +0.0), n <=
// the workgroup's size, and every thread calls it (barriers; n is uniform).  The tree over each group of 256 points, then
// over the group records (grp: room for one per group), as the levels of a single call fold them; thread 0 writes *out.
// n == 1: *out is the one point's terms (the fold of one value is the value: no +0.0 added, a -0.0 stays).
template <int SUMS>
__device__ __forceinline__ void fold_workgroup(FoldLds<SUMS> &L, FoldPart<SUMS> *grp, unsigned tid, unsigned n,
                                               const double (&v)[SUMS], unsigned in, unsigned nan, FoldPart<SUMS> *out) {
  if (n == 1) {
    if (tid == 0) *out = fold_part(v, in, nan);
    return;
  }
  const unsigned groups = (n + kFoldGroup - 1) / kFoldGroup;
  for (unsigned g = 0; g < groups; ++g) {
    const unsigned lane = tid - g * kFoldGroup;  // (wraps for the threads below the group: never < kFoldGroup then)
    if (lane < kFoldGroup) fold_put(L, lane, v, in, nan);
    fold_group(L, tid);
    if (tid == 0) grp[g] = fold_take(L);
    __syncthreads();
  }
  if (groups == 1) {
    if (tid == 0) *out = grp[0];
    return;
  }
  if (tid < kFoldGroup) {
    if (tid < groups) fold_put(L, tid, grp[tid].v, grp[tid].inliers, grp[tid].nan);
    else fold_put_zero(L, tid);
  }
  fold_group(L, tid);
  if (tid == 0) *out = fold_take(L);
}

// a level of the tree: records [256 g, 256 g + 256) of `in` (k of them), +0.0 beyond, folded -> out[g]
template <int SUMS>
__global__ __launch_bounds__(kFoldGroup) void k_fold_level(const FoldPart<SUMS> *__restrict__ in, unsigned k,
                                                           FoldPart<SUMS> *__restrict__ out) {
  __shared__ FoldLds<SUMS> L;
  const unsigned tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kFoldGroup + tid;
  if (i < k) fold_put(L, tid, in[i].v, in[i].inliers, in[i].nan);
  else fold_put_zero(L, tid);
  fold_group(L, tid);
  if (tid == 0) out[blockIdx.x] = fold_take(L);
}

// The levels above the first: from the k records in `cur` down to one, a launch per level, the two buffers in turns.
// *root: where the last level leaves its record (cur itself for k == 1).
template <int SUMS>
hipError_t fold_levels(FoldPart<SUMS> *cur, FoldPart<SUMS> *nxt, unsigned k, hipStream_t stream, FoldPart<SUMS> **root) {
  while (k > 1) {
    const unsigned k2 = (k + kFoldGroup - 1) / kFoldGroup;
    hipLaunchKernelGGL(k_fold_level<SUMS>, dim3(k2), dim3(kFoldGroup), 0, stream, (const FoldPart<SUMS> *)cur, k, nxt);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    std::swap(cur, nxt);
    k = k2;
  }
  *root = cur;
  return hipSuccess;
}

}  // namespace icp
