// The stable compaction, in one place.  A tile = kCompactTile consecutive elements = one workgroup of four waves, four
// rounds of 256 elements.  A first launch counts the survivors of every tile (a ballot per round and wave gives the
// wave's count and the lane's rank among its wave's survivors; the sixteen counts meet in LDS) into cnt[tile];
// k_compact_chunks adds the counts up in chunks of kCompactChunk tiles; in the last launch a workgroup per tile adds up
// the chunk sums and the counts in front of it and moves its survivors there.  Every term of a position counts survivors
// that come EARLIER in the input: the order is kept and a position is a pure function of the inputs.  No atomics, no
// workgroup waits for another.
//   the pieces  compact_wave_rank, compact_round_offset, compact_tile_ranks, compact_tile_base, k_compact_chunks: the
//               gates (gate.hip: k_gate_stage, k_gate_place; gate_plane.hip: k_plgate_stage, k_lngate_stage,
//               k_plgate_place) are built from these directly -- they compact into a tile's own staging segment and are
//               shaped around their registers
//   the bodies  compact_mark_tile and compact_place_tile: the whole of a mark and of a place kernel but its rule.  Every
//               other user is one call of a body with its rule as a lambda:
//                 marks   k_crop_mark<DIM>, k_crop_rec_mark (crop.hip), k_voxel_mark<DIM> (voxel.hip), k_mask_marks
//                         (query.hip), k_outlier_count (outlier.hip)
//                 places  k_crop_place<DIM> (crop.hip), k_voxel_place<DIM> (voxel.hip), k_vm_place (voxel_mean.hip;
//                         voxel_cov.hip runs the same chain)
//               The one exception is k_crop_rec_place (crop.hip), written out around the pieces: it was measurably
//               slower through the body (the reason stands at the kernel).
//   the host    compact_tiles, compact_chunks, launch_compact_chunks, and compact_total: the one read-back of the chunk
//               sums, which is how a caller learns the number of survivors
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace icp {

constexpr unsigned kCompactThreads = 256, kCompactWaves = kCompactThreads / 64;
constexpr unsigned kCompactRounds = 4;
constexpr unsigned kCompactTile = kCompactThreads * kCompactRounds;  // elements per workgroup
constexpr unsigned kCompactChunk = 8192;  // tiles whose counts one workgroup adds up itself (2^23 elements)

inline unsigned compact_tiles(size_t n) { return (unsigned)((n + kCompactTile - 1) / kCompactTile); }
inline unsigned compact_chunks(unsigned tiles) { return (tiles + kCompactChunk - 1) / kCompactChunk; }

// the sum of v over the workgroup (every thread calls it; every thread gets it)
__device__ __forceinline__ unsigned compact_block_sum(unsigned v, unsigned *lds) {
  const unsigned tid = threadIdx.x;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();  // (lds may still be read from an earlier call)
  if ((tid & 63u) == 0) lds[tid >> 6] = v;
  __syncthreads();
  unsigned t = 0;
#pragma unroll
  for (unsigned w = 0; w < kCompactWaves; ++w) t += lds[w];
  return t;
}

// One round of a tile (256 elements; mask: the ballot of the flag of the thread's): the survivors in front of the
// thread's element in its wave; the wave's count goes to wcnt[wave] (wcnt: the round's row of the tile's sixteen counts).
__device__ __forceinline__ unsigned compact_wave_rank(unsigned long long mask, unsigned *wcnt) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned rank = __popcll(mask & ((1ull << lane) - 1ull));
  if (lane == 0) wcnt[threadIdx.x >> 6] = __popcll(mask);
  return rank;
}

// ... and once every round has been through it and the workgroup has met (__syncthreads): adds to rank the survivors of
// the rounds and waves in front of the thread's wave in round k (rounds in order, waves in order inside one), so that
// it counts the tile's survivors in front of the thread's element.  wcnt: round k's row; total: the survivors of the
// rounds before on entry, of those and round k on return.
__device__ __forceinline__ void compact_round_offset(unsigned &rank, const unsigned *wcnt, unsigned &total) {
  const unsigned wave = threadIdx.x >> 6;
#pragma unroll
  for (unsigned w = 0; w < kCompactWaves; ++w) {
    if (w == wave) rank += total;
    total += wcnt[w];
  }
}

// both steps for flags that are all known: in[k] is the flag of the thread's element of round k (element
// k * kCompactThreads + tid of the tile).  rank[k] = the tile's survivors in front of that element (whether it survives
// or not); returns the tile's survivors.
__device__ __forceinline__ unsigned compact_tile_ranks(const bool (&in)[kCompactRounds], unsigned (&rank)[kCompactRounds],
                                                       unsigned (*wcnt)[kCompactWaves]) {
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) rank[k] = compact_wave_rank(__ballot(in[k]), wcnt[k]);
  __syncthreads();
  unsigned total = 0;
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) compact_round_offset(rank[k], wcnt[k], total);
  return total;
}

// the survivors of the tiles in front of `tile`: the chunk sums in front of its chunk + the counts in front of it there
// (no chunk in front below kCompactChunk tiles: sums unread)
__device__ __forceinline__ unsigned compact_tile_base(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ sums,
                                                      unsigned tile, unsigned *lds) {
  const unsigned tid = threadIdx.x, chunk = tile / kCompactChunk;
  unsigned s = 0;
  for (unsigned c = tid; c < chunk; c += kCompactThreads) s += sums[c];
  for (size_t t = (size_t)chunk * kCompactChunk + tid; t < tile; t += kCompactThreads) s += cnt[t];
  return compact_block_sum(s, lds);
}

// The body of a mark launch (one workgroup per tile, kCompactThreads threads): keep(i) is called once for every element
// i < n of the workgroup's tile, returns the element's flag and writes whatever mark words its caller keeps;
// cnt[tile] = the tile's survivors.
template <class Keep>
__device__ __forceinline__ void compact_mark_tile(size_t n, uint32_t *__restrict__ cnt, Keep keep) {
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  bool in[kCompactRounds];
  unsigned rank[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + threadIdx.x;
    in[k] = i < n && keep(i);
  }
  const unsigned total = compact_tile_ranks(in, rank, wcnt);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// The body of a place launch (the same geometry; cnt and sums as the mark launch and k_compact_chunks left them):
// kept(i) gives the flag of every element i < n of the tile; then each(i, at, in) runs for EVERY i < n, survivor
// (in) or not, with at = the survivors in front of i in the whole input: a survivor's position (< the survivors in all).
template <class Kept, class Each>
__device__ __forceinline__ void compact_place_tile(size_t n, const uint32_t *__restrict__ cnt,
                                                   const uint32_t *__restrict__ sums, Kept kept, Each each) {
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  __shared__ unsigned lds[kCompactWaves];
  const unsigned base = compact_tile_base(cnt, sums, blockIdx.x, lds);
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  bool in[kCompactRounds];
  unsigned rank[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + threadIdx.x;
    in[k] = i < n && kept(i);
  }
  (void)compact_tile_ranks(in, rank, wcnt);
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + threadIdx.x;
    if (i < n) each(i, (size_t)base + rank[k], in[k]);
  }
}

namespace {  // (a copy per translation unit that includes this: the library has no relocatable device code)

// sums[c] = the survivors of tiles [kCompactChunk c, kCompactChunk (c + 1))
__global__ __launch_bounds__(kCompactThreads) void k_compact_chunks(const uint32_t *__restrict__ cnt, unsigned tiles,
                                                                    uint32_t *__restrict__ sums) {
  __shared__ unsigned lds[kCompactWaves];
  const size_t t0 = (size_t)blockIdx.x * kCompactChunk;
  const size_t t1 = t0 + kCompactChunk < tiles ? t0 + kCompactChunk : tiles;
  unsigned s = 0;
  for (size_t t = t0 + threadIdx.x; t < t1; t += kCompactThreads) s += cnt[t];
  s = compact_block_sum(s, lds);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

[[maybe_unused]] hipError_t launch_compact_chunks(const uint32_t *cnt, unsigned tiles, uint32_t *sums, hipStream_t stream) {
  hipLaunchKernelGGL(k_compact_chunks, dim3(compact_chunks(tiles)), dim3(kCompactThreads), 0, stream, cnt, tiles, sums);
  return hipGetLastError();
}

// *total = the survivors in all: the chunk sums copied to the host on `stream`, which is waited for, and added up
[[maybe_unused]] hipError_t compact_total(const uint32_t *sums, unsigned chunks, hipStream_t stream, size_t *total) {
  std::vector<uint32_t> host(chunks);
  hipError_t e = hipMemcpyAsync(host.data(), sums, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return e;
  size_t t = 0;
  for (unsigned c = 0; c < chunks; ++c) t += host[c];
  *total = t;
  return hipSuccess;
}

}  // namespace
}  // namespace icp
