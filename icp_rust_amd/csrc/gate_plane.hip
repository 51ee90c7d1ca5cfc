// EXTENSION beyond the reference (include/icp_mi355x.h section 12): the gate of a POINT-TO-PLANE registration with a
// maximum correspondence distance -- from a source cloud, a pose, the indices of a search and the targets' normals, the
// PlanePair (p2plane_device.hpp: what k_p2pl_gather writes for every point) of the INLIERS only (d2 <= r * r, section
// 9's rule), written densely and in the order of the source cloud.  The stable compaction of compact_device.hpp around
// the wider record:
//   k_plgate_stage    a tile = 1 024 consecutive points.  A lane does the ONE gather of dst[j] and normals[j] of its four
//                     points and computes d2 and the eight values, and the tile's survivors go -- compacted, in order --
//                     to the start of the tile's own segment of the staging buffer (a survivor = four 16-byte stores,
//                     consecutive survivors = consecutive 64 bytes); the tile's count goes to cnt[tile]
//   k_compact_chunks  only beyond kCompactChunk tiles (2^23 points): the counts of every kCompactChunk tiles added up
//   k_plgate_place    a workgroup per tile: (survivors of the tiles in front) = where the tile's staged survivors go; it
//                     streams them there, 16 bytes per lane and step, and the workgroup of the last tile leaves the
//                     total in the handle's pinned result block
// No float reductions: like a survivor's position, its values are a pure function of the inputs.
// The gate of a POINT-TO-LINE registration on a 2-D handle (section 14) is the same with k_lngate_stage as the first
// launch: one stage body for both dimensions (normal_gate_stage<DIM>), one place kernel, one host driver.
#include "api_internal.hpp"
#include "compact_device.hpp"
#include "p2plane_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

constexpr unsigned kPairWords = sizeof(PlanePair) / sizeof(double2);  // 16-byte words of a pair
static_assert(sizeof(PlanePair) == 64 && kPairWords == 4, "a pair is four 16-byte words");

// The stage launch's body, DIM = 3 (k_plgate_stage) or 2 (k_lngate_stage: the clouds read at a stride of 2, d2 = ex ex +
// ey ey -- section 9's rule in the plane --, dz = 0, nz = 0).  Between the rounds the 2-D form holds THREE 16-byte words
// per point, (nx, ny) in the third, and forms (0, nx) | (ny, 0) at the store: a fourth word costs it registers.
template <int DIM>
__device__ __forceinline__ void normal_gate_stage(const double *__restrict__ src, unsigned n, const Pose &T,
                                                  const uint32_t *__restrict__ idx, const double *__restrict__ dst,
                                                  unsigned m, const double *__restrict__ normals, double r2,
                                                  double2 *__restrict__ st_pairs, uint32_t *__restrict__ st_pos,
                                                  uint32_t *__restrict__ cnt) {
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  const unsigned tid = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  double2 w0[kCompactRounds], w1[kCompactRounds], w2[kCompactRounds], w3[DIM == 3 ? kCompactRounds : 1];
  unsigned rank[kCompactRounds];
  bool keep[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + tid;
    bool in = false;
    w0[k] = w1[k] = w2[k] = make_double2(0., 0.);
    if constexpr (DIM == 3) w3[k] = make_double2(0., 0.);
    if (i < n) {
      const double px = src[i * DIM], py = src[i * DIM + 1];
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      uint32_t j = idx[i];
      if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the reads in bounds)
      const double *t = dst + (size_t)j * DIM, *nj = normals + (size_t)j * 3;
      const double bx = t[0], by = t[1];
      const double nx = nj[0], ny = nj[1];
      const double ex = qx - bx, ey = qy - by;
      double d2 = ex * ex + ey * ey;
      w0[k] = make_double2(qx, qy);  // PlanePair: ax, ay | qx, qy | dz, nx | ny, nz
      w1[k] = make_double2(bx, by);
      if constexpr (DIM == 3) {
        const double dz = src[i * DIM + 2] - t[2];
        d2 = d2 + dz * dz;
        w2[k] = make_double2(dz, nx);
        w3[k] = make_double2(ny, nj[2]);
      } else {
        w2[k] = make_double2(nx, ny);
      }
      in = d2 <= r2;  // (false for a NaN d2)
    }
    rank[k] = compact_wave_rank(__ballot(in), wcnt[k]);
    keep[k] = in;
  }
  __syncthreads();
  unsigned total = 0;
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    unsigned before = 0;  // (apart from rank[k]: summed into it, the kernel takes more registers)
    compact_round_offset(before, wcnt[k], total);
    if (!keep[k]) continue;
    const size_t at = first + before + rank[k];  // (< first + the tile's points: inside the tile's own segment)
    double2 *o = st_pairs + at * kPairWords;
    o[0] = w0[k];
    o[1] = w1[k];
    if constexpr (DIM == 3) {
      o[2] = w2[k];
      o[3] = w3[k];
    } else {
      o[2] = make_double2(0., w2[k].x);
      o[3] = make_double2(w2[k].y, 0.);
    }
    if (st_pos) st_pos[at] = (uint32_t)(first + k * kCompactThreads + tid);
  }
  if (tid == 0) cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCompactThreads) void k_plgate_stage(const double *__restrict__ src, unsigned n, Pose T,
                                                                  const uint32_t *__restrict__ idx,
                                                                  const double *__restrict__ dst, unsigned m,
                                                                  const double *__restrict__ normals, double r2,
                                                                  double2 *__restrict__ st_pairs,
                                                                  uint32_t *__restrict__ st_pos,
                                                                  uint32_t *__restrict__ cnt) {
  normal_gate_stage<3>(src, n, T, idx, dst, m, normals, r2, st_pairs, st_pos, cnt);
}

__global__ __launch_bounds__(kCompactThreads) void k_lngate_stage(const double *__restrict__ src, unsigned n, Pose T,
                                                                  const uint32_t *__restrict__ idx,
                                                                  const double *__restrict__ dst, unsigned m,
                                                                  const double *__restrict__ normals, double r2,
                                                                  double2 *__restrict__ st_pairs,
                                                                  uint32_t *__restrict__ st_pos,
                                                                  uint32_t *__restrict__ cnt) {
  normal_gate_stage<2>(src, n, T, idx, dst, m, normals, r2, st_pairs, st_pos, cnt);
}

__global__ __launch_bounds__(kCompactThreads) void k_plgate_place(const double2 *__restrict__ st_pairs,
                                                                  const uint32_t *__restrict__ st_pos,
                                                                  const uint32_t *__restrict__ cnt,
                                                                  const uint32_t *__restrict__ sums, unsigned tiles,
                                                                  double2 *__restrict__ out_pairs,
                                                                  uint32_t *__restrict__ out_pos,
                                                                  unsigned *__restrict__ h_total) {
  __shared__ unsigned lds[kCompactWaves];
  const unsigned tid = threadIdx.x, tile = blockIdx.x;
  const unsigned base = compact_tile_base(cnt, sums, tile, lds);
  const unsigned c = cnt[tile];  // (<= the tile's points: every read below stays inside the tile's segment)
  const double2 *from = st_pairs + (size_t)tile * kCompactTile * kPairWords;
  double2 *to = out_pairs + (size_t)base * kPairWords;
  for (unsigned r = tid; r < c * kPairWords; r += kCompactThreads) to[r] = from[r];
  if (out_pos)
    for (unsigned r = tid; r < c; r += kCompactThreads) out_pos[(size_t)base + r] = st_pos[(size_t)tile * kCompactTile + r];
  if (tile + 1 == tiles && tid == 0) *h_total = base + c;  // (pinned host memory: there when the stream's wait returns)
}

namespace api {

// Enqueues the gate on h->stream (the workspace holds max(n, 256) points: ensure_workspace; h->d_plane_stage holds n
// pairs: ensure_plane_stage; h->d_normals is current).  Counts, chunk sums and the staged positions: the residual
// buffers, as in launch_gate -- nothing of an evaluation is in flight on this stream's scratch while a gate runs, and the
// next evaluation starts behind it.  The count is in h_res->pad once the stream has been waited for (gate_count).
hipError_t launch_gate_normal(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx, double r2,
                              void *d_pairs, uint32_t *d_kept) {
  Workspace &w = h->ws;
  w.h_res->pad = 0;
  if (n == 0) return hipSuccess;
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  // (cap_n >= 256 doubles per residual buffer: tiles + chunks words fit -- a word per 1 024 points and one per 2^23)
  uint32_t *cnt = reinterpret_cast<uint32_t *>(w.d_ry), *sums = cnt + tiles;
  uint32_t *st_pos = d_kept ? reinterpret_cast<uint32_t *>(w.d_rx) : nullptr;
  double2 *st = reinterpret_cast<double2 *>(h->d_plane_stage);
  hipLaunchKernelGGL(h->dim == 3 ? k_plgate_stage : k_lngate_stage, dim3(tiles), dim3(kCompactThreads), 0, h->stream, d_src,
                     (unsigned)n, T, d_idx, h->d_dst, (unsigned)h->m, (const double *)h->d_normals, r2, st, st_pos, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (chunks > 1 && (e = launch_compact_chunks(cnt, tiles, sums, h->stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_plgate_place, dim3(tiles), dim3(kCompactThreads), 0, h->stream, (const double2 *)st,
                     (const uint32_t *)st_pos, (const uint32_t *)cnt, (const uint32_t *)sums, tiles,
                     reinterpret_cast<double2 *>(d_pairs), d_kept, &w.h_res->pad);
  return hipGetLastError();
}

}  // namespace api
}  // namespace icp
