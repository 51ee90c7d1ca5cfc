// EXTENSION beyond the reference (include/icp_mi355x.h section 10): the gate of a registration with a maximum
// correspondence distance -- from a source cloud, a pose and the indices of a search, the pairs (xy(T src), xy(dst[idx]))
// of the INLIERS (d2 <= r * r, section 9's rule), written densely and in the order of the source cloud.
// The stable compaction of compact_device.hpp in two launches (qsort.hip's count launch + scatter launch is the pattern):
//   k_gate_stage<DIM>   a tile = 1 024 consecutive points.  A lane recomputes q, b and d2 of its four points (the ONE
//                       gather of dst), and the tile's survivors go -- compacted, in order -- to the start of the tile's
//                       own segment of the staging buffers (consecutive survivors = consecutive 16-byte stores); the
//                       tile's count goes to cnt[tile]
//   k_compact_chunks    only beyond kCompactChunk tiles (2^23 points): a workgroup of the next launch then reads at most
//                       kCompactChunk counts and the chunk sums in front of it
//   k_gate_place        a workgroup per tile: (survivors of the tiles in front) = where the tile's staged survivors
//                       go; it copies them there (streaming: no gather, no recomputation), and the workgroup of the
//                       last tile leaves the total in the handle's pinned result block
// No float reductions: like a survivor's position, its values are a pure function of the inputs.
#include "api_internal.hpp"
#include "compact_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

template <int DIM>
__global__ __launch_bounds__(kCompactThreads) void k_gate_stage(const double *__restrict__ src, unsigned n, Pose T,
                                                                const uint32_t *__restrict__ idx,
                                                                const double *__restrict__ dst, unsigned m, double r2,
                                                                double2 *__restrict__ st_a, double2 *__restrict__ st_b,
                                                                uint32_t *__restrict__ st_pos, uint32_t *__restrict__ cnt) {
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  const unsigned tid = threadIdx.x;
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  double2 a[kCompactRounds], b[kCompactRounds];
  unsigned rank[kCompactRounds];
  bool keep[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t i = first + k * kCompactThreads + tid;
    bool in = false;
    a[k] = make_double2(0., 0.);
    b[k] = make_double2(0., 0.);
    if (i < n) {
      const double px = src[i * DIM], py = src[i * DIM + 1];
      const double pz = DIM == 3 ? src[i * DIM + 2] : 0.;
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      uint32_t j = idx[i];
      if (j >= m) j = 0;  // (the search always answers j < m: this only keeps the read in bounds)
      const double *t = dst + (size_t)j * DIM;
      const double bx = t[0], by = t[1];
      const double ex = qx - bx, ey = qy - by;
      double d2 = ex * ex + ey * ey;
      if (DIM == 3) {
        const double dz = pz - t[2];
        d2 = d2 + dz * dz;
      }
      in = d2 <= r2;  // (false for a NaN d2)
      a[k] = make_double2(qx, qy);
      b[k] = make_double2(bx, by);
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
    st_a[at] = a[k];
    st_b[at] = b[k];
    if (st_pos) st_pos[at] = (uint32_t)(first + k * kCompactThreads + tid);
  }
  if (tid == 0) cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kCompactThreads) void k_gate_place(const double2 *__restrict__ st_a,
                                                                const double2 *__restrict__ st_b,
                                                                const uint32_t *__restrict__ st_pos,
                                                                const uint32_t *__restrict__ cnt,
                                                                const uint32_t *__restrict__ sums, unsigned tiles,
                                                                double2 *__restrict__ out_a, double2 *__restrict__ out_b,
                                                                uint32_t *__restrict__ out_pos, unsigned *__restrict__ h_total) {
  __shared__ unsigned lds[kCompactWaves];
  const unsigned tid = threadIdx.x, tile = blockIdx.x;
  const unsigned base = compact_tile_base(cnt, sums, tile, lds);
  const unsigned c = cnt[tile];
  const size_t from = (size_t)tile * kCompactTile;
  for (unsigned r = tid; r < c; r += kCompactThreads) {
    out_a[(size_t)base + r] = st_a[from + r];
    out_b[(size_t)base + r] = st_b[from + r];
    if (out_pos) out_pos[(size_t)base + r] = st_pos[from + r];
  }
  if (tile + 1 == tiles && tid == 0) *h_total = base + c;  // (pinned host memory: there when the stream's wait returns)
}

namespace api {

// Enqueues the gate on h->stream (the workspace holds n points: ensure_workspace).  Staging: the third pair buffers;
// counts, chunk sums and the staged positions: the residual buffers -- nothing of an evaluation is in flight on this
// stream's scratch while a gate runs, and the next evaluation starts behind it.  The count is in h_res->pad once the
// stream has been waited for (gate_count).
hipError_t launch_gate(icp_handle *h, const double *d_src, size_t n, const Pose &T, const uint32_t *d_idx, double r2,
                       double *d_a, double *d_b, uint32_t *d_kept) {
  Workspace &w = h->ws;
  w.h_res->pad = 0;
  if (n == 0) return hipSuccess;
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  // (cap_n >= 256 doubles per residual buffer: tiles + chunks words fit -- a word per 1 024 points and one per 2^23)
  uint32_t *cnt = reinterpret_cast<uint32_t *>(w.d_ry), *sums = cnt + tiles;
  uint32_t *st_pos = d_kept ? reinterpret_cast<uint32_t *>(w.d_rx) : nullptr;
  double2 *st_a = reinterpret_cast<double2 *>(w.d_a3), *st_b = reinterpret_cast<double2 *>(w.d_b3);
  if (h->dim == 2)
    hipLaunchKernelGGL(k_gate_stage<2>, dim3(tiles), dim3(kCompactThreads), 0, h->stream, d_src, (unsigned)n, T, d_idx,
                       h->d_dst, (unsigned)h->m, r2, st_a, st_b, st_pos, cnt);
  else
    hipLaunchKernelGGL(k_gate_stage<3>, dim3(tiles), dim3(kCompactThreads), 0, h->stream, d_src, (unsigned)n, T, d_idx,
                       h->d_dst, (unsigned)h->m, r2, st_a, st_b, st_pos, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (chunks > 1 && (e = launch_compact_chunks(cnt, tiles, sums, h->stream)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_gate_place, dim3(tiles), dim3(kCompactThreads), 0, h->stream, (const double2 *)st_a,
                     (const double2 *)st_b, (const uint32_t *)st_pos, (const uint32_t *)cnt, (const uint32_t *)sums,
                     tiles, reinterpret_cast<double2 *>(d_a), reinterpret_cast<double2 *>(d_b), d_kept, &w.h_res->pad);
  return hipGetLastError();
}

size_t gate_count(const icp_handle *h) { return h->ws.h_res->pad; }

}  // namespace api
}  // namespace icp

extern "C" int icp_gate_pairs_device(icp_handle *h, const double *d_src, size_t n, const icp_pose *T,
                                     const uint32_t *d_idx, double max_dist, double *d_a, double *d_b, uint32_t *d_kept,
                                     size_t *kept) {
  // (max_dist >= 0 is false for a NaN)
  if (!h || !T || !kept || (n > 0 && (!d_src || !d_idx || !d_a || !d_b)) || !(max_dist >= 0.) || n >= 0xffffffffull)
    return ICP_BAD_ARGUMENT;
  *kept = 0;
  if (n == 0) return ICP_OK;
  if (!have_device()) return ICP_NO_DEVICE;
  if (h->m == 0) return ICP_EMPTY_DST;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(ensure_workspace(h, workspace_points(n), false));
  HIP_TRY(launch_gate(h, d_src, n, *T, d_idx, max_dist * max_dist, d_a, d_b, d_kept));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *kept = gate_count(h);
  return ICP_OK;
}
