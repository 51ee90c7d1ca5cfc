// EXTENSION beyond the reference (include/icp_mi355x.h section 11): the sliding-window map -- icp_crop_targets keeps the
// targets of a handle that lie in a disc of the xy plane and lets go of the others; the counterpart of
// icp_append_targets (section 6).  Two STABLE compactions (compact_device.hpp): a mark launch that counts the survivors
// of every tile of 1 024 consecutive elements, the chunk-sum launch k_compact_chunks (always run here: its sums are also
// how the host learns the total) and a place launch in which a workgroup per tile adds up the counts in front of it and
// moves its survivors there.  k_crop_mark, k_crop_place and k_crop_rec_mark are compact_mark_tile / compact_place_tile
// of that header with their rule as a lambda (k_crop_rec_place is written out: see there); the host learns a total
// through its compact_total.
//   targets  k_crop_mark<DIM>      w[i] = kept ? 0 : kCropGone by the keep rule, cnt[tile]
//             k_crop_place<DIM>     w[i] = the new index of target i (or kCropGone): the new_index table; the points, and
//                                   the normals where present, move to their new index in a second buffer
//   records   k_crop_rec_mark       the grid's records are cell-sorted and removing records keeps them sorted: the
//             k_crop_rec_place      record at sorted position p survives iff new_index[pts[p].idx] is valid and moves to
//                                   the number of survivors in front of it, its idx rewritten; that number is left in
//                                   w[p] for EVERY p, so that
//             k_crop_starts         start2[c] = w[start[c]] (one gather), and the sentinel records follow the last one
// The host side is in two halves (api_internal.hpp): target_marks hands out the mark and count words, and
// remove_marked_targets does everything behind a mark launch; icp_crop_targets runs k_crop_mark between them and
// icp_thin_targets (voxel.hip) its own keep rule.
// No float reductions.  The grid keeps the box and the cell size of its last full build (upper bounds of the kept
// cloud's: exact, like the grid of an incremental append).
#include <cmath>
#include <utility>

#include "api_internal.hpp"
#include "compact_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace {

// The kept cloud has fallen below 1 / kRebuildShrink of the cloud the grid's cell size was chosen for: rebuild (the
// mirror of append_grid's kRebuildGrowth)
constexpr double kRebuildShrink = 1.5;

}  // namespace

// The keep rule (include/icp_mi355x.h section 11): dx = x - cx, dy = y - cy, d2 = dx dx + dy dy (no FMA: the library is
// compiled with -ffp-contract=off), kept iff d2 <= r2 (false for a NaN d2).  z takes no part.
template <int DIM>
__global__ __launch_bounds__(kCompactThreads) void k_crop_mark(const double *__restrict__ dst, unsigned m, double cx, double cy,
                                                            double r2, uint32_t *__restrict__ w,
                                                            uint32_t *__restrict__ cnt) {
  compact_mark_tile(m, cnt, [=](size_t i) {
    const double dx = dst[i * DIM] - cx, dy = dst[i * DIM + 1] - cy;
    const double d2 = dx * dx + dy * dy;
    const bool in = d2 <= r2;
    w[i] = in ? 0u : kCropGone;
    return in;
  });
}

// w: in, the marks; out, the new_index table.  *normals_kept (nullable) receives the survivors among the first
// normals_m targets when normals_m < m (the host knows it otherwise: all of them).
template <int DIM>
__global__ __launch_bounds__(kCompactThreads) void k_crop_place(const double *__restrict__ dst,
                                                             const double *__restrict__ normals, unsigned normals_m,
                                                             unsigned m, uint32_t *__restrict__ w,
                                                             const uint32_t *__restrict__ cnt,
                                                             const uint32_t *__restrict__ sums, double *__restrict__ out,
                                                             double *__restrict__ out_normals,
                                                             uint32_t *__restrict__ normals_kept) {
  compact_place_tile(
      m, cnt, sums, [=](size_t i) { return w[i] != kCropGone; },
      [=](size_t i, size_t at, bool in) {  // (a survivor's at: inside a buffer that holds the survivors)
        if (normals_kept && i == normals_m) *normals_kept = (uint32_t)at;
        if (!in) return;
        w[i] = (uint32_t)at;
#pragma unroll
        for (int d = 0; d < DIM; ++d) out[at * DIM + d] = dst[i * DIM + d];
        if (out_normals && i < normals_m) {
#pragma unroll
          for (int d = 0; d < 3; ++d) out_normals[at * 3 + d] = normals[i * 3 + d];
        }
      });
}

// w[p] = the new index of the target behind the record at sorted position p (kCropGone: removed)
__global__ __launch_bounds__(kCompactThreads) void k_crop_rec_mark(const GridPoint *__restrict__ pts, unsigned m,
                                                                const uint32_t *__restrict__ new_index,
                                                                uint32_t *__restrict__ w, uint32_t *__restrict__ cnt) {
  compact_mark_tile(m, cnt, [=](size_t p) {
    const uint32_t j = pts[p].idx;
    const uint32_t to = j < m ? new_index[j] : kCropGone;  // (a record's idx is always < m: this only keeps the read in bounds)
    w[p] = to;
    return to != kCropGone;
  });
}

// w: in, the records' new indices; out, for EVERY sorted position p the survivors in front of it
__global__ __launch_bounds__(kCompactThreads) void k_crop_rec_place(const GridPoint *__restrict__ pts, unsigned m,
                                                                 uint32_t *__restrict__ w, const uint32_t *__restrict__ cnt,
                                                                 const uint32_t *__restrict__ sums,
                                                                 GridPoint *__restrict__ pts2) {
  // Not compact_place_tile: a place needs the word it read for the flag again (the record's new idx), and read through
  // the body's kept(p) the tile's four loads are each waited for before the next is issued, where the loads into to[]
  // below are in flight together (profiles/compact_bodies_ab.txt: + 1 us on an 83 us crop of 1M targets).
  __shared__ unsigned wcnt[kCompactRounds][kCompactWaves];
  __shared__ unsigned lds[kCompactWaves];
  const unsigned base = compact_tile_base(cnt, sums, blockIdx.x, lds);
  const size_t first = (size_t)blockIdx.x * kCompactTile;
  bool in[kCompactRounds];
  unsigned rank[kCompactRounds];
  uint32_t to[kCompactRounds];
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t p = first + k * kCompactThreads + threadIdx.x;
    to[k] = p < m ? w[p] : kCropGone;
    in[k] = to[k] != kCropGone;
  }
  (void)compact_tile_ranks(in, rank, wcnt);
#pragma unroll
  for (unsigned k = 0; k < kCompactRounds; ++k) {
    const size_t p = first + k * kCompactThreads + threadIdx.x;
    if (p >= m) continue;
    const size_t at = (size_t)base + rank[k];
    w[p] = (uint32_t)at;
    if (!in[k]) continue;
    GridPoint r = pts[p];
    r.idx = to[k];
    pts2[at] = r;
  }
}

// start2[c] = the survivors in front of sorted position start[c] (pos[] of k_crop_rec_place; start[c] == m: all of
// them); the threads behind the cell offsets write the sentinel records behind the last survivor
__global__ void k_crop_starts(const uint32_t *__restrict__ start, unsigned nscan, const uint32_t *__restrict__ pos,
                              unsigned m, unsigned kept, uint32_t *__restrict__ start2, GridPoint *__restrict__ pts2) {
  const unsigned c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nscan) {
    const uint32_t s = start[c];
    start2[c] = s < m ? pos[s] : kept;
  } else if (c < nscan + kGridPad) {
    pts2[(size_t)kept + (c - nscan)] = GridPoint{__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf(), 0u};
  }
}

namespace {

int crop_quiesce(icp_handle *h) {
  HIP_TRY(hipSetDevice(h->device));
  if (h->own_stream) HIP_TRY(hipStreamSynchronize(h->own_stream));
  if (h->stream != h->own_stream) HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->ws.spec_stream) HIP_TRY(hipStreamSynchronize(h->ws.spec_stream));
  return ICP_OK;
}

// the second compaction: the grid's records into the second set of the sorted arrays (nothing of the handle changes
// here; the caller swaps the sets on success)
hipError_t crop_move_records(icp_handle *h, unsigned m_old, unsigned kept, const uint32_t *new_index, uint32_t *cnt) {
  Grid &G = h->grid;
  hipStream_t s = h->stream;
  hipError_t e;
  const unsigned nscan = G.ncell + 1, tiles = compact_tiles(m_old);
  uint32_t *sums = cnt + tiles;
  if ((e = reserve(G.d_pts2, G.cap_pts2, (size_t)kept + kGridPad)) != hipSuccess) return e;
  if ((e = reserve(G.d_start2, G.cap_start2, (size_t)nscan)) != hipSuccess) return e;
  if ((e = reserve(G.d_rcell2, G.cap_rcell2, (size_t)m_old)) != hipSuccess) return e;  // (free between appends: the marks)
  uint32_t *w = G.d_rcell2;
  hipLaunchKernelGGL(k_crop_rec_mark, dim3(tiles), dim3(kCompactThreads), 0, s, (const GridPoint *)G.d_pts, m_old, new_index, w,
                     cnt);
  if ((e = launch_compact_chunks(cnt, tiles, sums, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_crop_rec_place, dim3(tiles), dim3(kCompactThreads), 0, s, (const GridPoint *)G.d_pts, m_old, w,
                     (const uint32_t *)cnt, (const uint32_t *)sums, G.d_pts2);
  hipLaunchKernelGGL(k_crop_starts, dim3((nscan + kGridPad + 255) / 256), dim3(256), 0, s, (const uint32_t *)G.d_start, nscan,
                     (const uint32_t *)w, m_old, kept, G.d_start2, G.d_pts2);
  return hipGetLastError();
}

}  // namespace

int api::target_marks(icp_handle *h, uint32_t **w, uint32_t **cnt) {
  ICP_TRY_RC(crop_quiesce(h));
  Grid &G = h->grid;
  const unsigned tiles = compact_tiles(h->m), chunks = compact_chunks(tiles);
  // the marks, later the new_index table: the grid's build temporary of m words, free between builds; the tile counts,
  // the chunk sums and one word for the normals: the append's shift table, free between appends
  HIP_TRY(reserve(G.t_cell_of, G.cap_tcell, h->m));
  HIP_TRY(reserve(G.t_shift, G.cap_shift, (size_t)tiles + chunks + 1));
  *w = G.t_cell_of;
  *cnt = G.t_shift;
  return ICP_OK;
}

int api::remove_marked_targets(icp_handle *h, uint32_t *w, uint32_t *cnt, unsigned long long &moved,
                               unsigned long long &rebuilt, uint32_t *new_index, size_t *removed) {
  Grid &G = h->grid;
  hipStream_t s = h->stream;
  const unsigned m_old = (unsigned)h->m, tiles = compact_tiles(m_old), chunks = compact_chunks(tiles);
  const int dim = h->dim;
  uint32_t *sums = cnt + tiles, *aux = sums + chunks;
  HIP_TRY(launch_compact_chunks(cnt, tiles, sums, s));
  size_t kept_ = 0;
  HIP_TRY(compact_total(sums, chunks, s, &kept_));
  const unsigned kept = (unsigned)kept_;
  if (kept == m_old) {  // nothing to remove: the handle is left exactly as it was
    if (new_index)
      for (unsigned i = 0; i < m_old; ++i) new_index[i] = i;
    return ICP_OK;
  }
  // ---- out of place: the kept points (and normals) into the second buffers ----
  const bool with_normals = h->d_normals && h->normals_m > 0;  // (a 2-D handle's line normals are m x 3 too)
  const unsigned normals_m = with_normals ? (unsigned)h->normals_m : 0u;
  if (kept > 0) {
    HIP_TRY(reserve(h->d_dst_alt, h->cap_dst_alt, (size_t)kept * dim));
    if (with_normals) HIP_TRY(reserve(h->d_normals_alt, h->cap_normals_alt, (size_t)kept * 3));
  }
  const bool count_normals = with_normals && normals_m < m_old;
  if (kept > 0 || new_index || count_normals) {
    if (dim == 3)
      hipLaunchKernelGGL(k_crop_place<3>, dim3(tiles), dim3(kCompactThreads), 0, s, h->d_dst, (const double *)h->d_normals,
                         normals_m, m_old, w, (const uint32_t *)cnt, (const uint32_t *)sums, h->d_dst_alt,
                         with_normals && kept > 0 ? h->d_normals_alt : nullptr, count_normals ? aux : nullptr);
    else
      hipLaunchKernelGGL(k_crop_place<2>, dim3(tiles), dim3(kCompactThreads), 0, s, h->d_dst, (const double *)h->d_normals,
                         normals_m, m_old, w, (const uint32_t *)cnt, (const uint32_t *)sums, h->d_dst_alt,
                         with_normals && kept > 0 ? h->d_normals_alt : nullptr, count_normals ? aux : nullptr);
    HIP_TRY(hipGetLastError());
  }
  size_t normals_after = with_normals ? kept : 0;
  if (count_normals) {
    uint32_t counted = 0;
    HIP_TRY(hipMemcpyAsync(&counted, aux, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    normals_after = counted;
  }
  if (new_index) {
    HIP_TRY(hipMemcpyAsync(new_index, w, (size_t)m_old * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  // ---- the grid: move the sorted records, unless there is none or its cell size is due for a re-tune ----
  const bool move = G.built && kept > 0 && G.m_full > 0 && !((double)kept < (double)G.m_full / kRebuildShrink);
  if (move) HIP_TRY(crop_move_records(h, m_old, kept, w, cnt));
  HIP_TRY(hipStreamSynchronize(s));
  // ---- success so far: swap.  What is kept for a way back: the old cloud's buffers (they become the second set) ----
  const double *old_dst = h->d_dst;
  const bool old_owns = h->owns_dst;
  const size_t old_normals_m = h->normals_m;
  if (kept > 0) {
    std::swap(h->d_dst_own, h->d_dst_alt);
    std::swap(h->cap_dst_own, h->cap_dst_alt);
    if (with_normals) {
      std::swap(h->d_normals, h->d_normals_alt);
      std::swap(h->cap_normals, h->cap_normals_alt);
    }
  }
  h->d_dst = h->d_dst_own;
  h->owns_dst = true;  // (a handle from icp_create_device stops borrowing, as at its first append)
  h->m = kept;
  h->normals_m = normals_after;
  h->qsort.valid = false;  // snapshots and previous matches refer to the old cloud
  h->qsort.have_prev = false;
  h->brute_valid = h->screen_valid = false;
  hipError_t e = hipSuccess;
  if (move) {
    std::swap(G.d_pts, G.d_pts2);
    std::swap(G.cap_pts, G.cap_pts2);
    std::swap(G.d_start, G.d_start2);
    std::swap(G.cap_start, G.cap_start2);
    G.rcell_valid = false;  // (the next incremental append derives it from the cell offsets again)
  } else {
    e = build_grid(h);
  }
  if (e == hipSuccess && resolved_nn_mode(h) == ICP_NN_BRUTE) {
    if ((e = build_target_soa(h)) == hipSuccess) e = build_target_screen(h);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    // back to the cloud as it was: its points and normals were never written; the search structures are rebuilt for
    // them (only a rebuild can fail here: the moved records were complete before the swap)
    if (kept > 0) {
      std::swap(h->d_dst_own, h->d_dst_alt);
      std::swap(h->cap_dst_own, h->cap_dst_alt);
      if (with_normals) {
        std::swap(h->d_normals, h->d_normals_alt);
        std::swap(h->cap_normals, h->cap_normals_alt);
      }
    }
    h->d_dst = old_dst;
    h->owns_dst = old_owns;
    h->m = m_old;
    h->normals_m = old_normals_m;
    (void)build_grid(h);
    (void)hipStreamSynchronize(s);
    return map_hip(e);
  }
  ++(move ? moved : rebuilt);
  if (removed) *removed = (size_t)m_old - kept;
  return ICP_OK;
}

namespace {

int crop_targets(icp_handle *h, double cx, double cy, double radius, uint32_t *new_index, size_t *removed) {
  if (removed) *removed = 0;
  if (h->m == 0) {
    ICP_TRY_RC(crop_quiesce(h));
    return ICP_OK;
  }
  uint32_t *w, *cnt;
  ICP_TRY_RC(target_marks(h, &w, &cnt));
  const unsigned m_old = (unsigned)h->m, tiles = compact_tiles(m_old);
  const double r2 = radius * radius;
  if (h->dim == 3)
    hipLaunchKernelGGL(k_crop_mark<3>, dim3(tiles), dim3(kCompactThreads), 0, h->stream, h->d_dst, m_old, cx, cy, r2, w, cnt);
  else
    hipLaunchKernelGGL(k_crop_mark<2>, dim3(tiles), dim3(kCompactThreads), 0, h->stream, h->d_dst, m_old, cx, cy, r2, w, cnt);
  return remove_marked_targets(h, w, cnt, h->grid.crops_moved, h->grid.crops_rebuilt, new_index, removed);
}

}  // namespace
}  // namespace icp

extern "C" int icp_crop_targets(icp_handle *h, const double center_xy[2], double radius, uint32_t *new_index,
                                size_t *removed) {
  // (radius >= 0 is false for a NaN; so is c == c)
  if (!h || !center_xy || !(center_xy[0] == center_xy[0]) || !(center_xy[1] == center_xy[1]) || !(radius >= 0.))
    return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  return crop_targets(h, center_xy[0], center_xy[1], radius, new_index, removed);
}

// Observability: out[0] = crops served by moving the grid's sorted records, out[1] = crops that rebuilt the grid
extern "C" int icp_grid_crop_counters(const icp_handle *h, uint64_t out[2]) {
  if (!h || !out) return ICP_BAD_ARGUMENT;
  out[0] = h->grid.crops_moved;
  out[1] = h->grid.crops_rebuilt;
  return ICP_OK;
}
