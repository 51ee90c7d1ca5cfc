// EXTENSION beyond the reference (include/icp_mi355x.h section 22): voxel thinning -- keep the first point of every voxel,
// in order.  icp_voxel_downsample[_device] thin a cloud; icp_thin_targets applies the same rule to a handle's targets
// through the back half of the crop (crop.hip: remove_marked_targets).
//   the rule  cell_a = floor(p_a / v) + 0.0 in f64 (one IEEE division, never a product with 1 / v; + 0.0 makes a -0.0
//             quotient +0.0); two points share a voxel iff their cells compare equal on every axis (+-inf is a cell like
//             any other); a point with a NaN or infinite coordinate is in no voxel and is dropped; of every voxel the
//             point with the lowest index is kept.
//   the table open addressing, linear probing, 2^ceil(log2(2 n)) words (at least 2) preset to kVoxelEmpty; a word holds
//             the index of a point of the voxel that owns the slot.
//             k_voxel_insert<DIM>  point i walks from the hash of its cell: atomicCAS(slot, empty, i) claims an empty
//                                  slot; a taken slot's owner is looked up in the (read-only) cloud: the same cell ->
//                                  atomicMin(slot, i) and done, another cell -> the next slot.  A slot never becomes
//                                  empty again and never changes its voxel; its word only decreases.  So every thread
//                                  of a voxel walks the same slots and ends on the same one, whatever the order they
//                                  arrive in, and the word ends as the voxel's lowest index: a pure function of the
//                                  input.  No thread waits for another: at most `slots` probes at a load of <= 0.5.
//                                  Of the lanes of a wave that share the cell of its first inserting lane only that
//                                  lane walks (it has the lowest index of them).
//             k_voxel_mark<DIM>    walks the same slots read-only: kept iff the walk ends on a word that holds i;
//                                  w[i] = kept ? 0 : kCropGone, cnt[tile] (compact_device.hpp: compact_mark_tile with
//                                  this rule)
//             k_voxel_place<DIM>   the stand-alone call's compaction: kept points and / or their indices
//                                  (compact_place_tile)
//             launch_voxel_front   what both stand-alone calls (this file's and voxel_mean.hip's) begin with: table, marks,
//                                  chunk sums; they end with compact_total
// No float reductions.  The hash only chooses where a walk starts: it has no part in the result.
// The cell, the hash, the read-only walk and the workspace are voxel_device.hpp's: voxel_mean.hip (section 25) shares them.
#include <cfloat>
#include <cmath>
#include <map>
#include <mutex>

#include "api_internal.hpp"
#include "compact_device.hpp"
#include "voxel_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {

template <int DIM>
__global__ __launch_bounds__(kVoxelThreads) void k_voxel_insert(const double *__restrict__ pts, size_t n, double v,
                                                                uint32_t *__restrict__ tab, size_t mask) {
  const size_t i = (size_t)blockIdx.x * kVoxelThreads + threadIdx.x;
  double c[3], o[3];
  const bool live = voxel_cell<DIM>(pts, i < n ? i : n - 1, v, c) && i < n;
  // A lane whose cell is that of the wave's first inserting lane adds nothing: that lane holds a lower index of the same
  // voxel (indices ascend with the lanes), and the word ends as the voxel's lowest index with or without this one.  A
  // cloud crowded into one voxel then sends one lane per wave to the voxel's word, not sixty-four.
  const unsigned long long all = __ballot(live);
  if (all == 0ull) return;
  const int lead = __ffsll((long long)all) - 1;
  double c0[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c0[a] = __shfl(c[a], lead, 64);
  if (!live || ((int)(threadIdx.x & 63u) != lead && voxel_same(c, c0))) return;
  size_t s = (size_t)voxel_hash(c) & mask;
  for (size_t probe = 0; probe <= mask; ++probe) {
    const uint32_t cur = atomicCAS(&tab[s], kVoxelEmpty, (uint32_t)i);
    if (cur == kVoxelEmpty || cur >= n) return;  // (the slot is this point's voxel's now; a word is always < n)
    (void)voxel_cell<DIM>(pts, cur, v, o);
    if (voxel_same(c, o)) {
      if (i < cur) (void)atomicMin(&tab[s], (uint32_t)i);
      return;
    }
    s = (s + 1) & mask;
  }
}

template <int DIM>
__global__ __launch_bounds__(kCompactThreads) void k_voxel_mark(const double *__restrict__ pts, size_t n, double v,
                                                                const uint32_t *__restrict__ tab, size_t mask,
                                                                uint32_t *__restrict__ w, uint32_t *__restrict__ cnt) {
  compact_mark_tile(n, cnt, [=](size_t i) {
    double c[3];
    const bool in = voxel_cell<DIM>(pts, i, v, c) && voxel_leader<DIM>(pts, n, v, tab, mask, i, c) == (uint32_t)i;
    w[i] = in ? 0u : kCropGone;
    return in;
  });
}

// out (nullable): the kept points; kept_index (nullable): their indices in the input
template <int DIM>
__global__ __launch_bounds__(kCompactThreads) void k_voxel_place(const double *__restrict__ pts, size_t n,
                                                                 const uint32_t *__restrict__ w,
                                                                 const uint32_t *__restrict__ cnt,
                                                                 const uint32_t *__restrict__ sums, double *__restrict__ out,
                                                                 uint32_t *__restrict__ kept_index) {
  compact_place_tile(
      n, cnt, sums, [=](size_t i) { return w[i] != kCropGone; },
      [=](size_t i, size_t at, bool in) {
        if (!in) return;  // (a kept point's at: < the kept points in all, which are <= n)
        if (kept_index) kept_index[at] = (uint32_t)i;
        if (out) {
#pragma unroll
          for (int d = 0; d < DIM; ++d) out[at * DIM + d] = pts[i * DIM + d];
        }
      });
}

namespace {
std::mutex g_mu;
std::map<int, VoxelWs> g_ws;
}  // namespace

std::mutex &voxel_mutex() { return g_mu; }
VoxelWs &voxel_ws(int device) { return g_ws[device]; }

bool voxel_size_ok(double v) { return v >= DBL_MIN && v <= DBL_MAX; }  // (false for a NaN)

static size_t voxel_slots(size_t n) {
  size_t slots = 2;
  while (slots < 2 * n) slots <<= 1;
  return slots;
}

// the table for n points, preset on `s` (a table grows to the next power of two: geometric by construction)
hipError_t voxel_table(VoxelWs &W, size_t n, hipStream_t s, size_t *mask) {
  const size_t slots = voxel_slots(n);
  hipError_t e;
  if (slots > W.cap_tab || !W.tab) {
    if (W.tab) (void)hipFree(W.tab);
    W.tab = nullptr;
    W.cap_tab = 0;
    if ((e = hipMalloc(&W.tab, slots * sizeof(uint32_t))) != hipSuccess) return e;
    W.cap_tab = slots;
  }
  *mask = slots - 1;
  return hipMemsetAsync(W.tab, 0xff, slots * sizeof(uint32_t), s);
}

// the insert and the mark launch on `s`: w[i] and cnt[tile] for the n > 0 points of d_pts
hipError_t launch_voxel_marks(int dim, const double *d_pts, size_t n, double v, uint32_t *tab, size_t mask,
                              uint32_t *w, uint32_t *cnt, hipStream_t s) {
  const unsigned blocks = (unsigned)((n + kVoxelThreads - 1) / kVoxelThreads), tiles = compact_tiles(n);
  if (dim == 3) {
    hipLaunchKernelGGL(k_voxel_insert<3>, dim3(blocks), dim3(kVoxelThreads), 0, s, d_pts, n, v, tab, mask);
    hipLaunchKernelGGL(k_voxel_mark<3>, dim3(tiles), dim3(kCompactThreads), 0, s, d_pts, n, v, (const uint32_t *)tab, mask, w, cnt);
  } else {
    hipLaunchKernelGGL(k_voxel_insert<2>, dim3(blocks), dim3(kVoxelThreads), 0, s, d_pts, n, v, tab, mask);
    hipLaunchKernelGGL(k_voxel_mark<2>, dim3(tiles), dim3(kCompactThreads), 0, s, d_pts, n, v, (const uint32_t *)tab, mask, w, cnt);
  }
  return hipGetLastError();
}

// the front half of a stand-alone call (voxel_device.hpp)
hipError_t launch_voxel_front(VoxelWs &W, int dim, const double *d_pts, size_t n, double v, hipStream_t s, size_t *mask,
                              uint32_t **sums) {
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  hipError_t e;
  if ((e = voxel_table(W, n, s, mask)) != hipSuccess) return e;
  if ((e = reserve(W.w, W.cap_w, n)) != hipSuccess) return e;
  if ((e = reserve(W.cnt, W.cap_cnt, (size_t)tiles + chunks)) != hipSuccess) return e;
  *sums = W.cnt + tiles;
  if ((e = launch_voxel_marks(dim, d_pts, n, v, W.tab, *mask, W.w, W.cnt, s)) != hipSuccess) return e;
  return launch_compact_chunks(W.cnt, tiles, *sums, s);
}

namespace {

// the stand-alone call on device buffers (g_mu held, the device current): everything on `s`, which is waited for
int voxel_downsample_on(VoxelWs &W, int dim, const double *d_pts, size_t n, double v, double *d_out,
                        uint32_t *d_kept_index, size_t *kept, hipStream_t s) {
  const unsigned tiles = compact_tiles(n), chunks = compact_chunks(tiles);
  size_t mask = 0;
  uint32_t *sums = nullptr;
  HIP_TRY(launch_voxel_front(W, dim, d_pts, n, v, s, &mask, &sums));
  if (d_out || d_kept_index) {
    if (dim == 3)
      hipLaunchKernelGGL(k_voxel_place<3>, dim3(tiles), dim3(kCompactThreads), 0, s, d_pts, n, (const uint32_t *)W.w,
                         (const uint32_t *)W.cnt, (const uint32_t *)sums, d_out, d_kept_index);
    else
      hipLaunchKernelGGL(k_voxel_place<2>, dim3(tiles), dim3(kCompactThreads), 0, s, d_pts, n, (const uint32_t *)W.w,
                         (const uint32_t *)W.cnt, (const uint32_t *)sums, d_out, d_kept_index);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(compact_total(sums, chunks, s, kept));
  return ICP_OK;
}

}  // namespace

bool voxel_args_ok(int dim, const void *pts, size_t n, double v, const size_t *kept) {
  return (dim == 2 || dim == 3) && kept && (n == 0 || pts) && voxel_size_ok(v) && n <= 0xfffffffeull;
}

int voxel_device(int *device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ICP_NO_DEVICE;
  if (*device < 0) HIP_TRY(hipGetDevice(device));
  if (*device >= count) return ICP_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(*device));
  return ICP_OK;
}

void api::voxel_trim() {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto &kv : g_ws) {
    VoxelWs &W = kv.second;
    for (void *p : {(void *)W.tab, (void *)W.w, (void *)W.cnt, (void *)W.idx, (void *)W.in, (void *)W.out, (void *)W.cov,
                    (void *)W.key, (void *)W.perm, (void *)W.start, (void *)W.ctr, (void *)W.count, (void *)W.of, (void *)W.items,
                    (void *)W.bigs, (void *)W.rec, W.sort_tmp})
      if (p) (void)hipFree(p);
    if (W.stream) (void)hipStreamDestroy(W.stream);
  }
  g_ws.clear();
}

}  // namespace icp

extern "C" int icp_voxel_downsample_device(int dim, const double *d_pts, size_t n, double voxel, double *d_out,
                                           uint32_t *d_kept_index, size_t *kept, int device, void *hip_stream) {
  if (!voxel_args_ok(dim, d_pts, n, voxel, kept) || device < -1) return ICP_BAD_ARGUMENT;
  *kept = 0;
  ICP_TRY_RC(voxel_device(&device));
  if (n == 0) return ICP_OK;
  std::lock_guard<std::mutex> lk(g_mu);
  return voxel_downsample_on(g_ws[device], dim, d_pts, n, voxel, d_out, d_kept_index, kept, (hipStream_t)hip_stream);
}

extern "C" int icp_voxel_downsample(int dim, const double *pts, size_t n, double voxel, double *out, uint32_t *kept_index,
                                    size_t *kept, int device) {
  if (!voxel_args_ok(dim, pts, n, voxel, kept) || device < -1) return ICP_BAD_ARGUMENT;
  *kept = 0;
  ICP_TRY_RC(voxel_device(&device));
  if (n == 0) return ICP_OK;
  std::lock_guard<std::mutex> lk(g_mu);
  VoxelWs &W = g_ws[device];
  if (!W.stream) HIP_TRY(hipStreamCreateWithFlags(&W.stream, hipStreamNonBlocking));
  HIP_TRY(reserve(W.in, W.cap_in, n * dim));
  if (out) HIP_TRY(reserve(W.out, W.cap_out, n * dim));
  if (kept_index) HIP_TRY(reserve(W.idx, W.cap_idx, n));
  HIP_TRY(hipMemcpyAsync(W.in, pts, n * dim * sizeof(double), hipMemcpyHostToDevice, W.stream));
  ICP_TRY_RC(voxel_downsample_on(W, dim, W.in, n, voxel, out ? W.out : nullptr, kept_index ? W.idx : nullptr, kept,
                                 W.stream));
  if (out && *kept)
    HIP_TRY(hipMemcpyAsync(out, W.out, *kept * dim * sizeof(double), hipMemcpyDeviceToHost, W.stream));
  if (kept_index && *kept)
    HIP_TRY(hipMemcpyAsync(kept_index, W.idx, *kept * sizeof(uint32_t), hipMemcpyDeviceToHost, W.stream));
  HIP_TRY(hipStreamSynchronize(W.stream));
  return ICP_OK;
}

extern "C" int icp_thin_targets(icp_handle *h, double voxel, uint32_t *new_index, size_t *removed) {
  if (!h || !voxel_size_ok(voxel)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (removed) *removed = 0;
  if (h->m == 0) return ICP_OK;
  uint32_t *w, *cnt;
  ICP_TRY_RC(target_marks(h, &w, &cnt));
  std::lock_guard<std::mutex> lk(g_mu);
  VoxelWs &W = g_ws[h->device];
  size_t mask = 0;
  HIP_TRY(voxel_table(W, h->m, h->stream, &mask));
  HIP_TRY(launch_voxel_marks(h->dim, h->d_dst, h->m, voxel, W.tab, mask, w, cnt, h->stream));
  return remove_marked_targets(h, w, cnt, h->grid.thins_moved, h->grid.thins_rebuilt, new_index, removed);
}

// Observability: out[0] = thins served by moving the grid's sorted records, out[1] = thins that rebuilt the grid
extern "C" int icp_grid_thin_counters(const icp_handle *h, uint64_t out[2]) {
  if (!h || !out) return ICP_BAD_ARGUMENT;
  out[0] = h->grid.thins_moved;
  out[1] = h->grid.thins_rebuilt;
  return ICP_OK;
}
