// EXTENSION beyond the reference (include/icp_mi355x.h section 23): the exact k-nearest-target lists of a handle and the two
// neighbourhood outlier filters built on them and on the grid.  The removal itself is the back half of the crop
// (crop.hip: target_marks / remove_marked_targets), as for icp_thin_targets.
//   the lists   k_target_neighbours<DIM, KMAX>  a lane per target: grid_k_nearest (normal_single_device.hpp, the body the
//               normals kernels run) with the 3-D guards in both dimensions; rows ordered by (d^2, index), self
//               included, padded with (0xffffffff, +inf).  KMAX = 16 serves k <= 16 with the LDS of the normals kernels
//               (12 KB per 64 lanes), KMAX = 32 the rest (24 KB).  A launch over ALL targets hands lane j the target of
//               the grid's j-th sorted record (neighbouring lanes, neighbouring cells); a sub-range goes by target index.
//               The same kernel in its `u` mode writes only the mean distance to the k nearest OTHER targets.
//   radius      k_radius_mark<DIM>  a lane per target in record order: counts the targets with d^2 <= r^2 in the block of
//               cells that holds them all and stops once min_neighbours is reached; w[i].
//   statistical u (above), two runs of the fold tree (fold_device.hpp: k_stat_level is its first level, k_fold_level the
//               others) for the mean and the deviation, k_stat_scalar between and behind them; the threshold stays on
//               the device.
//   shared      k_outlier_count  mark words (or u against the threshold) -> cnt[tile]: compact_device.hpp's
//               compact_mark_tile with either rule
// Counts are integers and every sum is a fixed tree or a left fold: a result is a pure function of the input.
#include <cmath>
#include <map>
#include <mutex>

#include "api_internal.hpp"
#include "compact_device.hpp"
#include "fold_device.hpp"
#include "normal_single_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace {

constexpr uint32_t kNoNeighbour = 0xffffffffu;
constexpr int kListMax = 32;  // the longest list: 1 <= k <= 32 (the statistical filter asks for k + 1)
using StatPart = FoldPart<1>;

}  // namespace

// idx / d2 (nullable): rows of `stride` entries for the targets [first, first + count); u (nullable): u[i - first] =
// (the left fold of sqrt(d^2) over the first k - 1 entries of the list that are not target i itself) / (k - 1).
// by_record: lane j serves the target of sorted record j (first == 0, count == m); otherwise target first + j.
// Needs 1 <= k <= min(KMAX, m).
template <int DIM, int KMAX>
__global__ __launch_bounds__(64) void k_target_neighbours(const double *__restrict__ dst, unsigned m, GridParams g,
                                                          const uint32_t *__restrict__ start,
                                                          const GridPoint *__restrict__ pts, int k, int stride,
                                                          unsigned first, unsigned count, int by_record,
                                                          uint32_t *__restrict__ idx, double *__restrict__ d2,
                                                          double *__restrict__ u) {
  __shared__ double s_d[64][KMAX];
  __shared__ uint32_t s_i[64][KMAX];
  const unsigned j = blockIdx.x * 64 + threadIdx.x;
  if (j >= count) return;
  unsigned i = first + j;
  if (by_record) {
    i = pts[j].idx;
    if (i >= m) return;  // (a record's idx is always < m: this only keeps the accesses in bounds)
  }
  double *bd = s_d[threadIdx.x];
  uint32_t *bi = s_i[threadIdx.x];
  double p[DIM];
  for (int d = 0; d < DIM; ++d) p[d] = dst[(size_t)i * DIM + d];
  const int cnt = grid_k_nearest<DIM, KMAX, true, false>(dst, m, g, start, pts, p, k, bd, bi);
  const size_t row = (size_t)(i - first) * stride;
  if (idx)
    for (int a = 0; a < stride; ++a) idx[row + a] = a < cnt ? bi[a] : kNoNeighbour;
  if (d2)
    for (int a = 0; a < stride; ++a) d2[row + a] = a < cnt ? bd[a] : __builtin_huge_val();
  if (u) {
    const int ke = k - 1;
    double s = 0.;
    int taken = 0;
    for (int a = 0; a < cnt && taken < ke; ++a) {
      if (bi[a] == i) continue;
      const double r = __dsqrt_rn(bd[a]);
      s = taken ? s + r : r;
      ++taken;
    }
    u[i - first] = s / (double)ke;
  }
}

// w[i] = 0 (kept) iff at least `need` targets j, i included, have d^2(i, j) <= r2.  The block of cells: those of
// fl(p - r) and fl(p + r) under the grid's clamped, monotone cell map, widened by one cell (x by fx) for the half ulp
// fl() may be off by, clamped.
template <int DIM>
__global__ __launch_bounds__(256) void k_radius_mark(const double *__restrict__ dst, unsigned m, GridParams g,
                                                     const uint32_t *__restrict__ start,
                                                     const GridPoint *__restrict__ pts, double r, double r2,
                                                     unsigned need, uint32_t *__restrict__ w) {
  const unsigned j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const unsigned i = pts[j].idx;
  if (i >= m) return;  // (a record's idx is always < m)
  double p[DIM];
  int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
  for (int d = 0; d < DIM; ++d) {
    p[d] = dst[(size_t)i * DIM + d];
    const int wd = d == 0 ? g.fx : 1;
    const double top = (double)(g.n[d] - 1);
    const double a = fmin(fmax(floor(((p[d] - r) - g.lo[d]) * g.inv_h[d]), 0.), top);
    const double b = fmin(fmax(floor(((p[d] + r) - g.lo[d]) * g.inv_h[d]), 0.), top);
    c0[d] = max((int)a - wd, 0);
    c1[d] = min((int)b + wd, g.n[d] - 1);
  }
  unsigned found = 0;
  for (int iz = c0[2]; iz <= c1[2] && found < need; ++iz)
    for (int iy = c0[1]; iy <= c1[1] && found < need; ++iy) {
      const uint32_t row = ((uint32_t)iz * g.n[1] + iy) * g.n[0];
      const uint32_t s = start[row + c0[0]], e = start[row + c1[0] + 1];
      for (uint32_t q = s; q < e && found < need; ++q) {
        const uint32_t ti = pts[q].idx;
        if (ti >= m) continue;
        const double dx = p[0] - dst[(size_t)ti * DIM], dy = p[1] - dst[(size_t)ti * DIM + 1];
        double dd = dx * dx + dy * dy;
        if (DIM == 3) {
          const double dz = p[DIM - 1] - dst[(size_t)ti * DIM + 2];
          dd = dd + dz * dz;
        }
        found += dd <= r2 ? 1u : 0u;
      }
    }
  w[i] = found >= need ? 0u : kCropGone;
}

// the first level of the tree over the per-target values: u itself (centre == nullptr) or (u - *centre)^2
__global__ __launch_bounds__(kFoldGroup) void k_stat_level(const double *__restrict__ u, unsigned m,
                                                           const double *__restrict__ centre,
                                                           StatPart *__restrict__ out) {
  __shared__ FoldLds<1> L;
  const unsigned tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * kFoldGroup + tid;
  if (i < m) {
    double v[1] = {u[i]};
    if (centre) {
      const double d = v[0] - *centre;
      v[0] = d * d;
    }
    fold_put(L, tid, v, 0ull, 0u);
  } else {
    fold_put_zero(L, tid);
  }
  fold_group(L, tid);
  if (tid == 0) out[blockIdx.x] = fold_take(L);
}

// scal = {mean, deviation, threshold}.  step 0: mean = root / m.  step 1: deviation = sqrt(root / (m - 1)), threshold =
// mean + ratio * deviation (two roundings: the library is compiled without FMA contraction).
__global__ void k_stat_scalar(const StatPart *__restrict__ root, unsigned m, int step, double ratio,
                              double *__restrict__ scal) {
  if (threadIdx.x || blockIdx.x) return;
  if (step == 0) {
    scal[0] = root->v[0] / (double)m;
  } else {
    const double dev = __dsqrt_rn(root->v[0] / (double)(m - 1));
    const double t = ratio * dev;
    scal[1] = dev;
    scal[2] = scal[0] + t;
  }
}

// cnt[tile] of the mark words; with u, the statistical rule writes them first: kept iff !(u[i] > *threshold)
__global__ __launch_bounds__(kCompactThreads) void k_outlier_count(uint32_t *__restrict__ w, unsigned m,
                                                                   const double *__restrict__ u,
                                                                   const double *__restrict__ threshold,
                                                                   uint32_t *__restrict__ cnt) {
  compact_mark_tile(m, cnt, [=](size_t i) {
    if (!u) return w[i] != kCropGone;  // (uniform: one mode per launch)
    const bool in = !(u[i] > *threshold);
    w[i] = in ? 0u : kCropGone;
    return in;
  });
}

namespace {

// What the calls keep between them, per device: u, the two buffers of the fold's levels, the three scalars, and the host
// entry's staging rows.  One call at a time (g_mu is held for the length of a call).
struct OutlierWs {
  double *u = nullptr, *scal = nullptr, *d2 = nullptr;
  StatPart *part_a = nullptr, *part_b = nullptr;
  uint32_t *idx = nullptr;
  size_t cap_u = 0, cap_scal = 0, cap_d2 = 0, cap_a = 0, cap_b = 0, cap_idx = 0;
};
std::mutex g_mu;
std::map<int, OutlierWs> g_ws;

// the list launch for targets [first, first + count) of a handle with a grid: 1 <= k <= min(32, m), rows of `stride`
hipError_t launch_neighbours(icp_handle *h, int k, int stride, size_t first, size_t count, uint32_t *d_idx, double *d_d2,
                             double *d_u) {
  const unsigned m = (unsigned)h->m, blocks = (unsigned)((count + 63) / 64);
  const int by_record = first == 0 && count == h->m;
  const Grid &G = h->grid;
#define ICP_LAUNCH_NEIGHBOURS(DIM, KMAX)                                                                               \
  hipLaunchKernelGGL((k_target_neighbours<DIM, KMAX>), dim3(blocks), dim3(64), 0, h->stream, h->d_dst, m, G.p,          \
                     (const uint32_t *)G.d_start, (const GridPoint *)G.d_pts, k, stride, (unsigned)first, (unsigned)count, \
                     by_record, d_idx, d_d2, d_u)
  if (h->dim == 3) {
    if (k <= 16) ICP_LAUNCH_NEIGHBOURS(3, 16);
    else ICP_LAUNCH_NEIGHBOURS(3, 32);
  } else {
    if (k <= 16) ICP_LAUNCH_NEIGHBOURS(2, 16);
    else ICP_LAUNCH_NEIGHBOURS(2, 32);
  }
#undef ICP_LAUNCH_NEIGHBOURS
  return hipGetLastError();
}

// the state-dependent refusals of the two list entries, after the argument-only ones
int neighbours_state(const icp_handle *h, size_t first, size_t count) {
  if (h->m == 0) return ICP_EMPTY_DST;
  if (first > h->m || count > h->m - first || !h->grid.built) return ICP_BAD_ARGUMENT;
  return ICP_OK;
}

int neighbours_device(icp_handle *h, int k, size_t first, size_t count, uint32_t *d_idx, double *d_d2) {
  HIP_TRY(hipSetDevice(h->device));
  if (count == 0 || (!d_idx && !d_d2)) return ICP_OK;
  const int ks = k < (int)h->m ? k : (int)h->m;  // (the rows keep k entries: the tail is padding)
  HIP_TRY(launch_neighbours(h, ks, k, first, count, d_idx, d_d2, nullptr));
  return ICP_OK;
}

// the whole statistical chain in front of the marks, on h->stream: u, the two trees, the scalars (W.scal)
int launch_statistics(icp_handle *h, OutlierWs &W, int k, double ratio) {
  const unsigned m = (unsigned)h->m, groups = (m + kFoldGroup - 1) / kFoldGroup;
  const int ke = k < (int)m - 1 ? k : (int)m - 1;
  HIP_TRY(reserve(W.u, W.cap_u, (size_t)m));
  HIP_TRY(reserve(W.scal, W.cap_scal, (size_t)3));
  HIP_TRY(reserve(W.part_a, W.cap_a, (size_t)groups));
  HIP_TRY(reserve(W.part_b, W.cap_b, (size_t)(groups + kFoldGroup - 1) / kFoldGroup));
  HIP_TRY(launch_neighbours(h, ke + 1, ke + 1, 0, m, nullptr, nullptr, W.u));
  for (int step = 0; step < 2; ++step) {
    hipLaunchKernelGGL(k_stat_level, dim3(groups), dim3(kFoldGroup), 0, h->stream, (const double *)W.u, m,
                       step ? (const double *)W.scal : (const double *)nullptr, W.part_a);
    HIP_TRY(hipGetLastError());
    StatPart *root = nullptr;
    HIP_TRY(fold_levels<1>(W.part_a, W.part_b, groups, h->stream, &root));
    hipLaunchKernelGGL(k_stat_scalar, dim3(1), dim3(1), 0, h->stream, (const StatPart *)root, m, step, ratio, W.scal);
    HIP_TRY(hipGetLastError());
  }
  return ICP_OK;
}

}  // namespace

void api::outlier_trim() {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto &kv : g_ws) {
    OutlierWs &W = kv.second;
    for (void *p : {(void *)W.u, (void *)W.scal, (void *)W.d2, (void *)W.part_a, (void *)W.part_b, (void *)W.idx})
      if (p) (void)hipFree(p);
  }
  g_ws.clear();
}

}  // namespace icp

extern "C" int icp_target_neighbours_device(icp_handle *h, int k, size_t first, size_t count, uint32_t *d_idx,
                                            double *d_d2) {
  if (!h || k < 1 || k > kListMax) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  ICP_TRY_RC(neighbours_state(h, first, count));
  return neighbours_device(h, k, first, count, d_idx, d_d2);
}

extern "C" int icp_target_neighbours(icp_handle *h, int k, size_t first, size_t count, uint32_t *idx, double *d2) {
  if (!h || k < 1 || k > kListMax) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  ICP_TRY_RC(neighbours_state(h, first, count));
  if (count == 0 || (!idx && !d2)) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(g_mu);
  OutlierWs &W = g_ws[h->device];
  const size_t cells = count * (size_t)k;
  if (idx) HIP_TRY(reserve(W.idx, W.cap_idx, cells));
  if (d2) HIP_TRY(reserve(W.d2, W.cap_d2, cells));
  ICP_TRY_RC(neighbours_device(h, k, first, count, idx ? W.idx : nullptr, d2 ? W.d2 : nullptr));
  if (idx) HIP_TRY(hipMemcpyAsync(idx, W.idx, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (d2) HIP_TRY(hipMemcpyAsync(d2, W.d2, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ICP_OK;
}

extern "C" int icp_remove_radius_outliers(icp_handle *h, double radius, size_t min_neighbours, uint32_t *new_index,
                                          size_t *removed) {
  if (!h || !(radius >= 0.)) return ICP_BAD_ARGUMENT;  // (false for a NaN)
  if (!have_device()) return ICP_NO_DEVICE;
  if (removed) *removed = 0;
  if (h->m == 0) return ICP_OK;
  if (!h->grid.built) return ICP_BAD_ARGUMENT;
  uint32_t *w, *cnt;
  ICP_TRY_RC(target_marks(h, &w, &cnt));
  const unsigned m = (unsigned)h->m, tiles = compact_tiles(m);
  const unsigned need = min_neighbours > (size_t)m ? m + 1u : (unsigned)min_neighbours;  // (m + 1: never reached)
  const double r2 = radius * radius;
  const Grid &G = h->grid;
  if (h->dim == 3)
    hipLaunchKernelGGL(k_radius_mark<3>, dim3((m + 255) / 256), dim3(256), 0, h->stream, h->d_dst, m, G.p,
                       (const uint32_t *)G.d_start, (const GridPoint *)G.d_pts, radius, r2, need, w);
  else
    hipLaunchKernelGGL(k_radius_mark<2>, dim3((m + 255) / 256), dim3(256), 0, h->stream, h->d_dst, m, G.p,
                       (const uint32_t *)G.d_start, (const GridPoint *)G.d_pts, radius, r2, need, w);
  hipLaunchKernelGGL(k_outlier_count, dim3(tiles), dim3(kCompactThreads), 0, h->stream, w, m, (const double *)nullptr,
                     (const double *)nullptr, cnt);
  HIP_TRY(hipGetLastError());
  return remove_marked_targets(h, w, cnt, h->grid.filters_moved, h->grid.filters_rebuilt, new_index, removed);
}

extern "C" int icp_remove_statistical_outliers(icp_handle *h, int k, double std_ratio, uint32_t *new_index,
                                               size_t *removed, double stats[3]) {
  if (!h || k < 1 || k > kListMax - 1 || !(std_ratio == std_ratio)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (removed) *removed = 0;
  if (stats) stats[0] = stats[1] = stats[2] = 0.;
  if (h->m <= 1) {  // no other target to be far from: nothing is removed
    if (new_index && h->m == 1) new_index[0] = 0;
    return ICP_OK;
  }
  if (!h->grid.built) return ICP_BAD_ARGUMENT;
  uint32_t *w, *cnt;
  ICP_TRY_RC(target_marks(h, &w, &cnt));
  const unsigned m = (unsigned)h->m, tiles = compact_tiles(m);
  std::lock_guard<std::mutex> lk(g_mu);
  OutlierWs &W = g_ws[h->device];
  ICP_TRY_RC(launch_statistics(h, W, k, std_ratio));
  hipLaunchKernelGGL(k_outlier_count, dim3(tiles), dim3(kCompactThreads), 0, h->stream, w, m, (const double *)W.u,
                     (const double *)(W.scal + 2), cnt);
  HIP_TRY(hipGetLastError());
  double host[3] = {0., 0., 0.};  // (arrives with remove_marked_targets' first wait)
  if (stats) HIP_TRY(hipMemcpyAsync(host, W.scal, sizeof(host), hipMemcpyDeviceToHost, h->stream));
  const int rc = remove_marked_targets(h, w, cnt, h->grid.filters_moved, h->grid.filters_rebuilt, new_index, removed);
  if (rc != ICP_OK) {
    (void)hipStreamSynchronize(h->stream);  // (the copy into `host` may still be in flight)
    return rc;
  }
  if (stats) stats[0] = host[0], stats[1] = host[1], stats[2] = host[2];
  return rc;
}

// Observability: out[0] = filters served by moving the grid's sorted records, out[1] = filters that rebuilt the grid
extern "C" int icp_grid_outlier_counters(const icp_handle *h, uint64_t out[2]) {
  if (!h || !out) return ICP_BAD_ARGUMENT;
  out[0] = h->grid.filters_moved;
  out[1] = h->grid.filters_rebuilt;
  return ICP_OK;
}
