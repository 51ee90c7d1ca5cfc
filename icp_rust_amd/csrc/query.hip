// EXTENSION beyond the reference (include/icp_mi355x.h section 24): neighbour queries of ARBITRARY points against a
// handle's targets, and the removal of targets by the caller's own keep mask.  With outlier.hip's lists and filters
// this closes the loop "query, decide, remove" (DESIGN.md section 9v).
//   lists    k_query_neighbours<DIM, KMAX>  a lane per query point: the point is moved by the pose in the kernel (no
//            moved copy of the cloud goes through HBM), then grid_k_nearest (normal_single_device.hpp, unchanged: the
//            body of the normals kernels and of outlier.hip's lists) with the 3-D guards; a point far outside the
//            targets' box scans the targets directly instead.  Rows by (d^2, index), padded with (0xffffffff, +inf).
//            KMAX = 16 / 32: 12 / 24 KB of LDS per 64 lanes, as k_target_neighbours.
//   counts   k_count_within<DIM>  a lane per query point: the block walk of k_radius_mark for a point that need not lie
//            in the grid (the containment argument: DESIGN.md section 9v), leaving at `cap`.
//   order    from kQueryCellMinN queries on, lane j serves the j-th query in (cell, index) order -- the per-call sort
//            of icp_sort_source_device (prepare_queries, sort only) -- and writes row perm[j].  Results are per query:
//            the order changes no bit.  With q == nullptr the counts' queries are the targets, in record order.
//   removal  k_mask_marks  keep bytes -> mark words and cnt[tile] (compact_device.hpp: compact_mark_tile with the mask
//            as its rule), then the crop's back half (crop.hip: remove_marked_targets).
// Counts are integers, lists are exact selections: a result is a pure function of the input.
#include <cmath>
#include <map>
#include <mutex>

#include "api_internal.hpp"
#include "compact_device.hpp"
#include "normal_single_device.hpp"

using namespace icp;
using namespace icp::api;

namespace icp {
namespace {

constexpr uint32_t kNoNeighbour = 0xffffffffu;
constexpr int kListMax = 32;  // 1 <= k <= 32, as section 23
// Calls with at least this many query points are served in cell order: the smallest measured size at which the sorted
// arm beat the caller's order by more than the spread of both arms' samples (against 1M targets: it loses at 120k, wins
// from 250k on).  The handle's sort keeps the caller's order up to kGridCoopMaxN points, so
// nothing below that could be adopted.
constexpr size_t kQueryCellMinN = 250000;
static_assert(kQueryCellMinN > (size_t)kGridCoopMaxN, "prepare_queries does not sort up to kGridCoopMaxN points");

// Query point i of q under the pose: px = (r00 x + r01 y) + tx, py = (r10 x + r11 y) + ty, z kept -- products, add, then
// + t (Transform::transform as normal_gather forms it; the library is compiled without FMA contraction).  Without a
// pose the coordinates are used as given: NOT a product with the identity (0 * inf is NaN).
template <int DIM>
__device__ __forceinline__ void query_point(const double *__restrict__ q, size_t i, int posed, const Pose &T,
                                            double (&p)[DIM]) {
  for (int d = 0; d < DIM; ++d) p[d] = q[i * DIM + d];
  if (posed) {
    const double x = p[0], y = p[1];
    p[0] = (T.r00 * x + T.r01 * y) + T.tx;
    p[1] = (T.r10 * x + T.r11 * y) + T.ty;
  }
}

// The k nearest targets of p by (d^2, index) without the grid: every target in index order through the insertion of
// grid_k_nearest (the same comparisons, so the same lists).  O(m) for the lane.  1 <= k <= m.
template <int DIM>
__device__ __forceinline__ int direct_k_nearest(const double *__restrict__ dst, unsigned m, const double (&p)[DIM], int k,
                                                double *bd, uint32_t *bi) {
  int cnt = 0;
  for (uint32_t ti = 0; ti < m; ++ti) {
    const double dx = p[0] - dst[(size_t)ti * DIM], dy = p[1] - dst[(size_t)ti * DIM + 1];
    double dd = dx * dx + dy * dy;
    if (DIM == 3) {
      const double dz = p[DIM - 1] - dst[(size_t)ti * DIM + 2];
      dd = dd + dz * dz;
    }
    if (dd != dd) continue;  // a NaN distance is no neighbour
    if (cnt == k && !(dd < bd[k - 1] || (dd == bd[k - 1] && ti < bi[k - 1]))) continue;
    int pos = cnt < k ? cnt : k - 1;
    while (pos > 0 && (dd < bd[pos - 1] || (dd == bd[pos - 1] && ti < bi[pos - 1]))) {
      bd[pos] = bd[pos - 1];
      bi[pos] = bi[pos - 1];
      --pos;
    }
    bd[pos] = dd;
    bi[pos] = ti;
    if (cnt < k) ++cnt;
  }
  return cnt;
}

}  // namespace

// Row i of idx / d2 (either nullable, `stride` entries): the min(k, m) nearest targets of query i.  ks = min(k, m) <=
// KMAX is the list length asked of the search.  perm (nullable): lane j serves query perm[j].
//   a NaN coordinate: every d^2 is NaN, no target is a neighbour: padding only.
//   a point outside the targets' box by more than a quarter of its largest extent on some axis takes the direct scan:
//   the ring search would visit R = (that distance in cells) rings and scan its growing block again in each, R^4 against
//   the scan's n^3; both are exact, so the cut decides the time only.  An infinite coordinate
//   lies outside by +inf: every d^2 is +inf and the scan keeps the targets 0 .. ks-1, by the arithmetic alone.  (The
//   ring search must not be asked there: its cover test reads "no face left" as "the whole grid was visited", which an
//   infinite distance to a face would imitate.)
template <int DIM, int KMAX>
__global__ __launch_bounds__(64) void k_query_neighbours(const double *__restrict__ q, unsigned n, int posed, Pose T,
                                                         const uint32_t *__restrict__ perm,
                                                         const double *__restrict__ dst, unsigned m, GridParams g,
                                                         const uint32_t *__restrict__ start,
                                                         const GridPoint *__restrict__ pts, int ks, int stride,
                                                         uint32_t *__restrict__ idx, double *__restrict__ d2) {
  __shared__ double s_d[64][KMAX];
  __shared__ uint32_t s_i[64][KMAX];
  const unsigned j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  const unsigned i = perm ? perm[j] : j;
  if (i >= n) return;  // (a permutation's entry is always < n: this only keeps the accesses in bounds)
  double *bd = s_d[threadIdx.x];
  uint32_t *bi = s_i[threadIdx.x];
  double p[DIM];
  query_point<DIM>(q, i, posed, T, p);
  bool nan = false;
  double outside = 0.;
  for (int d = 0; d < DIM; ++d) {
    nan |= p[d] != p[d];
    outside = fmax(outside, fmax(g.lo[d] - p[d], p[d] - g.hi[d]));
  }
  int cnt = 0;
  if (nan) {
    cnt = 0;
  } else if (outside > 0.25 * (double)g.ext) {
    cnt = direct_k_nearest<DIM>(dst, m, p, ks, bd, bi);
  } else {
    cnt = grid_k_nearest<DIM, KMAX, true, false>(dst, m, g, start, pts, p, ks, bd, bi);
  }
  const size_t row = (size_t)i * stride;
  if (idx)
    for (int a = 0; a < stride; ++a) idx[row + a] = a < cnt ? bi[a] : kNoNeighbour;
  if (d2)
    for (int a = 0; a < stride; ++a) d2[row + a] = a < cnt ? bd[a] : __builtin_huge_val();
}

// counts[i] = min(cap, #{ j : d^2(p_i, t_j) <= r2 }).  q == nullptr: the queries are the targets, lane j serves the
// target of sorted record j (n == m).  The block of cells per axis: with the rounding slack
// e = 2^-48 (|p| + r + |lo| + |hi|) below half a cell, the cells of fl(p - r) and fl(p + r) under the grid's clamped,
// monotone cell map, widened by one cell (x by fx); otherwise -- a point or a radius far beyond the box, an infinity, a
// NaN -- the whole axis.  The walk leaves once `cap` is reached.
template <int DIM>
__global__ __launch_bounds__(256) void k_count_within(const double *__restrict__ q, unsigned n, int posed, Pose T,
                                                      const uint32_t *__restrict__ perm,
                                                      const double *__restrict__ dst, unsigned m, GridParams g,
                                                      const uint32_t *__restrict__ start,
                                                      const GridPoint *__restrict__ pts, double r, double r2,
                                                      unsigned cap, uint32_t *__restrict__ counts) {
  const unsigned j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  unsigned i;
  double p[DIM];
  if (q) {
    i = perm ? perm[j] : j;
    if (i >= n) return;  // (a permutation's entry is always < n)
    query_point<DIM>(q, i, posed, T, p);
  } else {
    i = pts[j].idx;
    if (i >= m) return;  // (a record's idx is always < m)
    for (int d = 0; d < DIM; ++d) p[d] = dst[(size_t)i * DIM + d];
  }
  int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
  for (int d = 0; d < DIM; ++d) {
    const int wd = d == 0 ? g.fx : 1;
    const double e = 0x1p-48 * (((fabs(p[d]) + r) + fabs(g.lo[d])) + fabs(g.hi[d]));
    if (e * g.inv_h[d] < 0.5) {  // (false for a NaN)
      const double top = (double)(g.n[d] - 1);
      const double a = fmin(fmax(floor(((p[d] - r) - g.lo[d]) * g.inv_h[d]), 0.), top);
      const double b = fmin(fmax(floor(((p[d] + r) - g.lo[d]) * g.inv_h[d]), 0.), top);
      c0[d] = max((int)a - wd, 0);
      c1[d] = min((int)b + wd, g.n[d] - 1);
    } else {
      c0[d] = 0;
      c1[d] = g.n[d] - 1;
    }
  }
  unsigned found = 0;
  for (int iz = c0[2]; iz <= c1[2] && found < cap; ++iz)
    for (int iy = c0[1]; iy <= c1[1] && found < cap; ++iy) {
      const uint32_t row = ((uint32_t)iz * g.n[1] + iy) * g.n[0];
      const uint32_t s = start[row + c0[0]], e = start[row + c1[0] + 1];
      for (uint32_t a = s; a < e && found < cap; ++a) {
        const uint32_t ti = pts[a].idx;
        if (ti >= m) continue;
        const double dx = p[0] - dst[(size_t)ti * DIM], dy = p[1] - dst[(size_t)ti * DIM + 1];
        double dd = dx * dx + dy * dy;
        if (DIM == 3) {
          const double dz = p[DIM - 1] - dst[(size_t)ti * DIM + 2];
          dd = dd + dz * dz;
        }
        found += dd <= r2 ? 1u : 0u;  // (false for a NaN d^2)
      }
    }
  counts[i] = found;
}

// The keep rule of icp_remove_targets: w[i] = keep[i] != 0 ? 0 : kCropGone, and cnt[tile] -- compact_mark_tile with
// the caller's mask as its rule, as k_crop_mark with the disc.
__global__ __launch_bounds__(kCompactThreads) void k_mask_marks(const uint8_t *__restrict__ keep, unsigned m,
                                                                uint32_t *__restrict__ w, uint32_t *__restrict__ cnt) {
  compact_mark_tile(m, cnt, [=](size_t i) {
    const bool in = keep[i] != 0;
    w[i] = in ? 0u : kCropGone;
    return in;
  });
}

namespace {

// What the host entries keep between calls, per device: the staged query points, rows, counts and mask.  One call at a
// time (g_mu is held for the length of a host call).
struct QueryWs {
  double *q = nullptr, *d2 = nullptr;
  uint32_t *idx = nullptr, *counts = nullptr;
  uint8_t *keep = nullptr;
  size_t cap_q = 0, cap_d2 = 0, cap_idx = 0, cap_counts = 0, cap_keep = 0;
};
std::mutex g_mu;
std::map<int, QueryWs> g_ws;

const Pose kIdentity = {1., 0., 0., 1., 0., 0.};

// The order the lanes of a call over the n points of d_q take: *perm = the handle's (cell, index) order of the points
// under the pose (prepare_queries, sort only: no sorted copy, no snapshot) from kQueryCellMinN points on, nullptr (the
// caller's order) below.  Like icp_sort_source_device, the call owns the handle's snapshot state and leaves none.
hipError_t query_order(icp_handle *h, const double *d_q, size_t n, const icp_pose *pose, const uint32_t **perm) {
  *perm = nullptr;
  Grid &G = h->grid;
  const int force = G.query_force;
  const bool cell = (long)n > kGridCoopMaxN && (force > 0 || (force == 0 && n >= kQueryCellMinN));
  if (!cell) {
    ++G.queries_caller;
    return hipSuccess;
  }
  QuerySort &Q = h->qsort;
  Q.sort_only = true;
  const hipError_t e = prepare_queries(h, d_q, n, pose ? *pose : kIdentity);
  Q.sort_only = false;
  Q.valid = false;  // (the sort belonged to this call)
  Q.have_prev = false;
  if (e != hipSuccess) return e;
  *perm = Q.d_perm;
  ++G.queries_cell;
  return hipSuccess;
}

// the state-dependent refusals of the query entries, after the argument-only ones
int query_state(const icp_handle *h) {
  if (h->m == 0) return ICP_EMPTY_DST;
  if (!h->grid.built) return ICP_BAD_ARGUMENT;
  return ICP_OK;
}

bool list_args_ok(const icp_handle *h, const void *q, size_t n, int k) {
  return h && k >= 1 && k <= kListMax && (n == 0 || q) && n < 0xffffffffull;
}

// (radius >= 0 is false for a NaN.)  q == nullptr: the targets themselves, which takes pose == nullptr -- and n == m, which
// only the handle's state can tell (count_state)
bool count_args_ok(const icp_handle *h, const void *q, const icp_pose *pose, size_t n, double radius, uint32_t cap,
                   const void *counts) {
  return h && radius >= 0. && cap >= 1 && n < 0xffffffffull && (n == 0 || counts) && (q || !pose);
}

int count_state(const icp_handle *h, const void *q, size_t n) {
  ICP_TRY_RC(query_state(h));
  return !q && n != h->m ? ICP_BAD_ARGUMENT : ICP_OK;
}

int neighbours_device(icp_handle *h, const double *d_q, size_t n_, const icp_pose *pose, int k, uint32_t *d_idx,
                      double *d_d2) {
  HIP_TRY(hipSetDevice(h->device));
  if (n_ == 0 || (!d_idx && !d_d2)) return ICP_OK;
  const uint32_t *perm = nullptr;
  HIP_TRY(query_order(h, d_q, n_, pose, &perm));
  const unsigned n = (unsigned)n_, m = (unsigned)h->m, blocks = (n + 63) / 64;
  const int ks = k < (int)m ? k : (int)m;  // (the rows keep k entries: the tail is padding)
  const int posed = pose ? 1 : 0;
  const Pose T = pose ? *pose : kIdentity;
  const Grid &G = h->grid;
#define ICP_LAUNCH_QUERY(DIM, KMAX)                                                                                  \
  hipLaunchKernelGGL((k_query_neighbours<DIM, KMAX>), dim3(blocks), dim3(64), 0, h->stream, d_q, n, posed, T, perm,   \
                     h->d_dst, m, G.p, (const uint32_t *)G.d_start, (const GridPoint *)G.d_pts, ks, k, d_idx, d_d2)
  if (h->dim == 3) {
    if (k <= 16) ICP_LAUNCH_QUERY(3, 16);
    else ICP_LAUNCH_QUERY(3, 32);
  } else {
    if (k <= 16) ICP_LAUNCH_QUERY(2, 16);
    else ICP_LAUNCH_QUERY(2, 32);
  }
#undef ICP_LAUNCH_QUERY
  HIP_TRY(hipGetLastError());
  return ICP_OK;
}

int count_device(icp_handle *h, const double *d_q, size_t n_, const icp_pose *pose, double radius, uint32_t cap,
                 uint32_t *d_counts) {
  HIP_TRY(hipSetDevice(h->device));
  if (n_ == 0) return ICP_OK;
  const uint32_t *perm = nullptr;
  if (d_q) HIP_TRY(query_order(h, d_q, n_, pose, &perm));
  else ++h->grid.queries_cell;  // (the targets, in the grid's record order)
  const unsigned n = (unsigned)n_, m = (unsigned)h->m, blocks = (n + 255) / 256;
  const int posed = pose ? 1 : 0;
  const Pose T = pose ? *pose : kIdentity;
  const double r2 = radius * radius;
  const Grid &G = h->grid;
  if (h->dim == 3)
    hipLaunchKernelGGL(k_count_within<3>, dim3(blocks), dim3(256), 0, h->stream, d_q, n, posed, T, perm, h->d_dst, m, G.p,
                       (const uint32_t *)G.d_start, (const GridPoint *)G.d_pts, radius, r2, (unsigned)cap, d_counts);
  else
    hipLaunchKernelGGL(k_count_within<2>, dim3(blocks), dim3(256), 0, h->stream, d_q, n, posed, T, perm, h->d_dst, m, G.p,
                       (const uint32_t *)G.d_start, (const GridPoint *)G.d_pts, radius, r2, (unsigned)cap, d_counts);
  HIP_TRY(hipGetLastError());
  return ICP_OK;
}

// the removal behind both entries: d_keep holds m bytes on the handle's device
int remove_by_mask(icp_handle *h, const uint8_t *d_keep, uint32_t *new_index, size_t *removed) {
  uint32_t *w, *cnt;
  ICP_TRY_RC(target_marks(h, &w, &cnt));
  const unsigned m = (unsigned)h->m, tiles = compact_tiles(m);
  hipLaunchKernelGGL(k_mask_marks, dim3(tiles), dim3(kCompactThreads), 0, h->stream, d_keep, m, w, cnt);
  HIP_TRY(hipGetLastError());
  return remove_marked_targets(h, w, cnt, h->grid.removes_moved, h->grid.removes_rebuilt, new_index, removed);
}

}  // namespace

void api::query_trim() {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto &kv : g_ws) {
    QueryWs &W = kv.second;
    for (void *p : {(void *)W.q, (void *)W.d2, (void *)W.idx, (void *)W.counts, (void *)W.keep})
      if (p) (void)hipFree(p);
  }
  g_ws.clear();
}

}  // namespace icp

extern "C" int icp_query_neighbours_device(icp_handle *h, const double *d_q, size_t n, const icp_pose *pose, int k,
                                           uint32_t *d_idx, double *d_d2) {
  if (!list_args_ok(h, d_q, n, k)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  ICP_TRY_RC(query_state(h));
  return neighbours_device(h, d_q, n, pose, k, d_idx, d_d2);
}

extern "C" int icp_query_neighbours(icp_handle *h, const double *q, size_t n, const icp_pose *pose, int k, uint32_t *idx,
                                    double *d2) {
  if (!list_args_ok(h, q, n, k)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  ICP_TRY_RC(query_state(h));
  if (n == 0 || (!idx && !d2)) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(g_mu);
  QueryWs &W = g_ws[h->device];
  const size_t cells = n * (size_t)k;
  HIP_TRY(reserve(W.q, W.cap_q, n * h->dim));
  if (idx) HIP_TRY(reserve(W.idx, W.cap_idx, cells));
  if (d2) HIP_TRY(reserve(W.d2, W.cap_d2, cells));
  HIP_TRY(hipMemcpyAsync(W.q, q, n * h->dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int rc = neighbours_device(h, W.q, n, pose, k, idx ? W.idx : nullptr, d2 ? W.d2 : nullptr);
  if (rc != ICP_OK) {
    (void)hipStreamSynchronize(h->stream);  // (the copy out of `q` may still be in flight)
    return rc;
  }
  if (idx) HIP_TRY(hipMemcpyAsync(idx, W.idx, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  if (d2) HIP_TRY(hipMemcpyAsync(d2, W.d2, cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ICP_OK;
}

extern "C" int icp_count_within_device(icp_handle *h, const double *d_q, size_t n, const icp_pose *pose, double radius,
                                       uint32_t cap, uint32_t *d_counts) {
  if (!count_args_ok(h, d_q, pose, n, radius, cap, d_counts)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  ICP_TRY_RC(count_state(h, d_q, n));
  return count_device(h, d_q, n, pose, radius, cap, d_counts);
}

extern "C" int icp_count_within(icp_handle *h, const double *q, size_t n, const icp_pose *pose, double radius,
                                uint32_t cap, uint32_t *counts) {
  if (!count_args_ok(h, q, pose, n, radius, cap, counts)) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  ICP_TRY_RC(count_state(h, q, n));
  if (n == 0) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(g_mu);
  QueryWs &W = g_ws[h->device];
  HIP_TRY(reserve(W.counts, W.cap_counts, n));
  if (q) {
    HIP_TRY(reserve(W.q, W.cap_q, n * h->dim));
    HIP_TRY(hipMemcpyAsync(W.q, q, n * h->dim * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  const int rc = count_device(h, q ? W.q : nullptr, n, pose, radius, cap, W.counts);
  if (rc != ICP_OK) {
    (void)hipStreamSynchronize(h->stream);  // (the copy out of `q` may still be in flight)
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(counts, W.counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return ICP_OK;
}

extern "C" int icp_remove_targets_device(icp_handle *h, const uint8_t *d_keep, uint32_t *new_index, size_t *removed) {
  if (!h || !d_keep) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (removed) *removed = 0;
  if (h->m == 0) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  return remove_by_mask(h, d_keep, new_index, removed);
}

extern "C" int icp_remove_targets(icp_handle *h, const uint8_t *keep, uint32_t *new_index, size_t *removed) {
  if (!h || !keep) return ICP_BAD_ARGUMENT;
  if (!have_device()) return ICP_NO_DEVICE;
  if (removed) *removed = 0;
  if (h->m == 0) return ICP_OK;
  HIP_TRY(hipSetDevice(h->device));
  std::lock_guard<std::mutex> lk(g_mu);
  QueryWs &W = g_ws[h->device];
  HIP_TRY(reserve(W.keep, W.cap_keep, h->m));
  // (pageable memory: the copy has left `keep` when the call returns, and it runs in front of the mark launch)
  HIP_TRY(hipMemcpyAsync(W.keep, keep, h->m, hipMemcpyHostToDevice, h->stream));
  return remove_by_mask(h, W.keep, new_index, removed);
}

// Observability: out[0] = removals by mask served by moving the grid's sorted records, out[1] = ... that rebuilt the grid
extern "C" int icp_grid_remove_counters(const icp_handle *h, uint64_t out[2]) {
  if (!h || !out) return ICP_BAD_ARGUMENT;
  out[0] = h->grid.removes_moved;
  out[1] = h->grid.removes_rebuilt;
  return ICP_OK;
}

// out[0] = query / count calls whose lanes ran in cell order (the per-call sort; the targets' record order for
// icp_count_within without points), out[1] = calls served in the caller's order
extern "C" int icp_query_counters(const icp_handle *h, uint64_t out[2]) {
  if (!h || !out) return ICP_BAD_ARGUMENT;
  out[0] = h->grid.queries_cell;
  out[1] = h->grid.queries_caller;
  return ICP_OK;
}

// For measurements: 0 = the library's threshold, 1 = cell order wherever the handle's sort orders at all (more than
// kGridCoopMaxN points), -1 = the caller's order
extern "C" int icp_query_force_order(icp_handle *h, int mode) {
  if (!h || mode < -1 || mode > 1) return ICP_BAD_ARGUMENT;
  h->grid.query_force = mode;
  return ICP_OK;
}
