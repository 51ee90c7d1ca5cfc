// C ABI, EXTENSION beyond the reference (include/icp_mi355x.h section 8): many small registrations in one call.
// The items that fit one workgroup run as k_tiny_estimate_batch (gn_fast.hip), one workgroup each, in at most three
// launches (one per workgroup size); the rest go one by one through a handle of the pool, exactly as a single call would
// serve them.  Every item's bits are those of icp_create + icp_estimate on its own ranges.
// Section 15, the same call with the point-to-line residual of section 14: k_line_estimate_batch (p2line_batch.hip), one
// workgroup per item in at most two launches; one by one: icp_create_device + icp_compute_target_line_normals +
// icp_estimate_point_to_line_device.
// Section 17, section 15 with a maximum correspondence distance: k_line_estimate_gated_batch, driven the same way; one by
// one: icp_estimate_point_to_line_gated_device in the last step's place.
// Sections 9 and 16, the quality of many poses: k_quality_batch (quality.hip) and, with the line residual,
// k_line_quality_batch (quality_line.hip), one workgroup per item in one launch; one by one: the single calls.
// Section 20, section 16's call with the point-to-plane residual for 3-D batches: k_plane_quality_batch
// (quality_plane_batch.hip), through the driver section 16 runs on.
// Section 18, section 8's call with the point-to-plane residual for 3-D batches: k_plane_estimate_batch
// (p2plane_batch.hip), one workgroup per item in at most two launches; one by one: icp_create_device +
// icp_compute_target_normals + icp_estimate_point_to_plane_device.
// Section 19, section 18 with a maximum correspondence distance: k_plane_estimate_gated_batch, driven the same way; one
// by one: icp_estimate_point_to_plane_gated_device in the last step's place.
// Section 21, section 8 with a maximum correspondence distance: k_tiny_estimate_gated_batch (gn_fast.hip), driven the
// same way; one by one: icp_create_device + icp_estimate_gated_device.
#include <cstring>
#include <new>
#include <vector>

#include "../../include/icp_mi355x_debug.h"
#include "api_internal.hpp"
#include "normal_batch_device.hpp"  // (the LDS plans the debug entries report)

using namespace icp;
using namespace icp::api;

struct icp_batch {
  int dim = 2, device = 0;
  hipStream_t stream = nullptr;
  // staged copies of the host entry's clouds, and the indices the host entry reads back
  double *d_src = nullptr, *d_dst = nullptr;
  size_t cap_src = 0, cap_dst = 0;
  uint32_t *d_idx = nullptr;
  size_t cap_idx = 0;
  // the launches' item lists: built in pinned memory, copied once per call
  TinyBatchItem *d_items = nullptr, *h_items = nullptr;
  size_t cap_items = 0, cap_h_items = 0;
  TinyResult *h_res = nullptr;  // pinned: the workgroups write their results here, one per item of the call
  size_t cap_res = 0;
  uint32_t *h_inner = nullptr;  // pinned: count x max_iter inner counts
  size_t cap_inner = 0;
  uint32_t *h_inl = nullptr;  // pinned: count x max_iter inlier counts (sections 17, 19 and 21)
  size_t cap_inl = 0;
  // what each family of entries has done, by CounterSet: {items a workgroup served, items served one by one, launches,
  // launches the runtime refused their LDS} (icp_batch_evaluate_counters: the first three)
  enum CounterSet {
    kPoint, kPointGated, kLine, kLineGated, kPlane, kPlaneGated, kQuality, kLineQuality, kPlaneQuality, kCounterSets
  };
  uint64_t ctr[kCounterSets][4] = {};
  // icp_batch_evaluate (section 9): its item list and the records its workgroups write (pinned)
  QualityBatchItem *d_qitems = nullptr, *h_qitems = nullptr;
  size_t cap_qitems = 0, cap_h_qitems = 0;
  QualityPart *h_qres = nullptr;
  size_t cap_qres = 0;
  // icp_batch_evaluate_point_to_line / _plane (sections 16 and 20): the item list above, and their own records (pinned)
  NormalQualityPart *h_nqres = nullptr;
  size_t cap_nqres = 0;
};

namespace {

template <typename Tp>
hipError_t reserve_pinned(Tp *&p, size_t &cap, size_t need) {
  if (need <= cap && p) return hipSuccess;
  if (p) {
    (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  const size_t want = need + need / 8 + 1;
  const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), want * sizeof(Tp), hipHostMallocDefault);
  if (e == hipSuccess) cap = want;
  return e;
}

bool in_range(uint64_t first, uint64_t count, size_t points) { return first <= points && count <= points - first; }

// every argument, before anything touches the device
int check_args(const icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
               const icp_batch_item *items, size_t count, size_t max_iter, const void *out, const int *status,
               bool per_iteration_words) {  // (inner_iters or inliers: count x max_iter words must be addressable)
  if (!b) return ICP_BAD_ARGUMENT;
  if (count == 0) return ICP_OK;
  if (!items || !out || !status || count > 0x7fffffffu) return ICP_BAD_ARGUMENT;  // (one workgroup per item)
  const size_t point_bytes = (size_t)b->dim * sizeof(double);
  if ((src_points > 0 && !src) || (dst_points > 0 && !dst) || src_points > SIZE_MAX / point_bytes ||
      dst_points > SIZE_MAX / point_bytes)
    return ICP_BAD_ARGUMENT;
  if (per_iteration_words && max_iter > 0 && count > SIZE_MAX / sizeof(uint32_t) / max_iter) return ICP_BAD_ARGUMENT;
  for (size_t i = 0; i < count; ++i) {
    const icp_batch_item &it = items[i];
    if (!in_range(it.src_first, it.n, src_points) || !in_range(it.dst_first, it.m, dst_points)) return ICP_BAD_ARGUMENT;
    if (it.n >= 0xffffffffull || it.m >= 0xffffffffull) return ICP_BAD_ARGUMENT;  // (as icp_create / icp_estimate)
  }
  return ICP_OK;
}

// An item the way single calls serve it: a handle of the pool on the item's targets, serve(h, the item's sources) on it.
// The outcomes in `per_item` land in *status; anything else (HIP, memory, device) is the call's failure.
template <size_t N, typename Serve>
int with_pool_handle(icp_batch *b, const double *d_src, const double *d_dst, const icp_batch_item &it,
                     const int (&per_item)[N], int *status, Serve serve) {
  icp_handle *h = nullptr;
  int rc = icp_create_device(&h, b->dim, it.m > 0 ? d_dst + it.dst_first * b->dim : nullptr, (size_t)it.m, b->device);
  if (rc == ICP_OK) {
    rc = serve(h, it.n > 0 ? d_src + it.src_first * b->dim : nullptr);
    icp_destroy(h);
  }
  for (const int s : per_item)
    if (rc == s) {
      *status = rc;
      return ICP_OK;
    }
  return rc;
}

// What the caller of an estimate entry supplies besides the clouds and the items: k, the neighbours of the normals (the
// point residual has none); for the gated entries max_dist and where the pairs kept per outer iteration go (count x
// max_iter, or null).
struct Residual {
  int k = 0;
  double max_dist = 0.;
  uint32_t *inliers = nullptr;
};

// ---- the six estimates behind run(): what they differ in is a Kind ----
//   kMaxN, kMaxM, kMaxIter  the items a workgroup serves
//   threads(n)              its size
//   launch(...)             one launch over the items of one size (inl: the pinned inlier counts, or null)
//   kCounters               the entry's counters
//   kPerItem, normals, estimate   one by one: the statuses that are the item's own, and the single calls on its handle --
//                           the first failing step gives the item's status (ICP_BAD_ARGUMENT: targets the plane normals
//                           refuse, as section 20's one-by-one server)
struct PointKind {  // section 8: k_tiny_estimate_batch (gn_fast.hip); icp_estimate_device
  static constexpr unsigned kMaxN = kTinyMaxN, kMaxM = kTinyMaxM, kMaxIter = kTinyMaxIter;
  static constexpr icp_batch::CounterSet kCounters = icp_batch::kPoint;
  static constexpr int kPerItem[4] = {ICP_OK, ICP_NONE, ICP_EMPTY_DST, ICP_NAN_INPUT};
  static unsigned threads(size_t n) { return tiny_threads(n); }
  static hipError_t launch(icp_batch *b, const Residual &, unsigned threads, unsigned m_max, const double *d_src,
                           const double *d_dst, const TinyBatchItem *d_items, unsigned count, unsigned max_iter,
                           uint32_t *inner, uint32_t *d_idx, uint32_t *, bool *granted) {
    return launch_tiny_estimate_batch(b->dim, threads, m_max, d_src, d_dst, d_items, count, max_iter, b->h_res, inner, d_idx,
                                      b->stream, granted);
  }
  static int normals(icp_handle *, int) { return ICP_OK; }
  static int estimate(icp_handle *h, const double *s, size_t n, const icp_pose *init, size_t max_iter, const Residual &,
                      icp_pose *out, uint32_t *d_idx, uint32_t *inner, uint32_t *) {
    return icp_estimate_device(h, s, n, init, max_iter, out, d_idx, inner);
  }
};

struct GatedPointKind {  // section 21: k_tiny_estimate_gated_batch (gn_fast.hip); icp_estimate_gated_device
  static constexpr unsigned kMaxN = kTinyMaxN, kMaxM = kTinyMaxM, kMaxIter = kTinyMaxIter;
  static constexpr icp_batch::CounterSet kCounters = icp_batch::kPointGated;
  static constexpr const int (&kPerItem)[4] = PointKind::kPerItem;
  static unsigned threads(size_t n) { return tiny_threads(n); }
  static hipError_t launch(icp_batch *b, const Residual &res, unsigned threads, unsigned m_max, const double *d_src,
                           const double *d_dst, const TinyBatchItem *d_items, unsigned count, unsigned max_iter,
                           uint32_t *inner, uint32_t *d_idx, uint32_t *inl, bool *granted) {
    // (max_dist * max_dist in f64 on the host, as icp_estimate_gated_device forms it)
    return launch_tiny_estimate_gated_batch(b->dim, threads, m_max, d_src, d_dst, d_items, count, max_iter,
                                            res.max_dist * res.max_dist, b->h_res, inner, d_idx, inl, b->stream, granted);
  }
  static int normals(icp_handle *, int) { return ICP_OK; }
  static int estimate(icp_handle *h, const double *s, size_t n, const icp_pose *init, size_t max_iter, const Residual &res,
                      icp_pose *out, uint32_t *d_idx, uint32_t *inner, uint32_t *inl) {
    return icp_estimate_gated_device(h, s, n, init, max_iter, res.max_dist, out, d_idx, inner, inl);
  }
};

// sections 15 and 17 (DIM 2: the line residual, p2line_batch.hip), 18 and 19 (DIM 3: the plane residual,
// p2plane_batch.hip); GATED: sections 17 and 19
template <int DIM, bool GATED>
struct NormalKind {
  static constexpr unsigned kMaxN = DIM == 2 ? kLineBatchMaxN : kPlaneBatchMaxN;
  static constexpr unsigned kMaxM = DIM == 2 ? kLineBatchMaxM : kPlaneBatchMaxM;
  static constexpr unsigned kMaxIter = DIM == 2 ? kLineBatchMaxIter : kPlaneBatchMaxIter;
  static constexpr icp_batch::CounterSet kCounters =
      DIM == 2 ? (GATED ? icp_batch::kLineGated : icp_batch::kLine) : (GATED ? icp_batch::kPlaneGated : icp_batch::kPlane);
  static constexpr int kPerItem[4] = {ICP_OK, DIM == 2 ? ICP_NONE : ICP_BAD_ARGUMENT, ICP_EMPTY_DST, ICP_NAN_INPUT};
  static unsigned threads(size_t n) { return normal_batch_threads(n); }
  static hipError_t launch(icp_batch *b, const Residual &res, unsigned threads, unsigned m_max, const double *d_src,
                           const double *d_dst, const TinyBatchItem *d_items, unsigned count, unsigned max_iter,
                           uint32_t *inner, uint32_t *d_idx, uint32_t *inl, bool *granted) {
    // (max_dist * max_dist in f64 on the host, as the single gated entries form it)
    return launch_normal_estimate_batch<DIM, GATED>(threads, m_max, d_src, d_dst, d_items, count, max_iter, res.k,
                                                    res.max_dist * res.max_dist, b->h_res, inner, d_idx, inl, b->stream,
                                                    granted);
  }
  static int normals(icp_handle *h, int k) {
    return DIM == 2 ? icp_compute_target_line_normals(h, k) : icp_compute_target_normals(h, k);
  }
  static int estimate(icp_handle *h, const double *s, size_t n, const icp_pose *init, size_t max_iter, const Residual &res,
                      icp_pose *out, uint32_t *d_idx, uint32_t *inner, uint32_t *inl) {
    if constexpr (GATED)
      return (DIM == 2 ? icp_estimate_point_to_line_gated_device
                       : icp_estimate_point_to_plane_gated_device)(h, s, n, init, max_iter, res.max_dist, out, d_idx, inner, inl);
    else
      return (DIM == 2 ? icp_estimate_point_to_line_device
                       : icp_estimate_point_to_plane_device)(h, s, n, init, max_iter, out, d_idx, inner);
  }
};

template <typename Kind>
bool fits(const icp_batch_item &it, size_t max_iter) {
  return it.n >= 1 && it.n <= Kind::kMaxN && it.m >= 1 && it.m <= Kind::kMaxM && max_iter >= 1 && max_iter <= Kind::kMaxIter;
}

template <typename Kind>
int run(icp_batch *b, const double *d_src, const double *d_dst, const icp_batch_item *items, size_t count,
        size_t max_iter, const Residual &res, icp_pose *out, int *status, uint32_t *d_idx, uint32_t *inner_iters) {
  uint32_t *inliers = res.inliers;
  uint64_t *ctr = b->ctr[Kind::kCounters];
  // where each item's indices go, and which items a workgroup may serve, by workgroup size
  std::vector<uint64_t> idx_first(count);
  std::vector<size_t> cls[3], one_by_one;
  uint64_t at = 0;
  for (size_t i = 0; i < count; ++i) {
    idx_first[i] = at;
    at += items[i].n;
    if (fits<Kind>(items[i], max_iter)) {
      const unsigned t = Kind::threads(items[i].n);
      cls[t == 512u ? 0 : (t == 768u ? 1 : 2)].push_back(i);
    } else {
      one_by_one.push_back(i);
    }
  }
  const size_t n_tiny = cls[0].size() + cls[1].size() + cls[2].size();
  std::vector<size_t> handed_back;
  if (n_tiny > 0) {
    HIP_TRY(reserve_pinned(b->h_items, b->cap_h_items, n_tiny));
    HIP_TRY(reserve(b->d_items, b->cap_items, n_tiny));
    HIP_TRY(reserve_pinned(b->h_res, b->cap_res, count));
    if (inner_iters) HIP_TRY(reserve_pinned(b->h_inner, b->cap_inner, count * max_iter));
    if (inliers) HIP_TRY(reserve_pinned(b->h_inl, b->cap_inl, count * max_iter));
    size_t k = 0;
    unsigned m_max[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c)
      for (size_t i : cls[c]) {
        TinyBatchItem &d = b->h_items[k++];
        d.src_first = items[i].src_first;
        d.dst_first = items[i].dst_first;
        d.idx_first = idx_first[i];
        d.n = (unsigned)items[i].n;
        d.m = (unsigned)items[i].m;
        d.slot = (unsigned)i;
        d.pad = 0;
        d.init = items[i].init;
        if (d.m > m_max[c]) m_max[c] = d.m;
        b->h_res[i].status = -1;
      }
    HIP_TRY(hipMemcpyAsync(b->d_items, b->h_items, n_tiny * sizeof(TinyBatchItem), hipMemcpyHostToDevice, b->stream));
    static const unsigned kThreads[3] = {512u, 768u, 1024u};
    size_t first = 0;
    bool granted = true;
    for (int c = 0; c < 3; ++c) {
      if (cls[c].empty()) continue;
      HIP_TRY(Kind::launch(b, res, kThreads[c], m_max[c], d_src, d_dst, b->d_items + first, (unsigned)cls[c].size(),
                           (unsigned)max_iter, inner_iters ? b->h_inner : nullptr, d_idx, inliers ? b->h_inl : nullptr,
                           &granted));
      ++ctr[granted ? 2 : 3];
      first += cls[c].size();
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (int c = 0; c < 3; ++c)
      for (size_t i : cls[c]) {
        const TinyResult &r = b->h_res[i];
        if (!granted || r.status == -1) {
          handed_back.push_back(i);
          continue;
        }
        ++ctr[0];
        if (r.status == 3) {
          status[i] = ICP_NAN_INPUT;
          continue;
        }
        status[i] = ICP_OK;
        out[i] = r.pose;
        if (inner_iters) std::memcpy(inner_iters + i * max_iter, b->h_inner + i * max_iter, max_iter * sizeof(uint32_t));
        if (inliers) std::memcpy(inliers + i * max_iter, b->h_inl + i * max_iter, max_iter * sizeof(uint32_t));
      }
  }
  one_by_one.insert(one_by_one.end(), handed_back.begin(), handed_back.end());
  for (size_t i : one_by_one) {
    ICP_TRY_RC(with_pool_handle(b, d_src, d_dst, items[i], Kind::kPerItem, &status[i], [&](icp_handle *h, const double *s) {
      ICP_TRY_RC(Kind::normals(h, res.k));
      return Kind::estimate(h, s, (size_t)items[i].n, &items[i].init, max_iter, res, &out[i],
                            d_idx ? d_idx + idx_first[i] : nullptr, inner_iters ? inner_iters + i * max_iter : nullptr,
                            inliers ? inliers + i * max_iter : nullptr);
    }));
    ++ctr[1];
  }
  return ICP_OK;
}

}  // namespace

// The device is not touched here: the first call that computes resolves it and creates the stream (so that a batch, and
// every argument check of its calls, exists without a GPU).
extern "C" int icp_batch_create(icp_batch **out, int dim, int device) {
  if (!out || (dim != 2 && dim != 3) || device < -1) return ICP_BAD_ARGUMENT;
  *out = nullptr;
  icp_batch *b = new (std::nothrow) icp_batch();
  if (!b) return ICP_OUT_OF_MEMORY;
  b->dim = dim;
  b->device = device;
  *out = b;
  return ICP_OK;
}

namespace {

int ensure_device(icp_batch *b) {
  if (b->stream) return hipSetDevice(b->device) == hipSuccess ? ICP_OK : ICP_HIP_ERROR;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ICP_NO_DEVICE;
  int device = b->device;
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= count) return ICP_BAD_ARGUMENT;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  b->device = device;
  return ICP_OK;
}

}  // namespace

extern "C" void icp_batch_destroy(icp_batch *b) {
  if (!b) return;
  if (b->stream) {
    (void)hipSetDevice(b->device);
    (void)hipStreamSynchronize(b->stream);
    (void)hipFree(b->d_src);
    (void)hipFree(b->d_dst);
    (void)hipFree(b->d_idx);
    (void)hipFree(b->d_items);
    if (b->h_items) (void)hipHostFree(b->h_items);
    if (b->h_res) (void)hipHostFree(b->h_res);
    if (b->h_inner) (void)hipHostFree(b->h_inner);
    if (b->h_inl) (void)hipHostFree(b->h_inl);
    (void)hipFree(b->d_qitems);
    if (b->h_qitems) (void)hipHostFree(b->h_qitems);
    if (b->h_qres) (void)hipHostFree(b->h_qres);
    if (b->h_nqres) (void)hipHostFree(b->h_nqres);
    (void)hipStreamDestroy(b->stream);
  }
  delete b;
}

namespace {

// what the entries with normals check on top of check_args: a batch of the residual's dimension, 3 <= k <= 16
bool normal_args_ok(const icp_batch *b, int dim, int k) { return b && b->dim == dim && k >= 3 && k <= 16; }

// one set of counters -> out[0 .. n)
int counters_out(const icp_batch *b, icp_batch::CounterSet set, uint64_t *out, int n = 4) {
  if (!b || !out) return ICP_BAD_ARGUMENT;
  for (int q = 0; q < n; ++q) out[q] = b->ctr[set][q];
  return ICP_OK;
}

// an LDS plan -> out[0 .. 4), where the debug entry's arguments are in range
template <typename Plan>
int plan_out(bool in_range, uint32_t *out, Plan plan) {
  if (!out || !in_range) return ICP_BAD_ARGUMENT;
  const NormalPlan p = plan();
  out[0] = p.list_threads;
  out[1] = p.shared_bytes;
  out[2] = p.fixed_bytes;
  out[3] = p.lds_bytes;
  return ICP_OK;
}
bool estimate_plan_args_ok(unsigned threads, unsigned m) {
  return (threads == 512u || threads == 1024u) && m >= 1 && m <= kPlaneBatchMaxM;
}

template <typename Kind>
int estimate_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst, size_t dst_points,
                    const icp_batch_item *items, size_t count, size_t max_iter, const Residual &res, icp_pose *out,
                    int *status, uint32_t *d_last_idx, uint32_t *inner_iters) {
  ICP_TRY_RC(check_args(b, d_src, src_points, d_dst, dst_points, items, count, max_iter, out, status,
                        inner_iters || res.inliers));
  if (count == 0) return ICP_OK;
  ICP_TRY_RC(ensure_device(b));
  return run<Kind>(b, d_src, d_dst, items, count, max_iter, res, out, status, d_last_idx, inner_iters);
}

// the host entries' clouds, staged through the batch's buffers: *d_src / *d_dst are what run, run_quality
// and run_normal_quality read (null for an empty array)
int stage_clouds(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                 const double **d_src, const double **d_dst) {
  if (src_points > 0) {
    HIP_TRY(reserve(b->d_src, b->cap_src, src_points * b->dim));
    HIP_TRY(hipMemcpyAsync(b->d_src, src, src_points * b->dim * sizeof(double), hipMemcpyHostToDevice, b->stream));
  }
  if (dst_points > 0) {
    HIP_TRY(reserve(b->d_dst, b->cap_dst, dst_points * b->dim));
    HIP_TRY(hipMemcpyAsync(b->d_dst, dst, dst_points * b->dim * sizeof(double), hipMemcpyHostToDevice, b->stream));
  }
  // (the items served one by one run on their handles' streams: the staged clouds must have landed first)
  HIP_TRY(hipStreamSynchronize(b->stream));
  *d_src = src_points > 0 ? b->d_src : nullptr;
  *d_dst = dst_points > 0 ? b->d_dst : nullptr;
  return ICP_OK;
}

// the entries that take host clouds: staged, the last indices read back
template <typename Kind>
int estimate_host(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                  const icp_batch_item *items, size_t count, size_t max_iter, const Residual &res, icp_pose *out,
                  int *status, uint32_t *last_idx, uint32_t *inner_iters) {
  ICP_TRY_RC(check_args(b, src, src_points, dst, dst_points, items, count, max_iter, out, status,
                        inner_iters || res.inliers));
  if (count == 0) return ICP_OK;
  ICP_TRY_RC(ensure_device(b));
  const double *d_src, *d_dst;
  ICP_TRY_RC(stage_clouds(b, src, src_points, dst, dst_points, &d_src, &d_dst));
  size_t total_n = 0;
  for (size_t i = 0; i < count; ++i) total_n += items[i].n;
  // (as icp_estimate: no outer iteration, no correspondences -- last_idx is left as it was)
  const bool want_idx = last_idx && total_n > 0 && max_iter > 0;
  if (want_idx) HIP_TRY(reserve(b->d_idx, b->cap_idx, total_n));
  const int rc = run<Kind>(b, d_src, d_dst, items, count, max_iter, res, out, status, want_idx ? b->d_idx : nullptr,
                           inner_iters);
  if (rc != ICP_OK) return rc;
  if (want_idx) {
    HIP_TRY(hipMemcpyAsync(last_idx, b->d_idx, total_n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  return ICP_OK;
}

}  // namespace

extern "C" int icp_batch_estimate_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                         size_t dst_points, const icp_batch_item *items, size_t count, size_t max_iter,
                                         icp_pose *out, int *status, uint32_t *d_last_idx, uint32_t *inner_iters) {
  return estimate_device<PointKind>(b, d_src, src_points, d_dst, dst_points, items, count, max_iter, Residual{}, out,
                                    status, d_last_idx, inner_iters);
}

extern "C" int icp_batch_estimate(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                                  const icp_batch_item *items, size_t count, size_t max_iter, icp_pose *out, int *status,
                                  uint32_t *last_idx, uint32_t *inner_iters) {
  return estimate_host<PointKind>(b, src, src_points, dst, dst_points, items, count, max_iter, Residual{}, out, status,
                                  last_idx, inner_iters);
}

// ---- section 21: section 8's entries with a maximum correspondence distance (max_dist >= 0, or +inf) ----
extern "C" int icp_batch_estimate_gated_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                               size_t dst_points, const icp_batch_item *items, size_t count,
                                               size_t max_iter, double max_dist, icp_pose *out, int *status,
                                               uint32_t *d_last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  if (!(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return estimate_device<GatedPointKind>(b, d_src, src_points, d_dst, dst_points, items, count, max_iter,
                                         Residual{0, max_dist, inliers}, out, status, d_last_idx, inner_iters);
}

extern "C" int icp_batch_estimate_gated(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                        size_t dst_points, const icp_batch_item *items, size_t count, size_t max_iter,
                                        double max_dist, icp_pose *out, int *status, uint32_t *last_idx,
                                        uint32_t *inner_iters, uint32_t *inliers) {
  if (!(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return estimate_host<GatedPointKind>(b, src, src_points, dst, dst_points, items, count, max_iter,
                                       Residual{0, max_dist, inliers}, out, status, last_idx, inner_iters);
}

// ---- section 15: the same two entries with the point-to-line residual (2-D batches, 3 <= k <= 16) ----
extern "C" int icp_batch_estimate_point_to_line_device(icp_batch *b, const double *d_src, size_t src_points,
                                                       const double *d_dst, size_t dst_points, const icp_batch_item *items,
                                                       size_t count, int k, size_t max_iter, icp_pose *out, int *status,
                                                       uint32_t *d_last_idx, uint32_t *inner_iters) {
  if (!normal_args_ok(b, 2, k)) return ICP_BAD_ARGUMENT;
  return estimate_device<NormalKind<2, false>>(b, d_src, src_points, d_dst, dst_points, items, count, max_iter,
                                               Residual{k}, out, status, d_last_idx, inner_iters);
}

extern "C" int icp_batch_estimate_point_to_line(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                                size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                                size_t max_iter, icp_pose *out, int *status, uint32_t *last_idx,
                                                uint32_t *inner_iters) {
  if (!normal_args_ok(b, 2, k)) return ICP_BAD_ARGUMENT;
  return estimate_host<NormalKind<2, false>>(b, src, src_points, dst, dst_points, items, count, max_iter, Residual{k}, out,
                                             status, last_idx, inner_iters);
}

// ---- section 17: section 15's entries with a maximum correspondence distance (max_dist >= 0, or +inf) ----
extern "C" int icp_batch_estimate_point_to_line_gated_device(icp_batch *b, const double *d_src, size_t src_points,
                                                             const double *d_dst, size_t dst_points,
                                                             const icp_batch_item *items, size_t count, int k,
                                                             size_t max_iter, double max_dist, icp_pose *out, int *status,
                                                             uint32_t *d_last_idx, uint32_t *inner_iters,
                                                             uint32_t *inliers) {
  if (!normal_args_ok(b, 2, k) || !(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return estimate_device<NormalKind<2, true>>(b, d_src, src_points, d_dst, dst_points, items, count, max_iter,
                                              Residual{k, max_dist, inliers}, out, status, d_last_idx, inner_iters);
}

extern "C" int icp_batch_estimate_point_to_line_gated(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                                      size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                                      size_t max_iter, double max_dist, icp_pose *out, int *status,
                                                      uint32_t *last_idx, uint32_t *inner_iters, uint32_t *inliers) {
  if (!normal_args_ok(b, 2, k) || !(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return estimate_host<NormalKind<2, true>>(b, src, src_points, dst, dst_points, items, count, max_iter,
                                            Residual{k, max_dist, inliers}, out, status, last_idx, inner_iters);
}

// ---- section 18: section 8's two entries with the point-to-plane residual (3-D batches, 3 <= k <= 16) ----
extern "C" int icp_batch_estimate_point_to_plane_device(icp_batch *b, const double *d_src, size_t src_points,
                                                        const double *d_dst, size_t dst_points, const icp_batch_item *items,
                                                        size_t count, int k, size_t max_iter, icp_pose *out, int *status,
                                                        uint32_t *d_last_idx, uint32_t *inner_iters) {
  if (!normal_args_ok(b, 3, k)) return ICP_BAD_ARGUMENT;
  return estimate_device<NormalKind<3, false>>(b, d_src, src_points, d_dst, dst_points, items, count, max_iter,
                                               Residual{k}, out, status, d_last_idx, inner_iters);
}

extern "C" int icp_batch_estimate_point_to_plane(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                                 size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                                 size_t max_iter, icp_pose *out, int *status, uint32_t *last_idx,
                                                 uint32_t *inner_iters) {
  if (!normal_args_ok(b, 3, k)) return ICP_BAD_ARGUMENT;
  return estimate_host<NormalKind<3, false>>(b, src, src_points, dst, dst_points, items, count, max_iter, Residual{k}, out,
                                             status, last_idx, inner_iters);
}

// ---- section 19: section 18's entries with a maximum correspondence distance (max_dist >= 0, or +inf) ----
extern "C" int icp_batch_estimate_point_to_plane_gated_device(icp_batch *b, const double *d_src, size_t src_points,
                                                              const double *d_dst, size_t dst_points,
                                                              const icp_batch_item *items, size_t count, int k,
                                                              size_t max_iter, double max_dist, icp_pose *out, int *status,
                                                              uint32_t *d_last_idx, uint32_t *inner_iters,
                                                              uint32_t *inliers) {
  if (!normal_args_ok(b, 3, k) || !(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return estimate_device<NormalKind<3, true>>(b, d_src, src_points, d_dst, dst_points, items, count, max_iter,
                                              Residual{k, max_dist, inliers}, out, status, d_last_idx, inner_iters);
}

extern "C" int icp_batch_estimate_point_to_plane_gated(icp_batch *b, const double *src, size_t src_points,
                                                       const double *dst, size_t dst_points, const icp_batch_item *items,
                                                       size_t count, int k, size_t max_iter, double max_dist, icp_pose *out,
                                                       int *status, uint32_t *last_idx, uint32_t *inner_iters,
                                                       uint32_t *inliers) {
  if (!normal_args_ok(b, 3, k) || !(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return estimate_host<NormalKind<3, true>>(b, src, src_points, dst, dst_points, items, count, max_iter,
                                            Residual{k, max_dist, inliers}, out, status, last_idx, inner_iters);
}

// ---- the estimates' counters and the LDS plans of the plane kernels' launches (include/icp_mi355x_debug.h) ----
extern "C" int icp_batch_counters(icp_batch *b, uint64_t out[4]) { return counters_out(b, icp_batch::kPoint, out); }
extern "C" int icp_batch_gated_counters(icp_batch *b, uint64_t out[4]) {
  return counters_out(b, icp_batch::kPointGated, out);
}
extern "C" int icp_batch_line_counters(icp_batch *b, uint64_t out[4]) { return counters_out(b, icp_batch::kLine, out); }
extern "C" int icp_batch_line_gated_counters(icp_batch *b, uint64_t out[4]) {
  return counters_out(b, icp_batch::kLineGated, out);
}
extern "C" int icp_batch_plane_counters(icp_batch *b, uint64_t out[4]) { return counters_out(b, icp_batch::kPlane, out); }
extern "C" int icp_batch_plane_gated_counters(icp_batch *b, uint64_t out[4]) {
  return counters_out(b, icp_batch::kPlaneGated, out);
}

extern "C" int icp_debug_plane_batch_plan(unsigned threads, unsigned m, uint32_t out[4]) {
  return plan_out(estimate_plan_args_ok(threads, m), out, [&] { return normal_estimate_plan<3, false>(threads, m); });
}

extern "C" int icp_debug_plane_gated_batch_plan(unsigned threads, unsigned m, uint32_t out[4]) {
  return plan_out(estimate_plan_args_ok(threads, m), out, [&] { return normal_estimate_plan<3, true>(threads, m); });
}

// ---- icp_batch_evaluate (include/icp_mi355x.h section 9): the quality of many poses in one launch ----
// The items that fit one workgroup run as k_quality_batch (quality.hip), one workgroup each, in one launch; the rest go
// one by one through a handle of the pool and icp_evaluate_device, exactly as a single call serves them.
namespace {

int check_quality_args(const icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                       const icp_batch_item *items, size_t count, double max_dist, const icp_quality *out,
                       const int *status) {
  if (!b || !(max_dist >= 0.)) return ICP_BAD_ARGUMENT;  // (NaN fails the comparison)
  return check_args(b, src, src_points, dst, dst_points, items, count, 0, out, status, false);
}

bool quality_fits(const icp_batch_item &it) {
  return it.n >= 1 && it.n <= kQualityMaxN && it.m >= 1 && it.m <= kQualityMaxM;
}

// What both evaluations do before their launch: the items that fit a workgroup (fits) -> fit, the others -> one_by_one;
// fit's QualityBatchItems (slot: the item's index in the call) copied to b->d_qitems; *m_max: their most targets.
int stage_quality_items(icp_batch *b, const icp_batch_item *items, size_t count, bool (*fits)(const icp_batch_item &),
                        std::vector<size_t> *fit, std::vector<size_t> *one_by_one, unsigned *m_max) {
  *m_max = 0;
  for (size_t i = 0; i < count; ++i) (fits(items[i]) ? fit : one_by_one)->push_back(i);
  if (fit->empty()) return ICP_OK;
  HIP_TRY(reserve_pinned(b->h_qitems, b->cap_h_qitems, fit->size()));
  HIP_TRY(reserve(b->d_qitems, b->cap_qitems, fit->size()));
  for (size_t k = 0; k < fit->size(); ++k) {
    const icp_batch_item &it = items[(*fit)[k]];
    QualityBatchItem &d = b->h_qitems[k];
    d.src_first = it.src_first;
    d.dst_first = it.dst_first;
    d.n = (unsigned)it.n;
    d.m = (unsigned)it.m;
    d.slot = (unsigned)(*fit)[k];
    d.pad = 0;
    d.T = it.init;
    if (d.m > *m_max) *m_max = d.m;
  }
  HIP_TRY(hipMemcpyAsync(b->d_qitems, b->h_qitems, fit->size() * sizeof(QualityBatchItem), hipMemcpyHostToDevice,
                         b->stream));
  return ICP_OK;
}

int run_quality(icp_batch *b, const double *d_src, const double *d_dst, const icp_batch_item *items, size_t count,
                double max_dist, icp_quality *out, int *status) {
  std::vector<size_t> fit, one_by_one;
  unsigned m_max;
  ICP_TRY_RC(stage_quality_items(b, items, count, quality_fits, &fit, &one_by_one, &m_max));
  if (!fit.empty()) {
    HIP_TRY(reserve_pinned(b->h_qres, b->cap_qres, count));
    // (r * r in f64 on the host, as icp_evaluate_device forms it)
    HIP_TRY(launch_quality_batch(b->dim, m_max, d_src, d_dst, b->d_qitems, (unsigned)fit.size(), max_dist * max_dist,
                                 b->h_qres, b->stream));
    ++b->ctr[icp_batch::kQuality][2];
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t i : fit) {
      status[i] = quality_result((size_t)items[i].n, b->h_qres[i], &out[i]);
      ++b->ctr[icp_batch::kQuality][0];
    }
  }
  for (size_t i : one_by_one) {
    ICP_TRY_RC(with_pool_handle(b, d_src, d_dst, items[i], {ICP_OK, ICP_EMPTY_DST, ICP_NAN_INPUT}, &status[i],
                                [&](icp_handle *h, const double *s) {
                                  return icp_evaluate_device(h, s, (size_t)items[i].n, &items[i].init, max_dist, &out[i],
                                                             nullptr);
                                }));
    ++b->ctr[icp_batch::kQuality][1];
  }
  return ICP_OK;
}

}  // namespace

extern "C" int icp_batch_evaluate_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst,
                                         size_t dst_points, const icp_batch_item *items, size_t count, double max_dist,
                                         icp_quality *out, int *status) {
  ICP_TRY_RC(check_quality_args(b, d_src, src_points, d_dst, dst_points, items, count, max_dist, out, status));
  if (count == 0) return ICP_OK;
  ICP_TRY_RC(ensure_device(b));
  return run_quality(b, d_src, d_dst, items, count, max_dist, out, status);
}

extern "C" int icp_batch_evaluate(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                  size_t dst_points, const icp_batch_item *items, size_t count, double max_dist,
                                  icp_quality *out, int *status) {
  ICP_TRY_RC(check_quality_args(b, src, src_points, dst, dst_points, items, count, max_dist, out, status));
  if (count == 0) return ICP_OK;
  ICP_TRY_RC(ensure_device(b));
  const double *d_src, *d_dst;
  ICP_TRY_RC(stage_clouds(b, src, src_points, dst, dst_points, &d_src, &d_dst));
  return run_quality(b, d_src, d_dst, items, count, max_dist, out, status);
}

extern "C" int icp_batch_evaluate_counters(icp_batch *b, uint64_t out[3]) {
  return counters_out(b, icp_batch::kQuality, out, 3);
}

// ---- icp_batch_evaluate_point_to_line (include/icp_mi355x.h section 16) and icp_batch_evaluate_point_to_plane
// (section 20): the same with the point-to-line residual of a 2-D batch, the point-to-plane residual of a 3-D batch ----
// The items that fit one workgroup run as k_line_quality_batch (quality_line.hip) / k_plane_quality_batch
// (quality_plane_batch.hip), one workgroup each, in one launch; the rest, and those a workgroup hands back, go one by
// one through a handle of the pool: icp_create_device + the residual's normals + its single evaluation, exactly as
// single calls serve them.  ONE driver and one pair of entries; what the two residuals differ in is a Kind below.
namespace {

struct LineQualityKind {
  using Q = icp_line_quality;
  static constexpr int kDim = 2;
  static bool fits(const icp_batch_item &it) {
    return it.n >= 1 && it.n <= kLineQualityMaxN && it.m >= 1 && it.m <= kLineQualityMaxM;
  }
  static constexpr auto launch = launch_normal_quality_batch<2>;
  static int result(size_t n, const NormalQualityPart &p, Q *q) { return line_quality_result(n, p, q); }
  static int normals(icp_handle *h, int k) { return icp_compute_target_line_normals(h, k); }
  static int evaluate(icp_handle *h, const double *s, size_t n, const icp_pose *T, double max_dist, Q *out) {
    return icp_evaluate_point_to_line_device(h, s, n, T, max_dist, out, nullptr);
  }
  static uint64_t *counters(icp_batch *b) { return b->ctr[icp_batch::kLineQuality]; }
};

struct PlaneQualityKind {
  using Q = icp_plane_quality;
  static constexpr int kDim = 3;
  static bool fits(const icp_batch_item &it) {  // (section 18's limits: what that serves in a launch, this does)
    return it.n >= 1 && it.n <= kPlaneQualityMaxN && it.m >= 1 && it.m <= kPlaneQualityMaxM;
  }
  static constexpr auto launch = launch_normal_quality_batch<3>;
  static int result(size_t n, const NormalQualityPart &p, Q *q) { return plane_quality_result(n, p, q); }
  static int normals(icp_handle *h, int k) { return icp_compute_target_normals(h, k); }
  static int evaluate(icp_handle *h, const double *s, size_t n, const icp_pose *T, double max_dist, Q *out) {
    return icp_evaluate_point_to_plane_device(h, s, n, T, max_dist, out, nullptr);
  }
  static uint64_t *counters(icp_batch *b) { return b->ctr[icp_batch::kPlaneQuality]; }
};

// One by one: the first failing step's status is the item's -- ICP_EMPTY_DST and ICP_BAD_ARGUMENT (targets the normals
// refuse) come from the normals, ICP_NAN_INPUT from the evaluation; *out then holds n and zeros.
template <typename Kind>
int serve_normal_quality_one(icp_batch *b, const double *d_src, const double *d_dst, const icp_batch_item &it, int k,
                             double max_dist, typename Kind::Q *out, int *status) {
  quality_clear((size_t)it.n, out);
  return with_pool_handle(b, d_src, d_dst, it, {ICP_OK, ICP_EMPTY_DST, ICP_NAN_INPUT, ICP_BAD_ARGUMENT}, status,
                          [&](icp_handle *h, const double *s) {
                            ICP_TRY_RC(Kind::normals(h, k));
                            return Kind::evaluate(h, s, (size_t)it.n, &it.init, max_dist, out);
                          });
}

template <typename Kind>
int run_normal_quality(icp_batch *b, const double *d_src, const double *d_dst, const icp_batch_item *items, size_t count,
                       int k, double max_dist, typename Kind::Q *out, int *status) {
  std::vector<size_t> fit, one_by_one;
  unsigned m_max;
  uint64_t *ctr = Kind::counters(b);
  ICP_TRY_RC(stage_quality_items(b, items, count, Kind::fits, &fit, &one_by_one, &m_max));
  if (!fit.empty()) {
    HIP_TRY(reserve_pinned(b->h_nqres, b->cap_nqres, count));
    for (size_t i : fit) b->h_nqres[i].pad = 1;  // handed back, unless its workgroup writes the record
    bool granted = true;
    // (r * r in f64 on the host, as the single evaluations form it)
    HIP_TRY(Kind::launch(m_max, d_src, d_dst, b->d_qitems, (unsigned)fit.size(), max_dist * max_dist, k, b->h_nqres,
                         b->stream, &granted));
    ++ctr[granted ? 2 : 3];
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (size_t i : fit) {
      if (!granted || b->h_nqres[i].pad != 0) {
        one_by_one.push_back(i);
        continue;
      }
      status[i] = Kind::result((size_t)items[i].n, b->h_nqres[i], &out[i]);
      ++ctr[0];
    }
  }
  for (size_t i : one_by_one) {
    ICP_TRY_RC(serve_normal_quality_one<Kind>(b, d_src, d_dst, items[i], k, max_dist, &out[i], &status[i]));
    ++ctr[1];
  }
  return ICP_OK;
}

// every argument, before anything touches the device
template <typename Kind>
int check_normal_quality_args(const icp_batch *b, const double *src, size_t src_points, const double *dst,
                              size_t dst_points, const icp_batch_item *items, size_t count, int k, double max_dist,
                              const typename Kind::Q *out, const int *status) {
  // (a NaN bound fails the comparison)
  if (!b || b->dim != Kind::kDim || k < 3 || k > 16 || !(max_dist >= 0.)) return ICP_BAD_ARGUMENT;
  return check_args(b, src, src_points, dst, dst_points, items, count, 0, out, status, false);
}

template <typename Kind>
int normal_quality_device(icp_batch *b, const double *d_src, size_t src_points, const double *d_dst, size_t dst_points,
                          const icp_batch_item *items, size_t count, int k, double max_dist, typename Kind::Q *out,
                          int *status) {
  ICP_TRY_RC(check_normal_quality_args<Kind>(b, d_src, src_points, d_dst, dst_points, items, count, k, max_dist, out,
                                             status));
  if (count == 0) return ICP_OK;
  ICP_TRY_RC(ensure_device(b));
  return run_normal_quality<Kind>(b, d_src, d_dst, items, count, k, max_dist, out, status);
}

template <typename Kind>
int normal_quality_host(icp_batch *b, const double *src, size_t src_points, const double *dst, size_t dst_points,
                        const icp_batch_item *items, size_t count, int k, double max_dist, typename Kind::Q *out,
                        int *status) {
  ICP_TRY_RC(check_normal_quality_args<Kind>(b, src, src_points, dst, dst_points, items, count, k, max_dist, out, status));
  if (count == 0) return ICP_OK;
  ICP_TRY_RC(ensure_device(b));
  const double *d_src, *d_dst;
  ICP_TRY_RC(stage_clouds(b, src, src_points, dst, dst_points, &d_src, &d_dst));
  return run_normal_quality<Kind>(b, d_src, d_dst, items, count, k, max_dist, out, status);
}

}  // namespace

extern "C" int icp_batch_evaluate_point_to_line_device(icp_batch *b, const double *d_src, size_t src_points,
                                                       const double *d_dst, size_t dst_points, const icp_batch_item *items,
                                                       size_t count, int k, double max_dist, icp_line_quality *out,
                                                       int *status) {
  return normal_quality_device<LineQualityKind>(b, d_src, src_points, d_dst, dst_points, items, count, k, max_dist, out,
                                                status);
}

extern "C" int icp_batch_evaluate_point_to_line(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                                size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                                double max_dist, icp_line_quality *out, int *status) {
  return normal_quality_host<LineQualityKind>(b, src, src_points, dst, dst_points, items, count, k, max_dist, out, status);
}

extern "C" int icp_batch_line_quality_counters(icp_batch *b, uint64_t out[4]) {
  return counters_out(b, icp_batch::kLineQuality, out);
}

// ---- section 20: the two entries with the point-to-plane residual (3-D batches, 3 <= k <= 16) ----
extern "C" int icp_batch_evaluate_point_to_plane_device(icp_batch *b, const double *d_src, size_t src_points,
                                                        const double *d_dst, size_t dst_points, const icp_batch_item *items,
                                                        size_t count, int k, double max_dist, icp_plane_quality *out,
                                                        int *status) {
  return normal_quality_device<PlaneQualityKind>(b, d_src, src_points, d_dst, dst_points, items, count, k, max_dist, out,
                                                 status);
}

extern "C" int icp_batch_evaluate_point_to_plane(icp_batch *b, const double *src, size_t src_points, const double *dst,
                                                 size_t dst_points, const icp_batch_item *items, size_t count, int k,
                                                 double max_dist, icp_plane_quality *out, int *status) {
  return normal_quality_host<PlaneQualityKind>(b, src, src_points, dst, dst_points, items, count, k, max_dist, out, status);
}

extern "C" int icp_batch_plane_quality_counters(icp_batch *b, uint64_t out[4]) {
  return counters_out(b, icp_batch::kPlaneQuality, out);
}

extern "C" int icp_debug_plane_quality_batch_plan(unsigned m, uint32_t out[4]) {
  return plan_out(m >= 1 && m <= kPlaneQualityMaxM, out, [&] { return normal_quality_plan<3>(m); });
}
