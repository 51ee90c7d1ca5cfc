// What the one-workgroup batch kernels with a normal-based residual are made of, each piece once: the point-to-LINE
// kernels of 2-D items (p2line_batch.hip: k_line_estimate_batch, k_line_estimate_gated_batch; quality_line.hip:
// k_line_quality_batch) and the point-to-PLANE kernels of 3-D items (p2plane_batch.hip: k_plane_estimate_batch,
// k_plane_estimate_gated_batch; quality_plane_batch.hip: k_plane_quality_batch).  An item's bits are those of the single
// calls on a fresh handle, so the two residuals may not drift apart: they differ in NormalResidual<DIM> and
// NormalGate<DIM, B> below and nowhere else.
//   NormalResidual<DIM>              how a normal is stored, loaded and computed; a sorted target's NaN test
//   NormalGate<DIM, B>               the record a gated estimate keeps of a kept pair
//   normal_batch_plan<DIM>           the LDS plan of a launch, with its static assertions (DESIGN.md sections 9j - 9o)
//   normals_of_sorted_targets<DIM>   the normals of a workgroup's own targets, in rounds
//   normal_estimate_item<DIM, B, GATED>   one item of an estimate (the body of the four estimate kernels)
//   normal_quality_item<DIM>         one item of a pose quality (the body of the two quality kernels)
//   launch_one_workgroup_batch       the launch of either, behind its family's grant of LDS
#pragma once
#include "common.hpp"
#include "gn_device.hpp"
#include "p2line_device.hpp"
#include "p2plane_device.hpp"
#include "pair_loop_device.hpp"
#include "quality_device.hpp"
#include "tiny_device.hpp"

namespace icp {

// ---- what the two residuals differ in ----
// matched(tg, nrm, j, b, nn): the target at sorted position j and its normal.  pair(pr, tg, nrm, ax, ay, pz, j): the pair
// of k_line_gather / k_p2pl_gather from the moved point (ax, ay; pz: its own z) and that target; a line pair leaves dz =
// nz = +0.0 as the caller preset them.
// nan_target(tg, j, x, y): is a coordinate of the target just sorted to position j a NaN (x, y: its first two); the 2-D
// form never touches tg.tz, which is null there.
template <int DIM>
struct NormalResidual;

template <>
struct NormalResidual<2> {
  using Normal = double2;  // one per target, by sorted position
  static constexpr size_t kNormalBytes = sizeof(double2);
  static constexpr size_t kGateRecordBytes = 2 * sizeof(double) + sizeof(uint32_t);  // NormalGate<2, B>
  static __device__ __forceinline__ bool nan_target(const TinyTargets &, unsigned, double x, double y) {
    return (x != x) | (y != y);
  }
  static __device__ __forceinline__ void matched(const TinyTargets &tg, const Normal *nrm, unsigned j, double (&b)[2],
                                                 double (&nn)[2]) {
    const double2 nq = nrm[j];
    b[0] = tg.tx[j];
    b[1] = tg.ty[j];
    nn[0] = nq.x;
    nn[1] = nq.y;
  }
  static __device__ __forceinline__ void pair(PlanePair &pr, const TinyTargets &tg, const Normal *nrm, double ax, double ay,
                                              double, unsigned j) {
    const double2 nq = nrm[j];
    pr.ax = ax;
    pr.ay = ay;
    pr.qx = tg.tx[j];
    pr.qy = tg.ty[j];
    pr.nx = nq.x;
    pr.ny = nq.y;
  }
  static __device__ __forceinline__ double coordinate(const TinyTargets &tg, unsigned j, int d) {
    return d == 0 ? tg.tx[j] : tg.ty[j];
  }
  // line_normal_of_neighbours (p2line_device.hpp), the statement k_line_normals evaluates -> nrm[j]
  template <class Coord>
  static __device__ __forceinline__ void normal_of_neighbours(int cnt, Coord coord, Normal *nrm, unsigned j) {
    double nv[2];
    line_normal_of_neighbours(cnt, coord, nv);
    nrm[j] = make_double2(nv[0], nv[1]);
  }
};

template <>
struct NormalResidual<3> {
  using Normal = double;  // three per target, at [3 x sorted position]
  static constexpr size_t kNormalBytes = 3 * sizeof(double);
  static constexpr size_t kGateRecordBytes = sizeof(uint32_t);  // NormalGate<3, B>
  static __device__ __forceinline__ bool nan_target(const TinyTargets &tg, unsigned j, double x, double y) {
    const double z = tg.tz[j];  // (this thread has just written it)
    return (x != x) | (y != y) | (z != z);
  }
  static __device__ __forceinline__ void matched(const TinyTargets &tg, const Normal *nrm, unsigned j, double (&b)[3],
                                                 double (&nn)[3]) {
    b[0] = tg.tx[j];
    b[1] = tg.ty[j];
    b[2] = tg.tz[j];
    nn[0] = nrm[3 * j];
    nn[1] = nrm[3 * j + 1];
    nn[2] = nrm[3 * j + 2];
  }
  static __device__ __forceinline__ void pair(PlanePair &pr, const TinyTargets &tg, const Normal *nrm, double ax, double ay,
                                              double pz, unsigned j) {
    pr.ax = ax;
    pr.ay = ay;
    pr.qx = tg.tx[j];
    pr.qy = tg.ty[j];
    pr.dz = pz - tg.tz[j];
    pr.nx = nrm[3 * j];
    pr.ny = nrm[3 * j + 1];
    pr.nz = nrm[3 * j + 2];
  }
  static __device__ __forceinline__ double coordinate(const TinyTargets &tg, unsigned j, int d) {
    return d == 0 ? tg.tx[j] : (d == 1 ? tg.ty[j] : tg.tz[j]);
  }
  // plane_normal_of_neighbours (p2plane_device.hpp), the statement k_target_normals evaluates -> nrm[3 j]
  template <class Coord>
  static __device__ __forceinline__ void normal_of_neighbours(int cnt, Coord coord, Normal *nrm, unsigned j) {
    double nv[3];
    plane_normal_of_neighbours(cnt, coord, nv);
    nrm[3 * j] = nv[0];
    nrm[3 * j + 1] = nv[1];
    nrm[3 * j + 2] = nv[2];
  }
};

// ---- the gate's record (sections 17 and 19; DESIGN.md sections 9l and 9n) ----
// Behind the estimator's three sort buffers in the shared region (p), which the normals' lists have left by then: a
// record per kept pair, in pair order, and the 16 wave counts (cnt).  put(rank, tid, qx, qy, nb): source thread tid's
// moved point and the sorted position of its match are pair `rank`; pair(t, ...) forms pair t from its record.
template <int DIM, unsigned B>
struct NormalGate;

// two dimensions: the moved point (x | y, f64) and the position
template <unsigned B>
struct NormalGate<2, B> {
  double *qx, *qy;
  uint32_t *nb, *cnt;
  __device__ __forceinline__ explicit NormalGate(unsigned char *p)
      : qx(reinterpret_cast<double *>(p)), qy(qx + B), nb(reinterpret_cast<uint32_t *>(qy + B)), cnt(nb + B) {}
  __device__ __forceinline__ void put(unsigned rank, unsigned, double x, double y, unsigned pos) const {
    qx[rank] = x;
    qy[rank] = y;
    nb[rank] = pos;
  }
  __device__ __forceinline__ void pair(unsigned t, PlanePair &pr, const TinyTargets &tg, const double2 *nrm,
                                       const double *, const PairCtl *) const {
    NormalResidual<2>::pair(pr, tg, nrm, qx[t], qy[t], 0., nb[t]);
  }
};

// three dimensions: ONE word, (source thread << 16) | sorted position, both below 2^16.  The moved point is not kept:
// thread t reads the source row of pair t again and forms qx, qy with the expression and the pose the gate formed them
// with (C->T: thread 0 writes it next in tiny_outer_tail, behind the inner loop) -- the same expressions, the same bits;
// the eight values k_plgate_stage writes.  The two-dimensional record with z does not fit behind the sort buffers beyond
// 1664 targets (the assertions below).
template <unsigned B>
struct NormalGate<3, B> {
  uint32_t *w, *cnt;
  __device__ __forceinline__ explicit NormalGate(unsigned char *p) : w(reinterpret_cast<uint32_t *>(p)), cnt(w + B) {}
  __device__ __forceinline__ void put(unsigned rank, unsigned tid, double, double, unsigned pos) const {
    w[rank] = (tid << 16) | pos;  // (rank < kept <= n <= B; tid < 1024 and pos < m <= 2048: 16 bits each)
  }
  __device__ __forceinline__ void pair(unsigned t, PlanePair &pr, const TinyTargets &tg, const double *nrm,
                                       const double *src, const PairCtl *C) const {
    const unsigned v = w[t], s = v >> 16, g = v & 0xffffu;  // (s < n, g < m: written by put)
    const double sx = src[(size_t)s * 3], sy = src[(size_t)s * 3 + 1], sz = src[(size_t)s * 3 + 2];
    const Pose G = C->T;
    NormalResidual<3>::pair(pr, tg, nrm, (G.r00 * sx + G.r01 * sy) + G.tx, (G.r10 * sx + G.r11 * sy) + G.ty, sz, g);
  }
};
static_assert(kLineBatchMaxN <= 0x10000u && kPlaneBatchMaxN <= 0x10000u && kPlaneBatchMaxM <= 0x10000u,
              "a source thread and a sorted position in 16 bits each");

// ---- the LDS plan of a launch (DESIGN.md sections 9j, 9k, 9m, 9o; 9l and 9n for the gate) ----
// per workgroup, for its item's m targets (mp = m rounded up to 64): x | y (| z) in f64, the f32 screen records (+ 4
// pads), the normals by sorted position; then ONE shared region, sized by the launch; then the tail: an estimate's wave
// sums, totals and PairCtl, or a quality's control words.  The shared region holds, one after the other: the target
// sort's keys (8 B x the next power of two of m), the k-best lists of the normals ((8 + 4) B x 16 per list-holding
// thread), and what runs behind the normals (behind_bytes): the estimator's two sort buffers and sorted keys (3 x 8 B x
// threads) with the gate's records behind them, or the fold's group with the four group records.  Per-thread lists for
// every thread do not fit beside 2048 targets, so the normals run in rounds of `list_threads` targets: as many as the
// grant leaves room for, up to one per thread and per target.
constexpr size_t kNormalListBytes = kTinyKBestMax * (sizeof(double) + sizeof(uint32_t));
static_assert(kNormalListBytes == 192, "sixteen (d^2, index | position) entries");
static_assert(kLineBatchMaxM <= kTinyKBestMaxTargets && kPlaneBatchMaxM <= kTinyKBestMaxTargets &&
                  kLineQualityMaxM <= kTinyKBestMaxTargets && kPlaneQualityMaxM <= kTinyKBestMaxTargets,
              "(original index << 16) | sorted position: both below 2^16");
constexpr size_t normal_keys_bytes(unsigned m) {
  size_t keys = 64;
  while (keys < m) keys <<= 1;
  return keys * 8;
}
template <int DIM>
constexpr NormalPlan normal_batch_plan(unsigned threads, unsigned m_max, size_t behind_bytes, size_t tail_bytes) {
  const size_t mp = (m_max + 63u) & ~63u;
  const size_t fixed =
      mp * DIM * sizeof(double) + (mp + 4) * sizeof(float4) + mp * NormalResidual<DIM>::kNormalBytes + tail_bytes;
  const size_t keys = normal_keys_bytes(m_max);
  const size_t fit = (kTinyLdsGrant - fixed) / kNormalListBytes / 64 * 64;
  size_t lists = mp;  // (a list per target is all a round can use)
  lists = lists < threads ? lists : threads;
  lists = lists < fit ? lists : fit;
  size_t shared = lists * kNormalListBytes;
  shared = shared > keys ? shared : keys;
  shared = shared > behind_bytes ? shared : behind_bytes;
  return NormalPlan{(unsigned)lists, (unsigned)shared, (unsigned)fixed, (unsigned)(fixed + shared)};
}

// an estimate's: the sort buffers (and the gate's records) behind the lists; the wave sums, the totals and PairCtl
constexpr size_t kNormalEstimateTailBytes = sizeof(double) * 16 * kPairSums + sizeof(double) * 16 + 256;
static_assert(sizeof(PairCtl) <= 256, "PairCtl's share of the LDS");
template <int DIM>
constexpr size_t normal_gate_bytes(unsigned threads) {
  return (size_t)threads * NormalResidual<DIM>::kGateRecordBytes + 16 * sizeof(uint32_t);
}
template <int DIM, bool GATED>
constexpr NormalPlan normal_estimate_plan(unsigned threads, unsigned m_max) {
  return normal_batch_plan<DIM>(threads, m_max, (size_t)3 * threads * 8 + (GATED ? normal_gate_bytes<DIM>(threads) : 0),
                                kNormalEstimateTailBytes);
}
// a quality's: a thread per source point; the fold aliases the lists, which are dead by then; the control words
constexpr unsigned kNormalQualityThreads = 1024;
constexpr size_t kNormalQualityFoldBytes =
    sizeof(FoldLds<kNormalQualitySums>) + (kNormalQualityThreads / kFoldGroup) * sizeof(NormalQualityPart);
constexpr size_t kNormalQualityCtlBytes = 256;
struct NormalQualityCtl {
  unsigned pos0;  // the sorted position of the target of original index 0
  int bail;       // a NaN target: the single call decides what such a cloud is
};
static_assert(sizeof(NormalQualityCtl) <= kNormalQualityCtlBytes, "the control words' share of the LDS");
static_assert(kNormalQualityFoldBytes == 23936 && kNormalQualityFoldBytes % 16 == 0, "a group of the tree and four records");
static_assert(kLineQualityMaxN == kNormalQualityThreads && kPlaneQualityMaxN == kNormalQualityThreads,
              "a thread per source point");
static_assert(kPlaneQualityMaxN >= kPlaneBatchMaxN && kPlaneQualityMaxM >= kPlaneBatchMaxM,
              "every item the estimate serves in a launch is served in a launch here");
template <int DIM>
constexpr NormalPlan normal_quality_plan(unsigned m_max) {
  return normal_batch_plan<DIM>(kNormalQualityThreads, m_max, kNormalQualityFoldBytes, kNormalQualityCtlBytes);
}

// -- the line estimate's plan at its corners: the smallest item, a golden scan (two rounds of 640), the largest item
// (rounds of 320); gated: the gate's records lie where the lists were, nothing on top of the ungated plan at m = 2048
static_assert(normal_estimate_plan<2, false>(1024, kLineBatchMaxM).fixed_bytes + 3 * 1024 * 8 <= kTinyLdsGrant &&
                  (kTinyLdsGrant - normal_estimate_plan<2, false>(1024, kLineBatchMaxM).fixed_bytes) / kNormalListBytes >= 256,
              "2048 targets leave room for the sort buffers and for at least 256 lists");
static_assert(normal_estimate_plan<2, false>(512, 1).list_threads == 64 &&
                  normal_estimate_plan<2, false>(512, 1).shared_bytes == 3 * 512 * 8,
              "m = 1");
static_assert(normal_estimate_plan<2, false>(1024, 668).list_threads == 640 &&
                  normal_estimate_plan<2, false>(1024, 668).lds_bytes == 158784,
              "m = 668");
static_assert(normal_estimate_plan<2, false>(512, kLineBatchMaxM).list_threads == 320 &&
                  normal_estimate_plan<2, false>(1024, kLineBatchMaxM).list_threads == 320 &&
                  normal_estimate_plan<2, false>(1024, kLineBatchMaxM).lds_bytes == 161856 &&
                  normal_estimate_plan<2, false>(1024, kLineBatchMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048");
static_assert(normal_estimate_plan<2, true>(512, 1).list_threads == 64 &&
                  normal_estimate_plan<2, true>(512, 1).shared_bytes == 3 * 512 * 8 + normal_gate_bytes<2>(512) &&
                  normal_estimate_plan<2, true>(1024, 1).shared_bytes == 3 * 1024 * 8 + normal_gate_bytes<2>(1024),
              "m = 1: the sort buffers and the gate's words");
static_assert(normal_estimate_plan<2, true>(1024, 668).list_threads == 640 &&
                  normal_estimate_plan<2, true>(1024, 668).lds_bytes == 158784,
              "m = 668: the gate's words lie where the lists were");
static_assert(normal_estimate_plan<2, true>(512, kLineBatchMaxM).list_threads == 320 &&
                  normal_estimate_plan<2, true>(1024, kLineBatchMaxM).list_threads == 320 &&
                  normal_estimate_plan<2, true>(512, kLineBatchMaxM).lds_bytes == 161856 &&
                  normal_estimate_plan<2, true>(1024, kLineBatchMaxM).lds_bytes == 161856 &&
                  normal_estimate_plan<2, true>(1024, kLineBatchMaxM).fixed_bytes + 3 * 1024 * 8 + normal_gate_bytes<2>(1024) <=
                      kTinyLdsGrant,
              "m = 2048: nothing on top of the ungated plan");

// -- the plane estimate's: the smallest item, 1024 targets (three rounds of 448), the largest item (sixteen rounds of
// 128, with most of the workgroup idle)
static_assert(1024 / 64 * 6 * sizeof(double) <= normal_estimate_plan<3, false>(512, 1).fixed_bytes, "the box's wave minima");
static_assert(normal_estimate_plan<3, false>(512, 1).list_threads == 64 &&
                  normal_estimate_plan<3, false>(512, 1).shared_bytes == 3 * 512 * 8 &&
                  normal_estimate_plan<3, false>(1024, 1).shared_bytes == 3 * 1024 * 8 &&
                  normal_estimate_plan<3, false>(512, 1).fixed_bytes == 6208,
              "m = 1");
static_assert(normal_estimate_plan<3, false>(1024, 1024).fixed_bytes == 67648 &&
                  normal_estimate_plan<3, false>(1024, 1024).list_threads == 448 &&
                  normal_estimate_plan<3, false>(512, 1024).list_threads == 448 &&
                  normal_estimate_plan<3, false>(1024, 1024).shared_bytes == 448 * 192,
              "m = 1024");
static_assert(normal_estimate_plan<3, false>(1024, kPlaneBatchMaxM).fixed_bytes == 133184 &&
                  kTinyLdsGrant - normal_estimate_plan<3, false>(1024, kPlaneBatchMaxM).fixed_bytes == 30400 &&
                  normal_estimate_plan<3, false>(512, kPlaneBatchMaxM).list_threads == 128 &&
                  normal_estimate_plan<3, false>(1024, kPlaneBatchMaxM).list_threads == 128 &&
                  normal_estimate_plan<3, false>(1024, kPlaneBatchMaxM).shared_bytes == 3 * 1024 * 8 &&
                  normal_estimate_plan<3, false>(1024, kPlaneBatchMaxM).lds_bytes == 157760 &&
                  normal_estimate_plan<3, false>(1024, kPlaneBatchMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048: the sort buffers fit in what the fixed part leaves");

// -- the gated plane estimate's, and why its record is one word: the record the line kernel keeps (x | y as f64 and the
// position, with z 28 B a pair) does not fit behind the sort buffers beyond 1664 targets
constexpr size_t plane_gate_line_style_bytes(unsigned threads) {
  return (size_t)threads * (3 * sizeof(double) + sizeof(uint32_t)) + 16 * sizeof(uint32_t);
}
// (what a 1024-thread workgroup of m targets would need with the line kernel's record behind its sort buffers)
constexpr size_t plane_line_style_lds(unsigned m) {
  return normal_estimate_plan<3, false>(1024, m).fixed_bytes + 3 * 1024 * 8 + plane_gate_line_style_bytes(1024);
}
static_assert(normal_gate_bytes<3>(512) == 2112 && normal_gate_bytes<3>(1024) == 4160 &&
                  plane_gate_line_style_bytes(512) == 14400 && plane_gate_line_style_bytes(1024) == 28736,
              "the gate's words, and what the line kernel's record would take");
static_assert(normal_estimate_plan<3, true>(512, 1).list_threads == 64 &&
                  normal_estimate_plan<3, true>(1024, 1).list_threads == 64 &&
                  normal_estimate_plan<3, true>(512, 1).shared_bytes == 3 * 512 * 8 + 2112 &&
                  normal_estimate_plan<3, true>(1024, 1).shared_bytes == 3 * 1024 * 8 + 4160 &&
                  normal_estimate_plan<3, true>(512, 1).lds_bytes == 6208 + 14400 &&
                  normal_estimate_plan<3, true>(1024, 1).lds_bytes == 6208 + 28736,
              "m = 1: the sort buffers and the gate's words");
static_assert(normal_estimate_plan<3, true>(512, 1024).list_threads == 448 &&
                  normal_estimate_plan<3, true>(1024, 1024).list_threads == 448 &&
                  normal_estimate_plan<3, true>(512, 1024).lds_bytes == normal_estimate_plan<3, false>(512, 1024).lds_bytes &&
                  normal_estimate_plan<3, true>(1024, 1024).lds_bytes == 67648 + 448 * 192,
              "m = 1024: the gate's words lie where the lists were");
static_assert(normal_estimate_plan<3, false>(1024, 1664).fixed_bytes == 108608 && plane_line_style_lds(1664) == 161920 &&
                  plane_line_style_lds(1664) <= kTinyLdsGrant &&
                  normal_estimate_plan<3, true>(512, 1664).list_threads == 256 &&
                  normal_estimate_plan<3, true>(1024, 1664).list_threads == 256 &&
                  normal_estimate_plan<3, true>(512, 1664).lds_bytes == 108608 + 256 * 192 &&
                  normal_estimate_plan<3, true>(1024, 1664).lds_bytes == 108608 + 256 * 192,
              "m = 1664: the last m at which the line kernel's record would still fit; nothing on top of the ungated plan");
static_assert(normal_estimate_plan<3, false>(1024, 1665).fixed_bytes == 112704 && plane_line_style_lds(1665) > kTinyLdsGrant &&
                  normal_estimate_plan<3, true>(512, 1665).list_threads == 256 &&
                  normal_estimate_plan<3, true>(1024, 1665).list_threads == 256 &&
                  normal_estimate_plan<3, true>(512, 1665).lds_bytes == 112704 + 256 * 192 &&
                  normal_estimate_plan<3, true>(1024, 1665).lds_bytes == 161856,
              "m = 1665: the line kernel's record overflows the grant, the one word per pair does not");
static_assert(normal_estimate_plan<3, true>(512, kPlaneBatchMaxM).list_threads == 128 &&
                  normal_estimate_plan<3, true>(1024, kPlaneBatchMaxM).list_threads == 128 &&
                  normal_estimate_plan<3, true>(512, kPlaneBatchMaxM).lds_bytes == 157760 &&
                  normal_estimate_plan<3, true>(1024, kPlaneBatchMaxM).shared_bytes == 3 * 1024 * 8 + 4160 &&
                  normal_estimate_plan<3, true>(1024, kPlaneBatchMaxM).shared_bytes <= 30400 &&
                  normal_estimate_plan<3, true>(1024, kPlaneBatchMaxM).lds_bytes == 133184 + 28736 &&
                  normal_estimate_plan<3, true>(1024, kPlaneBatchMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048: 28 736 of the 30 400 bytes the fixed part leaves");

// -- the qualities': the smallest item (the fold sizes the region); line: a golden scan (two rounds of 640), the largest
// item (rounds of 320); plane: 1024 targets (three rounds of 448), the largest item (sixteen rounds of 128: their lists
// are just above the fold's bytes)
static_assert(kNormalQualityThreads / 64 * 6 * sizeof(double) <= normal_quality_plan<2>(1).fixed_bytes, "the box's wave minima");
static_assert(normal_quality_plan<2>(1).list_threads == 64 && normal_quality_plan<2>(1).shared_bytes == kNormalQualityFoldBytes,
              "m = 1");
static_assert(normal_quality_plan<2>(668).list_threads == 640 && normal_quality_plan<2>(668).shared_bytes == 640 * 192 &&
                  normal_quality_plan<2>(668).lds_bytes == 156992,
              "m = 668");
static_assert(normal_quality_plan<2>(kLineQualityMaxM).list_threads == 320 &&
                  normal_quality_plan<2>(kLineQualityMaxM).shared_bytes == 320 * 192 &&
                  normal_quality_plan<2>(kLineQualityMaxM).lds_bytes == 160064 &&
                  normal_quality_plan<2>(kLineQualityMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048");
static_assert(normal_quality_plan<3>(1).fixed_bytes == 4416 && normal_quality_plan<3>(1).list_threads == 64 &&
                  normal_quality_plan<3>(1).shared_bytes == kNormalQualityFoldBytes &&
                  normal_quality_plan<3>(1).lds_bytes == 28352,
              "m = 1");
static_assert(normal_quality_plan<3>(1024).fixed_bytes == 65856 && normal_quality_plan<3>(1024).list_threads == 448 &&
                  normal_quality_plan<3>(1024).shared_bytes == 448 * 192 && normal_quality_plan<3>(1024).lds_bytes == 151872,
              "m = 1024");
static_assert(normal_quality_plan<3>(kPlaneQualityMaxM).fixed_bytes == 131392 &&
                  normal_quality_plan<3>(kPlaneQualityMaxM).list_threads == 128 &&
                  normal_quality_plan<3>(kPlaneQualityMaxM).shared_bytes == 128 * 192 &&
                  normal_quality_plan<3>(kPlaneQualityMaxM).shared_bytes >= kNormalQualityFoldBytes &&
                  normal_quality_plan<3>(kPlaneQualityMaxM).lds_bytes == 155968 &&
                  normal_quality_plan<3>(kPlaneQualityMaxM).lds_bytes <= kTinyLdsGrant,
              "m = 2048");

// ... and at every m between, in both dimensions: within the grant, at least one round's lists and at most a list per
// thread, room for the lists, for the sort's keys and for what runs behind them in the shared region, room for the box's
// wave minima in front of it; the rounds of a gated estimate's normals those of the ungated one
template <int DIM, bool GATED>
constexpr bool normal_estimate_plan_fits_everywhere(unsigned max_m) {
  for (unsigned m = 1; m <= max_m; ++m)
    for (unsigned threads = 512; threads <= 1024; threads += 512) {
      const NormalPlan plan = normal_estimate_plan<DIM, GATED>(threads, m);
      if (plan.list_threads < 64 || plan.list_threads > threads || plan.lds_bytes > kTinyLdsGrant) return false;
      if (plan.list_threads != normal_estimate_plan<DIM, false>(threads, m).list_threads) return false;
      if (plan.shared_bytes < 3 * threads * 8 + (GATED ? normal_gate_bytes<DIM>(threads) : 0)) return false;
      if (plan.lds_bytes != plan.fixed_bytes + plan.shared_bytes) return false;
    }
  return true;
}
template <int DIM>
constexpr bool normal_quality_plan_fits_everywhere(unsigned max_m) {
  for (unsigned m = 1; m <= max_m; ++m) {
    const NormalPlan plan = normal_quality_plan<DIM>(m);
    if (plan.lds_bytes > kTinyLdsGrant || plan.lds_bytes != plan.fixed_bytes + plan.shared_bytes) return false;
    if (plan.list_threads < 64 || plan.list_threads > kNormalQualityThreads || plan.list_threads % 64 != 0) return false;
    if (plan.shared_bytes < plan.list_threads * kNormalListBytes) return false;
    if (plan.shared_bytes < kNormalQualityFoldBytes || plan.shared_bytes < normal_keys_bytes(m)) return false;
    if (kNormalQualityThreads / 64 * 6 * sizeof(double) > plan.fixed_bytes - kNormalQualityCtlBytes) return false;
  }
  return true;
}
static_assert(normal_estimate_plan_fits_everywhere<2, false>(kLineBatchMaxM) &&
                  normal_estimate_plan_fits_everywhere<3, false>(kPlaneBatchMaxM),
              "every launch's LDS is within the grant");
static_assert(normal_estimate_plan_fits_everywhere<2, true>(kLineBatchMaxM) &&
                  normal_estimate_plan_fits_everywhere<3, true>(kPlaneBatchMaxM),
              "every gated launch's LDS is within the grant");
static_assert(normal_quality_plan_fits_everywhere<2>(kLineQualityMaxM) &&
                  normal_quality_plan_fits_everywhere<3>(kPlaneQualityMaxM),
              "every quality launch's LDS is within the grant");

// The item's targets sorted into LDS (tiny_sort_targets); *pos0: the sorted position of the target of original index 0;
// *bail = 1 for a NaN target: the single call decides what such a cloud is.  Both in LDS, preset to 0 by thread 0.
template <int DIM, unsigned B>
__device__ __forceinline__ void normal_sort_targets(const double *dst, double cx, double cy, double cz,
                                                    unsigned char *shared, const TinyTargets &tg, unsigned *pos0,
                                                    int *bail) {
  tiny_sort_targets<DIM, B>(dst, cx, cy, cz, reinterpret_cast<unsigned long long *>(shared), tg,
                            [&](unsigned j, unsigned k, double x, double y) {
                              if (k == 0) *pos0 = j;
                              if (NormalResidual<DIM>::nan_target(tg, j, x, y)) *bail = 1;
                            });
}

// ---- the normals of a workgroup's own targets ----
// Per target the k best by (d^2, index) from a sweep outwards over the targets SORTED BY x in LDS (tiny_device.hpp:
// tiny_k_best_of_target; exact: the k-nearest set under that order is unique), L targets per round with their lists in
// `shared` ((8 + 4) B x kTinyKBestMax x L, free again on return; at most 2048 / 128 = sixteen rounds), then the
// residual's normal_of_neighbours -> nrm.  kk: the entries' k, clamped here to m.  Every thread of the workgroup calls
// it; it ends with a barrier.
template <int DIM>
__device__ __forceinline__ void normals_of_sorted_targets(const TinyTargets &tg, double cx, double cy, double cz,
                                                          double scale, int kk, unsigned L, unsigned char *shared,
                                                          typename NormalResidual<DIM>::Normal *nrm) {
  const unsigned tid = threadIdx.x, m = tg.m;
  double *ld = reinterpret_cast<double *>(shared);                      // [kTinyKBestMax][L]: d^2
  uint32_t *li = reinterpret_cast<uint32_t *>(ld + kTinyKBestMax * L);  // [kTinyKBestMax][L]: (index << 16) | position
  int k = kk < (int)m ? kk : (int)m;
  k = k < kTinyKBestMax ? k : kTinyKBestMax;  // (the entries refuse k > 16: this only keeps the lists inside their rows)
  for (unsigned base = 0; base < m; base += L) {
    const unsigned j = base + tid;
    if (tid < L && j < m) {
      double *bd = ld + tid;
      const int cnt = tiny_k_best_of_target<DIM>(tg, j, cx, cy, DIM == 3 ? cz : 0., scale, k, L, bd, li + tid);
      NormalResidual<DIM>::normal_of_neighbours(cnt, [&](int q, int d) {
        return NormalResidual<DIM>::coordinate(tg, (unsigned)__double_as_longlong(bd[q * L]), d);
      }, nrm, j);
    }
  }
  __syncthreads();
}

// ---- one item of an estimate, by the workgroup's B threads ----
// Item i's result is what icp_create(DIM, dst_i) + the residual's normals (k) + its estimate return on a fresh handle, bit
// for bit, or the workgroup hands the item back (TinyResult::status = -1).  GATED: the gate between the search and the
// inner loop; r2, inl_all: the squared bound and the inlier counts (count x max_iter, or null).
template <int DIM, unsigned B, bool GATED>
__device__ __forceinline__ void normal_estimate_item(const double *__restrict__ src_all, const double *__restrict__ dst_all,
                                                     const TinyBatchItem *__restrict__ items, unsigned max_iter, int kk,
                                                     unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                     uint32_t *inner_all, uint32_t *idx_all, double r2, uint32_t *inl_all) {
  static_assert(B == 512 || B == 1024, "one or two blocks of the 512-thread fold tree, a power of two for the sort");
  extern __shared__ unsigned char lds_raw[];
  const TinyBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m;          // 1 <= n <= B, 1 <= m <= 2048 (api_batch.hip: the kind's limits)
  const double *__restrict__ src = src_all + item.src_first * DIM;
  const double *__restrict__ dst = dst_all + item.dst_first * DIM;
  TinyResult *res = res_all + item.slot;
  uint32_t *inner_out = inner_all ? inner_all + (size_t)item.slot * max_iter : nullptr;
  uint32_t *idx_out = idx_all ? idx_all + item.idx_first : nullptr;
  const unsigned tid = threadIdx.x;
  const int wave = tid >> 6;

  double cx, cy, cz, scale;  // (cz: +0.0 in two dimensions)
  if (!tiny_batch_box<DIM, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) {
    if (tid == 0) res->status = -1;
    return;
  }
  // ---- LDS carve-up (normal_batch_plan) ----  (targets are kept SORTED BY x: position j below is not the target's index)
  // (written out in both item bodies: behind a function of its own the kernels lose their instruction streams)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  double *tz = DIM == 3 ? ty + mp : nullptr;
  unsigned char *p = reinterpret_cast<unsigned char *>((DIM == 3 ? tz : ty) + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y, z relative to the box centre as f32, original index}
  p += sizeof(float4) * (mp + 4);
  typename NormalResidual<DIM>::Normal *nrm = reinterpret_cast<typename NormalResidual<DIM>::Normal *>(p);
  p += NormalResidual<DIM>::kNormalBytes * mp;  // the normal of the target at sorted position j
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then what runs behind them
  p += shared_bytes;
  double(*sm)[kPairSums] = reinterpret_cast<double(*)[kPairSums]>(p);
  p += sizeof(double) * 16 * kPairSums;
  double *tot = reinterpret_cast<double *>(p);
  p += sizeof(double) * 16;
  PairCtl *C = reinterpret_cast<PairCtl *>(p);
  const TinyTargets tg = {tx, ty, tz, g4, m};

  if (tid == 0) {
    C->T = item.init;
    C->nan = C->bail = 0;
    C->evals = 0;
    C->pos0 = 0;
    C->mad[0][0] = C->mad[0][1] = 0.;
  }
  if (tid < 16) {  // (the wave sums of the waves a 512-thread workgroup does not have stay +0.0)
#pragma unroll
    for (int q = 0; q < kPairSums; ++q) sm[tid][q] = 0.;
  }
  normal_sort_targets<DIM, B>(dst, cx, cy, cz, shared, tg, &C->pos0, &C->bail);
  if (C->bail) {  // (uniform)
    if (tid == 0) res->status = -1;
    return;
  }
  normals_of_sorted_targets<DIM>(tg, cx, cy, cz, scale, kk, L, shared, nrm);
  unsigned long long(*sbuf)[1][B] = reinterpret_cast<unsigned long long(*)[1][B]>(shared);  // two sort buffers, then the sorted keys
  const bool has = tid < n;
  double px = 0., py = 0., pz = 0.;
  if (has) {
    px = src[(size_t)tid * DIM];
    py = src[(size_t)tid * DIM + 1];
    if constexpr (DIM == 3) pz = src[(size_t)tid * DIM + 2];
  }
  // the pairs the inner loop sees: all n, thread t its own; gated: the kept ones, thread t the t-th of them
  unsigned cnt = n;
  bool hasp = has;
  int blocks = n > 512u ? 2 : 1;  // reduce_geometry(cnt) for cnt <= 1024: 512-thread blocks
  const NormalGate<DIM, B> gate(shared + (size_t)3 * B * 8);
  uint32_t *inl_out = GATED && inl_all ? inl_all + (size_t)item.slot * max_iter : nullptr;
  unsigned bi = 0xffffffffu;
  for (unsigned it = 0; it < max_iter; ++it) {
    const Pose T = C->T;
    // ---- transform (xy; z is carried) + exact nearest neighbour, the pair of k_line_gather / k_p2pl_gather ----
    PlanePair pr;
    pr.ax = pr.ay = pr.qx = pr.qy = pr.dz = pr.nx = pr.ny = pr.nz = 0.;
    double qx = 0., qy = 0.;
    unsigned nb = 0;  // sorted position of the nearest target
    bool in = false;  // (gated) the pair passes the gate
    if (has) {
      qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      qy = (T.r10 * px + T.r11 * py) + T.ty;
      unsigned nbo;  // original index of the nearest target
      tiny_nearest<DIM>(tg, qx, qy, pz, cx, cy, cz, scale, bi, &nb, &nbo);
      bi = nb;
      if (nb == 0xffffffffu) {  // no finite distance (NaN query): index 0, as a scan from 0 would
        nb = C->pos0;
        nbo = 0;
      }
      if constexpr (GATED) {  // k_lngate_stage's / k_plgate_stage's expressions
        const double ex = qx - tg.tx[nb], ey = qy - tg.ty[nb];
        double d2;
        if constexpr (DIM == 3) {
          const double dz = pz - tg.tz[nb];
          d2 = (ex * ex + ey * ey) + dz * dz;
        } else {
          d2 = ex * ex + ey * ey;
        }
        in = d2 <= r2;  // (false for a NaN d2)
      } else {
        NormalResidual<DIM>::pair(pr, tg, nrm, qx, qy, pz, nb);
      }
      if (idx_out && it + 1 == max_iter) idx_out[tid] = nbo;
    }
    if constexpr (GATED) {
      // ---- the gate: the kept pairs in thread order (stable), pair t to thread t ----
      // rank = kept lanes before this one in its wave + the counts of the waves before it; the kept lanes of a wave
      // write consecutive records
      const unsigned long long bal = __ballot(in);
      unsigned rank = (unsigned)__popcll(bal & ((1ull << (tid & 63)) - 1ull));
      if ((tid & 63) == 0) gate.cnt[wave] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned kept = 0;
#pragma unroll
      for (int w = 0; w < (int)(B / 64); ++w) {
        const unsigned c = gate.cnt[w];
        rank += w < wave ? c : 0u;
        kept += c;
      }
      if (in) gate.put(rank, tid, qx, qy, nb);
      cnt = (unsigned)__builtin_amdgcn_readfirstlane((int)kept);  // (the same in every thread)
      hasp = tid < cnt;
      blocks = cnt > 512u ? 2 : 1;
    }
    // ---- p2pl_loop_on_pairs (api_normal.hip) on the cnt pairs (pair_loop_device.hpp) ----
    tiny_pair_loop<B>(pr, hasp, cnt, blocks, C, sbuf, sm, tot, [&]() {
      if constexpr (GATED) {
        if (hasp) gate.pair(tid, pr, tg, nrm, src, C);
      }
    });
    if (tid == 0) {
      tiny_outer_tail(C, it, max_iter, inner_out);
      if constexpr (GATED) {
        // the iterations a fixed point skips repeat this one's search and gate: this one's count is theirs
        if (inl_out) {
          inl_out[it] = cnt;
          if (C->fixed && it + 2 < max_iter)
            for (unsigned k = it + 1; k + 1 < max_iter; ++k) inl_out[k] = cnt;
        }
      }
    }
    __syncthreads();
    if (C->nan | C->bail) break;
    if (C->fixed && it + 2 < max_iter) it = max_iter - 2;  // (uniform: the flag is the workgroup's)
  }
  if (tid == 0) {
    res->pose = C->T;
    res->evals = C->evals;
    res->sorted = C->evals;
    res->status = C->nan ? 3 : (C->bail ? -1 : 0);
  }
}

// ---- one item of a pose quality, by the workgroup's kNormalQualityThreads threads, a thread per source point ----
// (1 <= n <= 1024, 1 <= m <= 2048: api_batch.hip, the kind's limits).  Item i's record is what icp_create(DIM, dst_i) +
// the residual's normals (k) + its evaluation (src_i, T_i, max_dist) fold on a fresh handle, bit for bit.  Hand-backs
// (the item's record is left as the host preset it, pad != 0): a box that is not finite, a NaN target.
template <int DIM>
__device__ __forceinline__ void normal_quality_item(const double *src_all, const double *dst_all,
                                                    const QualityBatchItem *items, double r2, int kk, unsigned L,
                                                    unsigned shared_bytes, NormalQualityPart *res) {
  constexpr unsigned B = kNormalQualityThreads;
  extern __shared__ unsigned char lds_raw[];
  const QualityBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m, tid = threadIdx.x;
  const double *__restrict__ src = src_all + item.src_first * DIM;
  const double *__restrict__ dst = dst_all + item.dst_first * DIM;

  double cx, cy, cz, scale;  // (cz: +0.0 in two dimensions)
  if (!tiny_batch_box<DIM, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) return;
  // ---- LDS carve-up (normal_batch_plan) ----  (targets are kept SORTED BY x: position j below is not the target's index)
  // (written out in both item bodies: behind a function of its own the kernels lose their instruction streams)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  double *tz = DIM == 3 ? ty + mp : nullptr;
  unsigned char *p = reinterpret_cast<unsigned char *>((DIM == 3 ? tz : ty) + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y, z relative to the box centre as f32, original index}
  p += sizeof(float4) * (mp + 4);
  typename NormalResidual<DIM>::Normal *nrm = reinterpret_cast<typename NormalResidual<DIM>::Normal *>(p);
  p += NormalResidual<DIM>::kNormalBytes * mp;  // the normal of the target at sorted position j
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then what runs behind them
  p += shared_bytes;
  NormalQualityCtl *C = reinterpret_cast<NormalQualityCtl *>(p);
  const TinyTargets tg = {tx, ty, tz, g4, m};

  if (tid == 0) {
    C->pos0 = 0;
    C->bail = 0;
  }
  normal_sort_targets<DIM, B>(dst, cx, cy, cz, shared, tg, &C->pos0, &C->bail);
  if (C->bail) return;  // (uniform)
  normals_of_sorted_targets<DIM>(tg, cx, cy, cz, scale, kk, L, shared, nrm);

  // ---- transform (xy; z is carried), exact nearest neighbour from a cold start, the ten terms ----
  double v[kNormalQualitySums] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  unsigned in = 0, nan = 0;
  if (tid < n) {
    const double px = src[(size_t)tid * DIM], py = src[(size_t)tid * DIM + 1];
    double pz = 0.;
    if constexpr (DIM == 3) pz = src[(size_t)tid * DIM + 2];
    const double qx = (item.T.r00 * px + item.T.r01 * py) + item.T.tx;  // Transform::transform, src/transform.rs:22-24
    const double qy = (item.T.r10 * px + item.T.r11 * py) + item.T.ty;
    unsigned nb, nbo;  // sorted position / original index of the nearest target
    tiny_nearest<DIM>(tg, qx, qy, pz, cx, cy, cz, scale, 0xffffffffu, &nb, &nbo);
    if (nb == 0xffffffffu) nb = C->pos0;  // no finite distance (NaN query): index 0, as a scan from 0 would
    double q[DIM] = {qx, qy}, b[DIM], nn[DIM];
    if constexpr (DIM == 3) q[2] = pz;
    NormalResidual<DIM>::matched(tg, nrm, nb, b, nn);
    normal_quality_terms<DIM>(q, b, nn, r2, v, in, nan);
  }
  // ---- the tree of a batch item, k_quality_batch's ----
  // (the normals' lists are dead since the barrier behind their last round: the fold takes their place)
  FoldLds<kNormalQualitySums> &F = *reinterpret_cast<FoldLds<kNormalQualitySums> *>(shared);
  NormalQualityPart *grp = reinterpret_cast<NormalQualityPart *>(shared + sizeof(FoldLds<kNormalQualitySums>));
  fold_workgroup(F, grp, tid, n, v, in, nan, &res[item.slot]);
}

// ---- the launch of a family of these kernels: k512 for workgroups of 512 threads, k1024 for 1024 (a quality: both) ----
// grant: the family's, above 64 KB of dynamic LDS, asked once per process.  *granted = false: refused, nothing launches.
template <class... P, class... A>
hipError_t launch_one_workgroup_batch(TinyLdsGrant &grant, void (*k512)(P...), void (*k1024)(P...), unsigned threads,
                                      const NormalPlan &plan, unsigned count, hipStream_t stream, bool *granted, A... args) {
  *granted = grant.ask({reinterpret_cast<const void *>(k512), reinterpret_cast<const void *>(k1024)}, kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  const bool small = threads == 512u;
  hipLaunchKernelGGL(small ? k512 : k1024, dim3(count), dim3(small ? 512 : 1024), plan.lds_bytes, stream, args...);
  return hipGetLastError();
}

}  // namespace icp
