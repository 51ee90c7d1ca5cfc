// EXTENSION beyond the reference (include/icp_mi355x.h section 15): batched point-to-LINE registration, one workgroup per
// item.  Item i's result is what icp_create(2, dst_i) + icp_compute_target_line_normals(k) + icp_estimate_point_to_line
// return on a fresh handle, bit for bit (section 14; p2line.hip, p2plane.hip, api_ext.hip: p2pl_loop_on_pairs), or the
// workgroup hands the item back (TinyResult::status = -1) and api_batch.hip serves it through exactly those entries.
// Nothing crosses workgroups: no flag, no atomic, no barrier across them.  What a workgroup does:
//   box        fmin / fmax over its own targets (gn_fast.hip: tiny_batch_box restated for two dimensions)
//   targets    sorted by fl32(x - cx) into LDS, with the f32 screen records of tiny_estimate_body.inc
//   normals    per target the k best by (d^2, index) from a sweep outwards over the sorted targets (exact: the k-nearest
//              set under that order is unique), lists in LDS for as many targets per round as the grant allows, then
//              line_normal_of_neighbours (p2line_device.hpp), the statement k_line_normals evaluates
//   outer      transform, exact nearest neighbour (tiny_estimate_body.inc's sweep and prune), the pair of k_line_gather
//   inner      plane_residual, exact median and MAD of r from one bitonic sort of the keys (ranks on the sorted keys, as
//              k_tiny_eval's sorting path), the 13 sums of k_p2pl_accumulate in the tree of reduce_geometry(n) -- one or two
//              blocks of 512 folded as block_reduce_store, then k_final_reduce's fold over the blocks -- solve_update, the
//              three break tests in p2pl_loop_on_pairs' order, transform_new with the restated sin / cos
// Hand-back reasons: a box that is not finite; a NaN target coordinate; a rotation update outside the restated range of
// sin / cos.  A NaN residual is the item's ICP_NAN_INPUT.
#include "common.hpp"
#include "gn_device.hpp"
#include "p2line_device.hpp"
#include "p2plane_device.hpp"

namespace icp {

constexpr int kLineSums = kNAcc;  // jtj[9], jtr[3], huber error: what k_p2pl_accumulate folds

struct LineCtl {
  Pose Ti, T;
  double mad[2];
  int done, nan, bail, fixed;
  unsigned applied, evals, pos0, pad;
};

// ---- the LDS plan of a launch ----
// per workgroup, for its item's m targets (mp = m rounded up to 64): x | y (f64), the f32 screen records (+ 4 pads), the
// normals; then ONE shared region, sized by the launch; then the wave sums, the totals and LineCtl.  The shared region
// holds, one after the other: the target sort's keys (8 B x the next power of two of m), the k-best lists of the
// normals ((8 + 4) B x 16 per list-holding thread), the estimator's two sort buffers and sorted keys (3 x 8 B x B).
// Per-thread lists for every thread do not fit beside 2048 targets, so the normals run in rounds of `list_threads`
// targets: as many as the grant leaves room for, up to one per thread and per target.
constexpr size_t kLineLdsGrant = 160 * 1024 - 256;
constexpr size_t kLineListBytes = kLineKMax * (sizeof(double) + sizeof(uint32_t));
constexpr size_t line_fixed_bytes(unsigned m) {
  const size_t mp = (m + 63u) & ~63u;
  return mp * 2 * sizeof(double) + (mp + 4) * sizeof(float4) + mp * sizeof(double2) + sizeof(double) * 16 * kLineSums +
         sizeof(double) * 16 + 256;
}
static_assert(sizeof(LineCtl) <= 256, "LineCtl's share of the LDS");
static_assert(line_fixed_bytes(kLineBatchMaxM) + 3 * 1024 * 8 <= kLineLdsGrant &&
                  (kLineLdsGrant - line_fixed_bytes(kLineBatchMaxM)) / kLineListBytes >= 256,
              "2048 targets leave room for the sort buffers and for at least 256 lists");
struct LinePlan {
  unsigned list_threads, shared_bytes;
  size_t lds_bytes;
};
constexpr LinePlan line_batch_plan(unsigned threads, unsigned m_max) {
  const size_t fixed = line_fixed_bytes(m_max);
  size_t keys = 64;
  while (keys < m_max) keys <<= 1;
  const size_t fit = (kLineLdsGrant - fixed) / kLineListBytes / 64 * 64;
  size_t lists = (m_max + 63u) & ~63u;  // (a list per target is all a round can use)
  lists = lists < threads ? lists : threads;
  lists = lists < fit ? lists : fit;
  size_t shared = lists * kLineListBytes;
  shared = shared > keys * 8 ? shared : keys * 8;
  shared = shared > (size_t)3 * threads * 8 ? shared : (size_t)3 * threads * 8;
  return LinePlan{(unsigned)lists, (unsigned)shared, fixed + shared};
}
// the plan at its corners: the smallest item, a golden scan (two rounds of 640), the largest item (rounds of 320)
static_assert(line_batch_plan(512, 1).list_threads == 64 && line_batch_plan(512, 1).shared_bytes == 3 * 512 * 8, "m = 1");
static_assert(line_batch_plan(1024, 668).list_threads == 640 && line_batch_plan(1024, 668).lds_bytes == 158784, "m = 668");
static_assert(line_batch_plan(512, kLineBatchMaxM).list_threads == 320 && line_batch_plan(1024, kLineBatchMaxM).list_threads == 320 &&
                  line_batch_plan(1024, kLineBatchMaxM).lds_bytes == 161856 &&
                  line_batch_plan(1024, kLineBatchMaxM).lds_bytes <= kLineLdsGrant,
              "m = 2048");

// gn_fast.hip's tiny_batch_box for two dimensions: the centre of the targets' box and a bound on the screen's margin,
// false where the box is not finite.  Uses the start of the LDS as scratch (two barriers; free again on return).
template <unsigned B>
__device__ __forceinline__ bool line_batch_box(const double *dst, unsigned m, double *wpart, double *cx, double *cy,
                                               double *scale) {
  const unsigned tid = threadIdx.x;
  double v[4] = {__builtin_huge_val(), __builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
  for (unsigned k = tid; k < m; k += B)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const double x = dst[(size_t)k * 2 + d];
      v[d] = fmin(v[d], x);
      v[2 + d] = fmax(v[2 + d], x);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      v[d] = fmin(v[d], __shfl_xor(v[d], o));
      v[2 + d] = fmax(v[2 + d], __shfl_xor(v[2 + d], o));
    }
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) wpart[(tid >> 6) * 4 + q] = v[q];
  __syncthreads();
  double lo[2], hi[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    lo[d] = wpart[d];
    hi[d] = wpart[2 + d];
    for (unsigned w = 1; w < B / 64; ++w) {
      lo[d] = fmin(lo[d], wpart[w * 4 + d]);
      hi[d] = fmax(hi[d], wpart[w * 4 + 2 + d]);
    }
  }
  __syncthreads();
  double emax = 0., amax = 0.;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    ok = ok && __builtin_isfinite(lo[d]) && __builtin_isfinite(hi[d]);
    emax = fmax(emax, hi[d] - lo[d]);
    amax = fmax(amax, fmax(fabs(lo[d]), fabs(hi[d])));
  }
  ok = ok && __builtin_isfinite(emax);
  *cx = 0.5 * (lo[0] + hi[0]);
  *cy = 0.5 * (lo[1] + hi[1]);
  *scale = amax + 2. * emax + 1.;
  return ok;  // (the same in every thread)
}

// Bitonic sort of B keys, one per thread (gn_fast.hip's bitonic_sort2_1024 for one array and B threads): stages whose
// partner is in the same wave are register shuffles, the others go through LDS, double-buffered so that each costs one
// workgroup barrier.  On return thread t holds the t-th smallest key.
template <unsigned B>
__device__ __forceinline__ void line_sort_keys(unsigned long long &key, unsigned long long (*buf)[B]) {
  const unsigned tid = threadIdx.x;
  int cur = 0;
  for (unsigned k = 2; k <= B; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      unsigned long long p;
      if (j >= 64) {
        buf[cur][tid] = key;
        __syncthreads();
        p = buf[cur][tid ^ j];
        cur ^= 1;  // the next LDS stage writes the other buffer: nobody is still reading it
      } else {
        p = __shfl_xor(key, (int)j);
      }
      const bool keep_min = ((tid & j) == 0) == ((tid & k) == 0);
      key = keep_min ? (key < p ? key : p) : (key > p ? key : p);
    }
}

// gn_fast.hip's mad_ranks: the two middle order statistics of fl(|r - med|) over the n residuals whose keys are sorted
// in S, without sorting again (left of the median the distances fall with the index, right of it they rise: rounding is
// monotone).  Every thread ranks its own distance; those whose rank interval holds a wanted rank publish it.
__device__ __forceinline__ void line_mad_ranks(const unsigned long long *S, unsigned n, double med, unsigned lo_rank,
                                               unsigned hi_rank, double *out /* LDS, [2] */) {
  const unsigned tid = threadIdx.x;
  if (tid >= n) return;
  auto dist = [&](unsigned i) { return fabs(k2f(S[i]) - med); };
  unsigned p;
  {
    unsigned lo = 0, hi = n;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if (k2f(S[mid]) < med) lo = mid + 1;
      else hi = mid;
    }
    p = lo;
  }
  const double d = dist(tid);
  auto left_first = [&](bool strict) {
    unsigned lo = 0, hi = p;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      const double v = dist(mid);
      if (strict ? (v < d) : (v <= d)) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  };
  auto right_end = [&](bool strict) {
    unsigned lo = p, hi = n;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      const double v = dist(mid);
      if (strict ? (v < d) : (v <= d)) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  const unsigned less = (p - left_first(true)) + (right_end(true) - p);
  const unsigned leq = (p - left_first(false)) + (right_end(false) - p);
  if (less <= lo_rank && lo_rank < leq) out[0] = d;
  if (less <= hi_rank && hi_rank < leq) out[1] = d;
}

// what the f32 screen compares against for a best (or k-th best) exact distance d: rounded up (nn_brute.hip)
__device__ __forceinline__ float line_screen_bound(double d, double ec) {
  const double rr = sqrt(d) + ec;
  return (float)(rr * rr * 1.000004) * 1.000001f + 1e-37f;
}

template <unsigned B>
__global__ __launch_bounds__(B) void k_line_estimate_batch(const double *__restrict__ src_all,
                                                           const double *__restrict__ dst_all,
                                                           const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                           int kk, unsigned L, unsigned shared_bytes, TinyResult *res_all,
                                                           uint32_t *inner_all, uint32_t *idx_all) {
  static_assert(B == 512 || B == 1024, "one or two blocks of the 512-thread fold tree, a power of two for the sort");
  extern __shared__ unsigned char lds_raw[];
  const TinyBatchItem &item = items[blockIdx.x];  // (read in place: a copy of the pose would live in scratch)
  const unsigned n = item.n, m = item.m;          // 1 <= n <= B, 1 <= m <= kLineBatchMaxM (api_batch.hip: line_fits)
  const double *__restrict__ src = src_all + item.src_first * 2;
  const double *__restrict__ dst = dst_all + item.dst_first * 2;
  TinyResult *res = res_all + item.slot;
  uint32_t *inner_out = inner_all ? inner_all + (size_t)item.slot * max_iter : nullptr;
  uint32_t *idx_out = idx_all ? idx_all + item.idx_first : nullptr;
  const unsigned tid = threadIdx.x;
  const int wave = tid >> 6;

  double cx, cy, scale;
  if (!line_batch_box<B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &scale)) {
    if (tid == 0) res->status = -1;
    return;
  }
  // ---- LDS carve-up ----  (targets are kept SORTED BY x: position j below is not the target's index)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  unsigned char *p = reinterpret_cast<unsigned char *>(ty + mp);
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y relative to the box centre as f32, -, original index}
  p += sizeof(float4) * (mp + 4);
  double2 *nrm = reinterpret_cast<double2 *>(p);  // the line normal of the target at sorted position j
  p += sizeof(double2) * mp;
  unsigned char *shared = p;  // the target sort's keys, then the normals' lists, then the estimator's sort (line_batch_plan)
  p += shared_bytes;
  double(*sm)[kLineSums] = reinterpret_cast<double(*)[kLineSums]>(p);
  p += sizeof(double) * 16 * kLineSums;
  double *tot = reinterpret_cast<double *>(p);
  p += sizeof(double) * 16;
  LineCtl *C = reinterpret_cast<LineCtl *>(p);

  if (tid == 0) {
    C->T = item.init;
    C->nan = C->bail = 0;
    C->evals = 0;
    C->pos0 = 0;
    C->mad[0] = C->mad[1] = 0.;
  }
  if (tid < 16) {  // (the wave sums of the waves a 512-thread workgroup does not have stay +0.0)
#pragma unroll
    for (int q = 0; q < kLineSums; ++q) sm[tid][q] = 0.;
  }
  // ---- targets sorted by x (tiny_estimate_body.inc): keys = (order-preserving bits of fl32(x - cx), index) ----
  {
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(shared);
    unsigned P = 64;
    while (P < m) P <<= 1;
    for (unsigned k = tid; k < P; k += B) {
      unsigned long long key = ~0ull;
      if (k < m) {
        const unsigned u = __float_as_uint((float)(dst[(size_t)k * 2] - cx));
        const unsigned o = (u >> 31) ? ~u : (u | 0x80000000u);
        key = ((unsigned long long)o << 32) | k;
      }
      keys[k] = key;
    }
    __syncthreads();
    for (unsigned k2 = 2; k2 <= P; k2 <<= 1)
      for (unsigned j = k2 >> 1; j > 0; j >>= 1) {
        for (unsigned t = tid; t < (P >> 1); t += B) {
          const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const unsigned long long a = keys[i], c = keys[l];
          const bool up = (i & k2) == 0;
          if ((a > c) == up) {
            keys[i] = c;
            keys[l] = a;
          }
        }
        __syncthreads();
      }
    for (unsigned j = tid; j < mp + 4; j += B) {
      if (j < m) {
        const unsigned k = (unsigned)(keys[j] & 0xffffffffull);
        const double x = dst[(size_t)k * 2], y = dst[(size_t)k * 2 + 1];
        tx[j] = x;
        ty[j] = y;
        g4[j] = make_float4((float)(x - cx), (float)(y - cy), 0.f, __uint_as_float(k));
        if (k == 0) C->pos0 = j;
        if ((x != x) | (y != y)) C->bail = 1;  // a NaN target: the single call decides what such a cloud is
      } else {  // pads: beyond every bound
        g4[j] = make_float4(__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf(), __uint_as_float(0xffffffffu));
      }
    }
    __syncthreads();
  }
  if (C->bail) {  // (uniform)
    if (tid == 0) res->status = -1;
    return;
  }
  // ---- line normals: the k best by (d^2, index) of every target, L targets per round ----
  {
    double *ld = reinterpret_cast<double *>(shared);                // [kLineKMax][L]: d^2
    uint32_t *li = reinterpret_cast<uint32_t *>(ld + kLineKMax * L);  // [kLineKMax][L]: (index << 16) | sorted position
    int k = kk < (int)m ? kk : (int)m;
    k = k < kLineKMax ? k : kLineKMax;  // (the entries refuse k > 16: this only keeps the lists inside their rows)
    for (unsigned base = 0; base < m; base += L) {
      const unsigned j = base + tid;
      if (tid < L && j < m) {
        double *bd = ld + tid;
        uint32_t *bi = li + tid;
        const double x = tx[j], y = ty[j];
        const float4 own = g4[j];
        const double ec = (fmax(fabs(x - cx), fabs(y - cy)) + 2. * scale) * 1.2e-7 * 1.7320508075688774;
        // The k best are kept UNORDERED while the sweep runs, with the worst of them -- its (d^2, index) and its slot --
        // in registers: a candidate is refused without touching the list, an accepted one replaces the worst and the
        // new worst is found by k independent reads (a sorted insertion is a chain of dependent LDS accesses as long as
        // the deepest insertion among the wave's 64 lanes).  They are ordered once, after the sweep.
        float thr = __builtin_huge_valf();  // the screen's bound: the worst kept distance once k are kept
        double wd = __builtin_huge_val();
        uint32_t wi = 0xffffffffu;
        int wq = 0, cnt = 0;
        auto offer = [&](unsigned jj, unsigned orig) {
          const double dx = x - tx[jj], dy = y - ty[jj];
          const double dd = dx * dx + dy * dy;
          const uint32_t ti = (orig << 16) | jj;  // (index and position below 2^16: ordered as the indices are)
          if (cnt == k && !(dd < wd || (dd == wd && ti < wi))) return;
          const int at = cnt < k ? cnt : wq;
          bd[at * L] = dd;
          bi[at * L] = ti;
          if (cnt < k) ++cnt;
          if (cnt == k) {
            wd = bd[0];
            wi = bi[0];
            wq = 0;
            for (int q = 1; q < k; ++q) {
              const double dq = bd[q * L];
              const uint32_t iq = bi[q * L];
              if (dq > wd || (dq == wd && iq > wi)) {
                wd = dq;
                wi = iq;
                wq = q;
              }
            }
            thr = line_screen_bound(wd, ec);
          }
        };
        // outwards from the target's own position while a target's x alone does not rule it out: the f32 difference is
        // within ec of the true one and thr carries that margin, so fx^2 > thr  =>  strictly farther than the k-th best.
        // Four targets per step, their LDS reads in flight together (tiny_estimate_body.inc); unlike a nearest-neighbour
        // search a list must not be offered a target twice, so a step's slots past either end are masked, not repeated.
        auto visit = [&](const float4 g, unsigned jj, bool valid) {
          const float fx = own.x - g.x, fy = own.y - g.y;
          if (valid && !(__builtin_fmaf(fy, fy, fx * fx) > thr)) offer(jj, __float_as_uint(g.w));
        };
        offer(j, __float_as_uint(own.w));
        for (unsigned jj = j + 1; jj < m; jj += 4) {  // (g4 carries four +inf pads past mp)
          const float4 g0 = g4[jj], g1 = g4[jj + 1], g2 = g4[jj + 2], g3 = g4[jj + 3];
          const float f0 = own.x - g0.x;
          if (f0 * f0 > thr) break;  // sorted by x: everything further right is farther still
          visit(g0, jj, true);
          visit(g1, jj + 1, jj + 1 < m);
          visit(g2, jj + 2, jj + 2 < m);
          visit(g3, jj + 3, jj + 3 < m);
        }
        for (unsigned jj = j; jj > 0;) {
          const unsigned j0 = jj - 1, j1 = jj > 1 ? jj - 2 : 0, j2 = jj > 2 ? jj - 3 : 0, j3 = jj > 3 ? jj - 4 : 0;
          const float4 g0 = g4[j0], g1 = g4[j1], g2 = g4[j2], g3 = g4[j3];
          const float f0 = own.x - g0.x;
          if (f0 * f0 > thr) break;
          visit(g0, j0, true);
          visit(g1, j1, jj > 1);
          visit(g2, j2, jj > 2);
          visit(g3, j3, jj > 3);
          jj = j3;
        }
        // the (d^2, index) order: entry q's rank is the number of entries before it (the pairs are distinct); its
        // sorted position then goes where its d^2 was, at slot `rank` (every rank is known before the first is written)
        unsigned long long ranks = 0;
        for (int q = 0; q < cnt; ++q) {
          const double dq = bd[q * L];
          const uint32_t iq = bi[q * L];
          unsigned r = 0;
          for (int u = 0; u < cnt; ++u) {
            const double du = bd[u * L];
            const uint32_t iu = bi[u * L];
            r += (du < dq || (du == dq && iu < iq)) ? 1u : 0u;
          }
          ranks |= (unsigned long long)r << (4 * q);
        }
        for (int q = 0; q < cnt; ++q)
          bd[((ranks >> (4 * q)) & 15u) * L] = __longlong_as_double((long long)(bi[q * L] & 0xffffu));
        double nv[2];
        line_normal_of_neighbours(cnt, [&](int q, int d) {
          const unsigned pos = (unsigned)__double_as_longlong(bd[q * L]);
          return d == 0 ? tx[pos] : ty[pos];
        }, nv);
        nrm[j] = make_double2(nv[0], nv[1]);
      }
    }
    __syncthreads();
  }
  unsigned long long(*sbuf)[B] = reinterpret_cast<unsigned long long(*)[B]>(shared);  // two sort buffers ...
  unsigned long long *S = &sbuf[2][0];                                                 // ... and the sorted keys
  const bool has = tid < n;
  double px = 0., py = 0.;
  if (has) {
    px = src[(size_t)tid * 2];
    py = src[(size_t)tid * 2 + 1];
  }
  const int blocks = n > 512u ? 2 : 1;  // reduce_geometry(n) for n <= 1024: 512-thread blocks
  const unsigned lo_rank = (n - 1) / 2, hi_rank = n / 2;
  unsigned bi = 0xffffffffu;
  for (unsigned it = 0; it < max_iter; ++it) {
    const Pose T = C->T;
    // ---- transform + exact nearest neighbour (tiny_estimate_body.inc), the pair of k_line_gather ----
    PlanePair pr;
    pr.ax = pr.ay = pr.qx = pr.qy = pr.dz = pr.nx = pr.ny = pr.nz = 0.;
    if (has) {
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      const double ox = qx - cx, oy = qy - cy;
      const float hx = (float)ox, hy = (float)oy;
      const double ec = (fmax(fabs(ox), fabs(oy)) + 2. * scale) * 1.2e-7 * 1.7320508075688774;
      double best = __builtin_huge_val();
      float thr = __builtin_huge_valf();
      unsigned nb = 0xffffffffu, nbo = 0xffffffffu;  // sorted position / original index of the best so far
      auto exact = [&](unsigned j, unsigned orig) {
        const double dx = qx - tx[j], dy = qy - ty[j];
        const double d = dx * dx + dy * dy;
        if (d < best || (d == best && orig < nbo)) {  // ties -> lowest ORIGINAL index
          best = d;
          nb = j;
          nbo = orig;
          thr = line_screen_bound(d, ec);
        }
      };
      // start: the previous match (warm), else the first target at or right of the query's x
      unsigned start;
      if (bi != 0xffffffffu) {
        start = bi;
        exact(bi, __float_as_uint(g4[bi].w));
      } else {
        unsigned lo = 0, hi = m;
        while (lo < hi) {
          const unsigned mid = (lo + hi) >> 1;
          if (g4[mid].x < hx) lo = mid + 1;
          else hi = mid;
        }
        start = lo < m ? lo : m - 1;
      }
      auto visit = [&](const float4 g, unsigned j) {  // (beyond the x bound: s2 > thr as well)
        const float fx = hx - g.x, fy = hy - g.y;
        const float s2 = __builtin_fmaf(fy, fy, fx * fx);
        if (!(s2 > thr) && j < m) exact(j, __float_as_uint(g.w));
      };
      for (unsigned j = start; j < m; j += 4) {  // (g4 carries four +inf pads past mp)
        const float4 g0 = g4[j], g1 = g4[j + 1], g2 = g4[j + 2], g3 = g4[j + 3];
        const float f0 = hx - g0.x;
        if (f0 * f0 > thr) break;  // sorted by x: everything further right is farther still
        visit(g0, j);
        visit(g1, j + 1);
        visit(g2, j + 2);
        visit(g3, j + 3);
      }
      for (unsigned j = start; j > 0;) {
        const unsigned j0 = j - 1, j1 = j > 1 ? j - 2 : 0, j2 = j > 2 ? j - 3 : 0, j3 = j > 3 ? j - 4 : 0;
        const float4 g0 = g4[j0], g1 = g4[j1], g2 = g4[j2], g3 = g4[j3];  // (a repeated target is harmless)
        const float f0 = hx - g0.x;
        if (f0 * f0 > thr) break;
        visit(g0, j0);
        visit(g1, j1);
        visit(g2, j2);
        visit(g3, j3);
        j = j3;
      }
      bi = nb;
      if (nb == 0xffffffffu) {  // no finite distance (NaN query): index 0, as a scan from 0 would
        nb = C->pos0;
        nbo = 0;
      }
      const double2 nq = nrm[nb];
      pr.ax = qx;
      pr.ay = qy;
      pr.qx = tx[nb];
      pr.qy = ty[nb];
      pr.nx = nq.x;
      pr.ny = nq.y;
      if (idx_out && it + 1 == max_iter) idx_out[tid] = nbo;
    }
    // ---- p2pl_loop_on_pairs (api_ext.hip) on the n pairs ----
    if (tid == 0) {
      C->Ti = transform_identity();
      C->done = n < 2u ? 1 : 0;  // fewer than two pairs: the identity, no update
      C->applied = 0;
    }
    double prev_error = 1.7976931348623157e308;  // DBL_MAX (thread 0 only)
    __syncthreads();
    for (int k = 0; k < ICP_INNER_MAX_ITER && !C->done; ++k) {
      const Pose Ti = C->Ti;
      double r = 0.;
      if (has) {
        r = plane_residual(pr, Ti);
        if (r != r) C->nan = 1;
      }
      // exact median and MAD of r (launch_stddevs on ((r, 0), (0, 0)) under the identity: dimension 0's statistics of
      // ((1 r + 0 0) + 0) - 0 = r, which plane_residual's trailing + nz dz = + 0.0 has already rid of a -0.0)
      unsigned long long key = has ? f2k(r) : ~0ull;
      line_sort_keys<B>(key, sbuf);
      S[tid] = key;
      __syncthreads();
      const double xl = k2f(S[lo_rank]), xh = k2f(S[hi_rank]);
      const double med = (n & 1) ? xl : (xl + xh) / 2.;  // src/stats.rs:18-27
      line_mad_ranks(S, n, med, lo_rank, hi_rank, C->mad);
      __syncthreads();
      const double sigma = ICP_PPF34 * ((n & 1) ? C->mad[0] : (C->mad[0] + C->mad[1]) / 2.);  // src/stats.rs:42-46
      // k_p2pl_accumulate's terms, one pair per thread, folded as block_reduce_store folds a 512-thread block
      {
        double acc[kLineSums];
#pragma unroll
        for (int q = 0; q < kLineSums; ++q) acc[q] = 0.;
        if (has) {
          const double gw = 1. / sigma;
          const double e = r * r;
          if (sigma != 0.) {  // src/lib.rs:243-245
            const double a0 = -pr.ay, a1 = pr.ax;  // jacobian(), src/lib.rs:176-184
            const double b0 = Ti.r00 * a0 + Ti.r01 * a1;
            const double b1 = Ti.r10 * a0 + Ti.r11 * a1;
            const double J[3] = {pr.nx * Ti.r00 + pr.ny * Ti.r10, pr.nx * Ti.r01 + pr.ny * Ti.r11, pr.nx * b0 + pr.ny * b1};
            const double wg = huber_drho(e) * gw;
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[9 + q] = acc[9 + q] + (wg * J[q]) * r;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
              for (int b = 0; b < 3; ++b) acc[3 * a + b] = acc[3 * a + b] + (wg * J[a]) * J[b];
          }
          acc[12] = acc[12] + huber_rho(e);
        }
        wave_tree<kLineSums>(acc);
        if ((tid & 63) == 0) {
#pragma unroll
          for (int q = 0; q < kLineSums; ++q) sm[wave][q] = acc[q];
        }
      }
      __syncthreads();
      // the blocks' left folds of their eight wave sums, then k_final_reduce over the block sums: thread b of its one
      // 512-thread block holds 0 + sum_b, every other lane and wave +0.0, so its tree leaves (0 + sum_0) + (0 + sum_1)
      if (tid < (unsigned)kLineSums) {
        double p0 = sm[0][tid], p1 = 0.;
        for (int w = 1; w < 8; ++w) p0 = p0 + sm[w][tid];
        if (blocks > 1) {
          p1 = sm[8][tid];
          for (int w = 9; w < 16; ++w) p1 = p1 + sm[w][tid];
          p1 = 0. + p1;
        }
        tot[tid] = ((0. + p0) + p1) + 0.;
      }
      __syncthreads();
      if (tid == 0) {
        ++C->evals;
        double delta[3];
        if (C->nan) {
          C->done = 1;  // ICP_NAN_INPUT
        } else if (!solve_update(tot, tot + 9, delta)) {
          C->done = 1;
        } else if ((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2] < ICP_DELTA_NORM_THRESHOLD) {
          C->done = 1;
        } else if (tot[12] > prev_error) {
          C->done = 1;
        } else {
          prev_error = tot[12];
          bool in_range;
          const Pose D = transform_new_in_range(delta, &in_range);
          if (!in_range) {
            C->bail = 1;  // a rotation beyond the restated range of sin / cos: the single call's host serves
            C->done = 1;
          } else {
            C->Ti = transform_mul(D, Ti);
            ++C->applied;
          }
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (inner_out) inner_out[it] = C->applied;
      C->T = transform_mul(C->Ti, T);
      // An outer iteration that leaves the pose as it found it, bit for bit, is a fixed point of the loop: every later
      // iteration repeats it (tiny_estimate_body.inc).  Only the last one still runs: it reports the correspondences.
      const Pose &Tn = C->T;
      C->fixed = C->applied == 0 && __double_as_longlong(Tn.tx) == __double_as_longlong(T.tx) &&
                 __double_as_longlong(Tn.ty) == __double_as_longlong(T.ty) &&
                 __double_as_longlong(Tn.r00) == __double_as_longlong(T.r00) &&
                 __double_as_longlong(Tn.r01) == __double_as_longlong(T.r01) &&
                 __double_as_longlong(Tn.r10) == __double_as_longlong(T.r10) &&
                 __double_as_longlong(Tn.r11) == __double_as_longlong(T.r11);
      if (C->fixed && it + 2 < max_iter && inner_out)
        for (unsigned k = it + 1; k + 1 < max_iter; ++k) inner_out[k] = 0;
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

hipError_t launch_line_estimate_batch(unsigned threads, unsigned m_max, const double *d_src, const double *d_dst,
                                      const TinyBatchItem *d_items, unsigned count, unsigned max_iter, int k,
                                      TinyResult *res, uint32_t *inner, uint32_t *d_idx, hipStream_t stream, bool *granted) {
  // the grant above 64 KB of dynamic LDS, asked for both kernels once per process; refused: nothing launches
  static int lds_granted = 0;  // 0 not asked yet, 1 yes, -1 refused
  if (lds_granted == 0) {
    const void *kernels[] = {reinterpret_cast<const void *>(&k_line_estimate_batch<512>),
                             reinterpret_cast<const void *>(&k_line_estimate_batch<1024>)};
    lds_granted = 1;
    for (const void *kn : kernels)
      if (hipFuncSetAttribute(kn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLineLdsGrant) != hipSuccess) lds_granted = -1;
    if (lds_granted < 0) (void)hipGetLastError();
  }
  *granted = lds_granted > 0;
  if (!*granted || count == 0) return hipSuccess;
  const LinePlan plan = line_batch_plan(threads, m_max);
  if (threads == 512u)
    hipLaunchKernelGGL((k_line_estimate_batch<512>), dim3(count), dim3(512), plan.lds_bytes, stream, d_src, d_dst, d_items,
                       max_iter, k, plan.list_threads, plan.shared_bytes, res, inner, d_idx);
  else
    hipLaunchKernelGGL((k_line_estimate_batch<1024>), dim3(count), dim3(1024), plan.lds_bytes, stream, d_src, d_dst, d_items,
                       max_iter, k, plan.list_threads, plan.shared_bytes, res, inner, d_idx);
  return hipGetLastError();
}

}  // namespace icp
