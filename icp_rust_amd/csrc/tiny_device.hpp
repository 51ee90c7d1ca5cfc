// What the one-workgroup estimators share, each piece once: k_tiny_eval, k_tiny_estimate / k_tiny_estimate_batch
// (gn_fast.hip, tiny_estimate_body.inc), k_line_estimate_batch / k_line_estimate_gated_batch (p2line_batch.hip),
// k_plane_estimate_batch (p2plane_batch.hip) and, for the box, the targets and the search, k_line_quality_batch
// (quality_line.hip) and k_plane_quality_batch (quality_plane_batch.hip).  Every piece defines a result's bits -- the
// tie rule, the screen's margin, the order of the break tests -- and the batch entries promise what the single calls
// return, bit for bit: so there is one copy of each.  All functions are called by every thread of the workgroup unless
// they say otherwise.
#pragma once
#include <initializer_list>

#include "common.hpp"
#include "gn_device.hpp"

namespace icp {

// ---- the grant above 64 KB of dynamic LDS ----
constexpr size_t kTinyLdsGrant = 160 * 1024 - 256;
// Asked for a launch function's kernels once per process (the function keeps one of these in a static); refused: the
// caller launches nothing -- a kernel must never launch with an LDS size that was not granted.
struct TinyLdsGrant {
  int state = 0;  // 0 not asked yet, 1 yes, -1 refused
  bool ask(std::initializer_list<const void *> kernels, size_t bytes) {
    if (state == 0) {
      state = 1;
      for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) state = -1;
      if (state < 0) (void)hipGetLastError();
    }
    return state > 0;
  }
};

// ---- order statistics from a register bitonic sort ----
// Bitonic sort of NK x B keys, one key of each array per thread, the arrays in lockstep.  The compare-exchange stages
// whose partner is in the same wave (j < 64) are register shuffles; only the stages with j >= 64 go through LDS,
// double-buffered so that each costs ONE workgroup barrier.  (The first version ran all 55 stages of 1024 keys through
// LDS with a barrier each, twice per evaluation: 48 us per evaluation of a 650-point scan, 40 of them barriers.)  On
// return thread t holds the t-th smallest key of each array; the last LDS stage's readers may still be reading `buf`.
template <unsigned B, int NK>
__device__ __forceinline__ void tiny_bitonic_sort(unsigned long long (&key)[NK], unsigned long long (*buf)[NK][B]) {
  static_assert(B >= 64 && (B & (B - 1)) == 0, "a power of two, whole waves");
  const unsigned tid = threadIdx.x;
  int cur = 0;
  for (unsigned k = 2; k <= B; k <<= 1)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      unsigned long long p[NK];
      if (j >= 64) {
#pragma unroll
        for (int d = 0; d < NK; ++d) buf[cur][d][tid] = key[d];
        __syncthreads();
#pragma unroll
        for (int d = 0; d < NK; ++d) p[d] = buf[cur][d][tid ^ j];
        cur ^= 1;  // the next LDS stage writes the other buffer: nobody is still reading it
      } else {
#pragma unroll
        for (int d = 0; d < NK; ++d) p[d] = __shfl_xor(key[d], (int)j);
      }
      // ascending block (tid & k) == 0: the lower index keeps the smaller key
      const bool keep_min = ((tid & j) == 0) == ((tid & k) == 0);
#pragma unroll
      for (int d = 0; d < NK; ++d) key[d] = keep_min ? (key[d] < p[d] ? key[d] : p[d]) : (key[d] > p[d] ? key[d] : p[d]);
    }
}

// The two middle order statistics of fl(|r - med|) over the n residuals whose keys are sorted in
// S (src/stats.rs:30-37) WITHOUT sorting again: left of the median the distances fl(med - r) fall
// with the index, right of it fl(r - med) rise (rounding is monotone), so "how many distances are
// < d" and "<= d" are two binary searches on each side.  Every thread ranks its own distance; the
// threads whose rank interval [less, leq) holds a wanted rank publish it (equal values: benign).
__device__ __forceinline__ void mad_ranks(const unsigned long long *S, unsigned n, double med, unsigned lo_rank,
                                          unsigned hi_rank, double *out /* LDS, [2] */) {
  const unsigned tid = threadIdx.x;
  if (tid >= n) return;
  auto dist = [&](unsigned i) { return fabs(k2f(S[i]) - med); };
  // p = first index with r >= med (NaN residuals are reported through nan_flag; the loops are bounded)
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
  // left part [0, p): distances non-increasing in i -> {d_i < d} and {d_i <= d} are suffixes
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
  // right part [p, n): non-decreasing -> prefixes
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

// Median and sigma of each of NK residual arrays from their sorted keys, of which thread t holds the t-th smallest
// (tiny_bitonic_sort): the keys go to sorted[d] -- nobody may still be reading it --, the two middle ranks are plain
// lookups (src/stats.rs:18-27), the MADs come from ranks on the sorted keys (src/stats.rs:30-47; one array after the
// other: in lockstep is slower, measured).  mad: LDS, [NK][2].  Two barriers.
template <unsigned B, int NK>
__device__ __forceinline__ void tiny_sorted_median_sigma(const unsigned long long (&key)[NK], unsigned long long (*sorted)[B],
                                                         unsigned n, double (*mad)[2], double (&med)[NK], double (&sig)[NK]) {
  const unsigned tid = threadIdx.x;
  const unsigned lo_rank = (n - 1) / 2, hi_rank = n / 2;
#pragma unroll
  for (int d = 0; d < NK; ++d) sorted[d][tid] = key[d];
  __syncthreads();
#pragma unroll
  for (int d = 0; d < NK; ++d) {
    const double xl = k2f(sorted[d][lo_rank]), xh = k2f(sorted[d][hi_rank]);
    med[d] = (n & 1) ? xl : (xl + xh) / 2.;
  }
#pragma unroll
  for (int d = 0; d < NK; ++d) mad_ranks(sorted[d], n, med[d], lo_rank, hi_rank, mad[d]);
  __syncthreads();
#pragma unroll
  for (int d = 0; d < NK; ++d) sig[d] = ICP_PPF34 * ((n & 1) ? mad[d][0] : (mad[d][0] + mad[d][1]) / 2.);  // src/stats.rs:42-46
}

// ---- the targets' box ----
// A single call gets its targets' box from the handle's grid (build_grid); a batch item has no handle, so its workgroup
// first reduces min / max over its own targets -- fmin / fmax exactly as k_grid_bbox and build_grid fold them (NaN
// coordinates are skipped; exact and independent of the order), hence the same centre, bit for bit.  The screen's margin
// needs a bound on |coordinate| no smaller than build_grid's GridParams::scale = max |lo|, |hi| + hh, hh its cell size;
// hh <= max(2 emax, 1.26 emax, 1) <= 2 emax + 1 (emax the largest extent: the cell of ~2 targets has
// (2 vol / m)^(1/k) <= 2^(1/k) emax, a degenerate cloud gets 1, and the growth loop stops by 1.26 emax at the latest), so
// scale = max |lo|, |hi| + 2 emax + 1 serves; a larger margin only sends more candidates to the exact f64 test.  False
// (in every thread) where the box is not finite.  wpart: LDS scratch, [B / 64][6]; two barriers, free again on return.
template <int DIM, unsigned B>
__device__ __forceinline__ bool tiny_batch_box(const double *dst, unsigned m, double *wpart, double *cx, double *cy,
                                               double *cz, double *scale) {
  const unsigned tid = threadIdx.x;
  double v[6];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    v[d] = __builtin_huge_val();
    v[3 + d] = -__builtin_huge_val();
  }
  for (unsigned k = tid; k < m; k += B)
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const double x = dst[(size_t)k * DIM + d];
      v[d] = fmin(v[d], x);
      v[3 + d] = fmax(v[3 + d], x);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[d] = fmin(v[d], __shfl_xor(v[d], o));
      v[3 + d] = fmax(v[3 + d], __shfl_xor(v[3 + d], o));
    }
  if ((tid & 63) == 0)
#pragma unroll
    for (int q = 0; q < 6; ++q) wpart[(tid >> 6) * 6 + q] = v[q];
  __syncthreads();
  double lo[3], hi[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    lo[d] = wpart[d];
    hi[d] = wpart[3 + d];
    for (unsigned w = 1; w < B / 64; ++w) {
      lo[d] = fmin(lo[d], wpart[w * 6 + d]);
      hi[d] = fmax(hi[d], wpart[w * 6 + 3 + d]);
    }
  }
  __syncthreads();  // (everybody has read the wave minima before the caller carves the LDS up)
  double emax = 0., amax = 0.;
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d >= DIM) lo[d] = hi[d] = 0.;
    ok = ok && __builtin_isfinite(lo[d]) && __builtin_isfinite(hi[d]);
    emax = fmax(emax, hi[d] - lo[d]);
    amax = fmax(amax, fmax(fabs(lo[d]), fabs(hi[d])));
  }
  ok = ok && __builtin_isfinite(emax);
  *cx = 0.5 * (lo[0] + hi[0]);
  *cy = 0.5 * (lo[1] + hi[1]);
  *cz = 0.5 * (lo[2] + hi[2]);
  *scale = amax + 2. * emax + 1.;
  return ok;
}

// ---- the targets in LDS, and the exact nearest neighbour among them ----
// The m targets of a workgroup, kept SORTED BY x: position j below is not the target's index.  mp = m rounded up to 64.
struct TinyTargets {
  double *tx, *ty, *tz;  // [mp] each, exact (tz: three dimensions only)
  float4 *g4;            // [mp + 4]: {x, y, z relative to the box centre as f32, original index}, then four pads
  unsigned m;
};

// the f32 screen: how far a difference of f32 coordinates relative to the box centre may be from the true one, for a
// point at (ox, oy, oz) from the centre (oz = 0 in two dimensions) ...
__device__ __forceinline__ double tiny_screen_margin(double ox, double oy, double oz, double scale) {
  return (fmax(fmax(fabs(ox), fabs(oy)), fabs(oz)) + 2. * scale) * 1.2e-7 * 1.7320508075688774;
}
// ... and what the screen compares against for a best (or k-th best) exact distance d: rounded up (nn_brute.hip)
__device__ __forceinline__ float tiny_screen_bound(double d, double ec) {
  const double rr = sqrt(d) + ec;
  return (float)(rr * rr * 1.000004) * 1.000001f + 1e-37f;
}

// Targets sorted by x (once per call): keys = (order-preserving bits of fl32(x - cx), index), bitonic sort of the next
// power of two in LDS (`keys`: room for it, free again on return), then the exact coordinates and the screen records in
// sorted order and the four pads.  hook(j, k, x, y) sees the target of original index k at its sorted position j.
template <int DIM, unsigned B, class Hook>
__device__ __forceinline__ void tiny_sort_targets(const double *dst, double cx, double cy, double cz,
                                                  unsigned long long *keys, const TinyTargets &t, Hook hook) {
  const unsigned tid = threadIdx.x, m = t.m, mp = (m + 63u) & ~63u;
  unsigned P = 64;
  while (P < m) P <<= 1;
  for (unsigned k = tid; k < P; k += B) {
    unsigned long long key = ~0ull;
    if (k < m) {
      const unsigned u = __float_as_uint((float)(dst[(size_t)k * DIM] - cx));
      const unsigned o = (u >> 31) ? ~u : (u | 0x80000000u);
      key = ((unsigned long long)o << 32) | k;
    }
    keys[k] = key;
  }
  __syncthreads();
  for (unsigned kk = 2; kk <= P; kk <<= 1)
    for (unsigned j = kk >> 1; j > 0; j >>= 1) {
      for (unsigned s = tid; s < (P >> 1); s += B) {
        const unsigned i = ((s & ~(j - 1)) << 1) | (s & (j - 1)), l = i | j;
        const unsigned long long a = keys[i], c = keys[l];
        const bool up = (i & kk) == 0;
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
      const double x = dst[(size_t)k * DIM], y = dst[(size_t)k * DIM + 1];
      const double z = DIM == 3 ? dst[(size_t)k * DIM + 2] : 0.;
      t.tx[j] = x;
      t.ty[j] = y;
      if (DIM == 3) t.tz[j] = z;
      t.g4[j] = make_float4((float)(x - cx), (float)(y - cy), DIM == 3 ? (float)(z - cz) : 0.f, __uint_as_float(k));
      hook(j, k, x, y);
    } else {  // pads: beyond every bound
      t.g4[j] = make_float4(__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf(), __uint_as_float(0xffffffffu));
    }
  }
  __syncthreads();
}

// The exact nearest target of the query (qx, qy, qz) -- src/lib.rs:113-124 / 156-167 -- one query per calling thread:
// a sweep over the sorted targets that visits only those whose x lies within the current best distance of the query's,
// a few of them instead of all m (sweep and prune; exact: a target with |dx| > sqrt(best) is strictly farther).  It
// starts at `prev`, the sorted position of the previous match (warm), or, with prev = 0xffffffff, at the first target at
// or right of the query's x.  *pos / *orig: sorted position / original index of the nearest, ties to the lowest
// ORIGINAL index; *pos = 0xffffffff where no distance is finite (a NaN query): what then, the caller decides.
template <int DIM>
__device__ __forceinline__ void tiny_nearest(const TinyTargets &t, double qx, double qy, double qz, double cx, double cy,
                                             double cz, double scale, unsigned prev, unsigned *pos, unsigned *orig) {
  const unsigned m = t.m;
  const double ox = qx - cx, oy = qy - cy, oz = DIM == 3 ? qz - cz : 0.;
  const float hx = (float)ox, hy = (float)oy, hz = (float)oz;
  const double ec = tiny_screen_margin(ox, oy, oz, scale);
  double best = __builtin_huge_val();
  float thr = __builtin_huge_valf();
  unsigned nb = 0xffffffffu, nbo = 0xffffffffu;  // sorted position / original index of the best so far
  auto exact = [&](unsigned j, unsigned o) {
    const double dx = qx - t.tx[j], dy = qy - t.ty[j];
    double d = dx * dx + dy * dy;
    if (DIM == 3) {
      const double dz = qz - t.tz[j];
      d = d + dz * dz;
    }
    if (d < best || (d == best && o < nbo)) {  // ties -> lowest ORIGINAL index
      best = d;
      nb = j;
      nbo = o;
      thr = tiny_screen_bound(d, ec);
    }
  };
  unsigned start;
  if (prev != 0xffffffffu) {
    start = prev;
    exact(prev, __float_as_uint(t.g4[prev].w));
  } else {
    unsigned lo = 0, hi = m;
    while (lo < hi) {
      const unsigned mid = (lo + hi) >> 1;
      if (t.g4[mid].x < hx) lo = mid + 1;
      else hi = mid;
    }
    start = lo < m ? lo : m - 1;
  }
  // outwards in both directions while a target's x alone does not rule it out.  The f32 x
  // difference is within ec of the true one, so (|dx| - ec)^2 > best is what rules out; thr already
  // carries that margin: dx^2 > thr  =>  strictly farther.
  auto visit = [&](const float4 g, unsigned j) {  // (beyond the x bound: s2 > thr as well)
    const float fx = hx - g.x, fy = hy - g.y;
    float s2 = __builtin_fmaf(fy, fy, fx * fx);
    if (DIM == 3) {
      const float fz = hz - g.z;
      s2 = __builtin_fmaf(fz, fz, s2);
    }
    if (!(s2 > thr) && j < m) exact(j, __float_as_uint(g.w));
  };
  // four targets per step (their LDS reads in flight together: one CU has little else to hide the
  // latency with, and a wave is as slow as its lane with the widest window)
  for (unsigned j = start; j < m; j += 4) {  // (g4 carries four +inf pads past mp)
    const float4 g0 = t.g4[j], g1 = t.g4[j + 1], g2 = t.g4[j + 2], g3 = t.g4[j + 3];
    const float f0 = hx - g0.x;
    if (f0 * f0 > thr) break;  // sorted by x: everything further right is farther still
    visit(g0, j);
    visit(g1, j + 1);
    visit(g2, j + 2);
    visit(g3, j + 3);
  }
  for (unsigned j = start; j > 0;) {
    const unsigned j0 = j - 1, j1 = j > 1 ? j - 2 : 0, j2 = j > 2 ? j - 3 : 0, j3 = j > 3 ? j - 4 : 0;
    const float4 g0 = t.g4[j0], g1 = t.g4[j1], g2 = t.g4[j2], g3 = t.g4[j3];  // (a repeated target is harmless)
    const float f0 = hx - g0.x;
    if (f0 * f0 > thr) break;
    visit(g0, j0);
    visit(g1, j1);
    visit(g2, j2);
    visit(g3, j3);
    j = j3;
  }
  *pos = nb;
  *orig = nbo;
}

// ---- the k nearest targets of a target (the normals of the one-workgroup kernels: normal_batch_device.hpp:
// normals_of_sorted_targets<DIM>) ----
// The k best by (d^2, index) of the target at sorted position j, from a sweep outwards over the targets SORTED BY x
// (exact: the k-nearest set under that order is unique), one target per calling thread.  bd / bi: the thread's list in
// LDS, kTinyKBestMax entries each, entry q at [q * L].  Returns how many were found (min(k, m)); on return bd[q * L]
// holds, as an integer's bits, the sorted position of the q-th nearest in (d^2, index) order.  1 <= k <= kTinyKBestMax.
constexpr int kTinyKBestMax = 16;
constexpr unsigned kTinyKBestMaxTargets = 1u << 16;  // (original index << 16) | sorted position, in 32 bits
template <int DIM>
__device__ __forceinline__ int tiny_k_best_of_target(const TinyTargets &tg, unsigned j, double cx, double cy, double cz,
                                                     double scale, int k, unsigned L, double *bd, uint32_t *bi) {
  const unsigned m = tg.m;
  const double *tx = tg.tx, *ty = tg.ty, *tz = tg.tz;
  const float4 *g4 = tg.g4;
  const double x = tx[j], y = ty[j], z = DIM == 3 ? tz[j] : 0.;
  const float4 own = g4[j];
  const double ec = tiny_screen_margin(x - cx, y - cy, DIM == 3 ? z - cz : 0., scale);
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
    double dd = dx * dx + dy * dy;
    if (DIM == 3) {  // (dx dx + dy dy) + dz dz: k_target_normals' expression
      const double dz = z - tz[jj];
      dd = dd + dz * dz;
    }
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
      thr = tiny_screen_bound(wd, ec);
    }
  };
  // outwards from the target's own position while a target's x alone does not rule it out: the f32 difference is
  // within ec of the true one and thr carries that margin, so fx^2 > thr  =>  strictly farther than the k-th best.
  // Four targets per step, their LDS reads in flight together (as tiny_nearest); unlike a nearest-neighbour
  // search a list must not be offered a target twice, so a step's slots past either end are masked, not repeated.
  auto visit = [&](const float4 g, unsigned jj, bool valid) {
    const float fx = own.x - g.x, fy = own.y - g.y;
    float s2 = __builtin_fmaf(fy, fy, fx * fx);
    if (DIM == 3) {
      const float fz = own.z - g.z;
      s2 = __builtin_fmaf(fz, fz, s2);
    }
    if (valid && !(s2 > thr)) offer(jj, __float_as_uint(g.w));
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
  return cnt;
}

// ---- thread 0's part of the loops ----
// What the estimators' control blocks (in LDS) have in common; each kernel's block derives from it.  The two functions
// below read the poses from here, not from the copies the kernel's threads hold: handed the copies, every kernel needs
// about 12 VGPRs more.
struct TinyCtl {
  double prev_error;  // the inner loop's last error; f64::MAX before its first evaluation
  Pose Ti, T;         // the inner loop's pose (estimate_transform's), the outer loop's
  int done, nan, bail, fixed;
  unsigned applied, evals;
};

// The decision behind one inner evaluation (src/lib.rs:66-82; api_normal.hip: p2pl_loop_on_pairs takes the same steps),
// on thread 0 alone: the solve, the three break tests in the reference's order, then Transform::new * Ti.  tot: the
// combined totals, jtj[9] | jtr[3] | error.
__device__ __forceinline__ void tiny_inner_decide(TinyCtl *C, const double *tot) {
  ++C->evals;
  double delta[3];
  if (C->nan | C->bail) {
    C->done = 1;
  } else if (!solve_update(tot, tot + 9, delta)) {
    C->done = 1;  // None, src/lib.rs:67-69
  } else if ((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2] < ICP_DELTA_NORM_THRESHOLD) {
    C->done = 1;  // src/lib.rs:71-73
  } else if (tot[12] > C->prev_error) {
    C->done = 1;  // src/lib.rs:75-78
  } else {
    C->prev_error = tot[12];
    bool in_range;
    const Pose D = transform_new_in_range(delta, &in_range);
    if (!in_range) {
      C->bail = 1;  // a rotation beyond the restated range of sin / cos: the host-driven path serves
      C->done = 1;
    } else {
      C->Ti = transform_mul(D, C->Ti);  // src/lib.rs:81
      ++C->applied;
    }
  }
}

// The end of outer iteration `it`, which began at the pose C->T, on thread 0 alone: the inner count, the composed pose
// (src/lib.rs:127, 170), and the fixed-point test.  An outer iteration that leaves the pose as it found it, bit for
// bit, is a fixed point of the loop: every later iteration repeats it (correspondences and updates are functions of
// the pose and the two clouds).  Only the last one still runs -- it is the one that reports the correspondences; the
// inner counts between are 0, as the loop would find them.
__device__ __forceinline__ void tiny_outer_tail(TinyCtl *C, unsigned it, unsigned max_iter, uint32_t *inner_out) {
  const Pose T = C->T;
  if (inner_out) inner_out[it] = C->applied;
  C->T = transform_mul(C->Ti, T);
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

}  // namespace icp
