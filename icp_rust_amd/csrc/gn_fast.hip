// Dispatch of one inner Gauss-Newton evaluation (src/lib.rs:218-261 + :45-50) to the short
// pipelines, and the single-workgroup kernel for tiny inputs.
//
//   n <= 1024            k_tiny_eval below: ONE workgroup, ONE launch
//   otherwise            gn_pull.hip (7 or 9 launches; 15 with the full key, when either reports an
//                        overflow); icp_estimate's loop prefers gn_win.hip (3 launches) once it has a
//                        prediction -- see api.hip:wgn_step
//
// (The first short pipeline, whose launches ended in a last-workgroup tail, lived here; the
// "pull" variant replaced it: +8 % per step, same bits.  Its lessons are in DESIGN.md.)
#include <cstdio>

#include "common.hpp"
#include "gn_device.hpp"
#include "tiny_device.hpp"

namespace icp {

// ---------------------------------------------------------------------------------------
// n <= 1024 (the reference's own 2-D scans have ~650 points): the whole evaluation in ONE
// workgroup and ONE launch -- residuals, both medians (bitonic sort of the order-preserving keys:
// order statistics are then plain lookups), both MADs (ranked on the sorted residuals), and the weighted
// normal equations folded in exactly the multi-workgroup tree of reduce_geometry(n)
// (1 or 2 virtual blocks of 512 threads, then the 512-thread second stage), so the bits are
// the same as on the general path.
// (the sort, the ranks and the median / sigma block: tiny_device.hpp)

// src/stats.rs:18-27 on two order-preserving keys
__device__ __forceinline__ double middle_of_host(unsigned n, unsigned long long klo, unsigned long long khi) {
  const double lo = k2f(klo), hi = k2f(khi);
  return (n & 1) ? lo : (lo + hi) / 2.;
}

// fold `acc` over a group of 8 waves (512 threads) in the tree of block_reduce_store:
// wave shuffle tree, then a left fold of the wave sums from the group's first wave
template <int N>
__device__ __forceinline__ void group_reduce(double (&acc)[N], double (*sm)[N], int wave) {
  const int lane = threadIdx.x & 63;
  wave_tree<N>(acc);  // see block_reduce_store
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sm[wave][k] = acc[k];
  }
}

__global__ __launch_bounds__(1024) void k_tiny_eval(const double2 *__restrict__ a, const double2 *__restrict__ b,
                                                    unsigned n, Pose T, int blocks, GnResult *res,
                                                    unsigned seq) {
  __shared__ unsigned long long buf[2][2][1024];  // [buffer][x | y][slot]; buffer 0 ends up holding the sorted keys
  __shared__ double sm[16][kNSum + 1];
  __shared__ double part[2][kNSum + 1];
  __shared__ double s_tot[kNSum + 1];
  __shared__ double s_mad[2][2];
  __shared__ int s_nan;
  const unsigned tid = threadIdx.x;
  const int wave = tid >> 6;
#ifdef ICP_TINY_DEBUG
  long long tst[10];
  int tns = 0;
#define TSTAMP() tst[tns++] = wall_clock64()
#else
#define TSTAMP()
#endif
  TSTAMP();
  if (tid == 0) s_nan = 0;
  __syncthreads();
  const bool has = tid < n;
  double2 s = make_double2(0., 0.);
  double r0 = 0., r1 = 0.;
  if (has) {  // residual(), src/lib.rs:34-36
    s = a[tid];
    const double2 d = b[tid];
    r0 = ((T.r00 * s.x + T.r01 * s.y) + T.tx) - d.x;
    r1 = ((T.r10 * s.x + T.r11 * s.y) + T.ty) - d.y;
    if ((r0 != r0) | (r1 != r1)) s_nan = 1;
  }
  TSTAMP();
  // medians (src/stats.rs:11-28): sort the order-preserving keys, look the two middle ranks up; MADs
  // (src/stats.rs:30-47): ranks of the distances to the median, from the sorted residuals
  unsigned long long key[2] = {has ? f2k(r0) : ~0ull, has ? f2k(r1) : ~0ull};
  tiny_bitonic_sort<1024, 2>(key, buf);
  TSTAMP();
  __syncthreads();  // (the last LDS stage's readers)
  double med[2], sig[2];
  tiny_sorted_median_sigma<1024, 2>(key, buf[0], n, s_mad, med, sig);
  TSTAMP();
  // weighted normal equations + Huber error (src/lib.rs:238-255, 45-50), one point per thread
  double acc[kNSum + 1];
#pragma unroll
  for (int k = 0; k < kNSum + 1; ++k) acc[k] = 0.;
  if (has) accumulate_pair<false>(s, r0, r1, T, acc);
  TSTAMP();
  // stage 1: virtual blocks of 512 threads (8 waves each); a wave without points sums to +0.0
  if ((unsigned)wave * 64u < n) {
    group_reduce<kNSum + 1>(acc, sm, wave);
  } else if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kNSum + 1; ++k) sm[wave][k] = 0.;
  }
  __syncthreads();
  if (tid < 2 * (kNSum + 1)) {
    const int vb = tid / (kNSum + 1), k = tid % (kNSum + 1);
    double v = sm[8 * vb][k];
    for (int w = 1; w < 8; ++w) v = v + sm[8 * vb + w][k];
    part[vb][k] = v;
  }
  __syncthreads();
  // stage 2: one block of 512 threads over the `blocks` (<= 2) block sums.  Only threads 0 and 1 of
  // that block hold anything: every other operand of its wave tree and of the fold over its wave
  // sums is +0.0, and x + 0.0 is x (a -0.0 becomes +0.0, once and for all).  So lane 0 of wave 0
  // ends with (p0 + 0.0) + (p1 + 0.0) -- lane 1 joins at the last step -- and the fold adds zeros:
  // the same bits as the general path without its 84 shuffles.
  if (tid < kNSum + 1) {
    const double p0 = (0. + part[0][tid]) + 0.;
    const double p1 = blocks > 1 ? (0. + part[1][tid]) + 0. : 0.;
    s_tot[tid] = tid < kNSum ? (p0 + p1) + 0. : 0.;
  }
  __syncthreads();
  if (tid < kNAcc + 1) res->acc[tid] = tid < kNAcc ? combine_sum(s_tot, (int)tid, sig) : 0.;  // g_x S_x + g_y S_y
  TSTAMP();
  // everything the host reads is stored by lanes of wave 0, so one wave's fence orders it before
  // the sequence number (a system-scope fence in all sixteen waves cost 2 us)
  if (wave == 0) {
    if (tid == kNAcc + 1) {
      res->sigma[0] = sig[0];
      res->sigma[1] = sig[1];
    }
    if (tid == kNAcc + 2) {
      res->nan_flag = s_nan;
      res->overflow = 0;
    }
    __threadfence_system();
    TSTAMP();
    if (tid == 0) __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
#ifdef ICP_TINY_DEBUG
  TSTAMP();
  if (tid == 0 && (seq % 64) == 5)
    printf("[tiny] load %lld sort %lld median+mad %lld accumulate %lld reduce %lld fence %lld publish %lld (x10 ns)\n",
           tst[1] - tst[0], tst[2] - tst[1], tst[3] - tst[2], tst[4] - tst[3], tst[5] - tst[4], tst[6] - tst[5],
           tst[7] - tst[6]);
#endif
}

// =======================================================================================
// The WHOLE registration of a small cloud in ONE workgroup and ONE launch (round 2).
//
// Icp{2,3}d::estimate (src/lib.rs:105-130, 148-173) on the reference's own data -- 2-D scans of ~650
// points (scans/2d) -- used to be ~80 launches with a host round trip per inner iteration
// (src/lib.rs:66-82): 2.15 ms per estimate(20), level with one CPU core.  For n <= 1024 source points
// and m <= 2048 targets everything now stays on one CU: the targets live in LDS (exact f64 + an f32
// copy for the screen), every thread owns one source point; per outer iteration an exact
// nearest-neighbour sweep (warm-started from the previous match), then the inner loop -- residuals,
// the four exact order statistics, the weighted normal equations in the tree of reduce_geometry(n),
// and, on thread 0, the 3x3 solve, the two break tests and Transform::new * T (src/lib.rs:71-81) with
// the sin / cos of include/icp_trig.h, which the host and the oracle share -- so the bits are those of
// the host-driven path.
//
// Order statistics without a full sort (the bitonic sort of k_tiny_eval is 12 of its 29 us): 64
// evenly strided sample keys are sorted by one wave (register shuffles); every key finds its bucket
// among the 64 splitters; one wave scans the 65 counts, finds the bucket(s) of the two middle ranks; the
// ~10 keys in them are ranked by counting.  Exact for any input; more than 128 keys in the middle
// buckets (heavy duplicates) -> the sorting path below serves that evaluation.
// =======================================================================================
struct TinySel {
  unsigned spl[2][64];  // sorted splitters: the HIGH words of 64 sampled keys (monotone in the key, and 32-bit compares)
  unsigned long long list[2][128];
  unsigned long long out[2][2];
  unsigned hist[2][68];
  unsigned nlist[2];
  // round 4: the window the NEXT selection of the same kind (slot 0: medians, slot 1: MADs) tries first -- a key
  // range around this selection's middle ranks, per dimension (tiny_select_window below)
  unsigned long long wlo[2][2], whi[2][2];
  unsigned wvalid[2];
  unsigned wpos[2][2];  // where in the window's list the lower middle rank was expected (0xffffffff: unknown)
};
// ranks the window keeps on either side of the two middle ranks: twice the drift the last selection saw (the listed
// keys are ranked against each other: the cost grows with the square of their number)
constexpr unsigned kTinyWinMarginMin = 6, kTinyWinMarginMax = 32, kTinyWinMarginFirst = 16;

// cross-lane sums without the LDS pipe (DPP): over aligned groups of 8 lanes, and the wave's inclusive scan
#define ICP_DPP(v, ctrl, rows) (unsigned)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rows, 0xf, true)
__device__ __forceinline__ unsigned dpp_sum8(unsigned v) {
  v += ICP_DPP(v, 0xB1, 0xf);   // quad_perm [1,0,3,2]
  v += ICP_DPP(v, 0x4E, 0xf);   // quad_perm [2,3,0,1]
  v += ICP_DPP(v, 0x141, 0xf);  // row_half_mirror: lane i of an 8-group reads lane 7-i, in the other quad
  return v;
}

#ifdef ICP_TINY_PROFILE
#define SEL_STAMP(slot)                                             \
  do {                                                              \
    if (sp) {                                                       \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
      sp[slot] += now_ - st_;                                       \
      st_ = now_;                                                   \
    }                                                               \
  } while (0)
#else
#define SEL_STAMP(slot) ((void)0)
#endif

// the two middle order statistics (ranks (n-1)/2 and n/2) of the keys k0 (dimension 0) and k1, one
// key of each per thread (~0 from the threads past n); false: too many equal-ish keys, the caller
// sorts instead. B threads (a multiple of 64), five barriers, no single-wave phase: sample 64 keys per dimension
// and rank the samples (every thread a few compares) -> bucket every key between the sorted
// samples -> every wave scans the 65 bucket counts itself and the keys of the bucket(s) holding
// the two ranks are listed -> the listed keys are ranked against each other, 8 lanes per key.
// kbuf: 2 x 1024 keys of LDS (the sorting path's buffer).
template <unsigned B>
__device__ __forceinline__ bool tiny_select(unsigned long long k0, unsigned long long k1, bool has, unsigned n,
                                            TinySel *S, unsigned long long (*kbuf)[1024],
                                            unsigned long long *sp = nullptr, int wslot = -1) {
#ifdef ICP_TINY_PROFILE
  unsigned long long st_ = __builtin_amdgcn_s_memtime();
#endif
  // (opaque to the optimiser: everything below that depends on n alone -- the sample positions,
  // for one -- would otherwise be hoisted out of the caller's loop and, at 128 registers, spilled)
  asm volatile("" : "+s"(n));
  const unsigned tid = threadIdx.x, lane = tid & 63;
  const unsigned lo_rank = (n - 1) / 2, hi_rank = n / 2;
  const unsigned long long key[2] = {k0, k1};
  kbuf[0][tid] = k0;
  kbuf[1][tid] = k1;
  if (tid < 2 * 68) (&S->hist[0][0])[tid] = 0;
  if (tid < 2) S->nlist[tid] = 0;
  __syncthreads();
  SEL_STAMP(0);
  // sample j is the key of thread floor(j n / ns); slot (d, i, c) compares sample i with samples 8c .. 8c+7
  for (unsigned slot = tid; slot < 1024u; slot += B) {  // (whole 8-lane groups: B is a multiple of 64)
    const unsigned d = slot >> 9, i = (slot >> 3) & 63, c = slot & 7;
    const unsigned ns = n < 64u ? n : 64u;  // (the missing samples sort last)
    const unsigned *kh = reinterpret_cast<const unsigned *>(kbuf[d]);
    // floor(j n / ns) without a division: ns is 64, or n itself (24-bit products: j < 64, n <= 1024)
    auto sample = [&](unsigned j) -> unsigned {
      const unsigned t = n >= 64u ? __umul24(j, n) >> 6 : j;
      return j < ns ? kh[2 * t + 1] : 0xffffffffu;
    };
    const unsigned si = sample(i);
    unsigned part = 0;
#pragma unroll
    for (unsigned u = 0; u < 8; ++u) {
      const unsigned j = 8 * c + u;
      const unsigned sj = sample(j);
      part += (sj < si) | ((sj == si) & (j < i));
    }
    const unsigned rank = dpp_sum8(part);
    if (c == 0) S->spl[d][rank] = si;
  }
  __syncthreads();
  SEL_STAMP(1);
  // bucket = number of splitters below the key's high word (monotone in the key): a branch-free
  // lower bound over the 64 sorted splitters, the two dimensions' LDS reads in flight together
  unsigned bucket[2] = {0, 0};
  {
    const unsigned kd0 = (unsigned)(k0 >> 32), kd1 = (unsigned)(k1 >> 32);
#pragma unroll
    for (unsigned step = 32; step > 0; step >>= 1) {
      const unsigned s0 = S->spl[0][bucket[0] + step - 1], s1 = S->spl[1][bucket[1] + step - 1];
      bucket[0] += s0 < kd0 ? step : 0u;
      bucket[1] += s1 < kd1 ? step : 0u;
    }
    const unsigned s0 = S->spl[0][bucket[0]], s1 = S->spl[1][bucket[1]];  // (positions 0 .. 63)
    bucket[0] += s0 < kd0;
    bucket[1] += s1 < kd1;
    if (has) {
      atomicAdd(&S->hist[0][bucket[0]], 1u);
      atomicAdd(&S->hist[1][bucket[1]], 1u);
    }
  }
  __syncthreads();
  SEL_STAMP(2);
  unsigned below[2], expect[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const unsigned c = S->hist[d][lane], c64 = S->hist[d][64];
    const unsigned inc = wave_scan_inclusive(c);
    const unsigned long long m_lo = __ballot(inc > lo_rank), m_hi = __ballot(inc > hi_rank);
    const unsigned b_lo = m_lo ? (unsigned)__ffsll((long long)m_lo) - 1u : 64u;
    const unsigned b_hi = m_hi ? (unsigned)__ffsll((long long)m_hi) - 1u : 64u;
    const unsigned tot63 = (unsigned)__builtin_amdgcn_readlane((int)inc, 63);
    below[d] = b_lo < 64u ? (unsigned)__builtin_amdgcn_readlane((int)(inc - c), (int)b_lo) : tot63;
    const unsigned upto = b_hi < 64u ? (unsigned)__builtin_amdgcn_readlane((int)inc, (int)b_hi) : tot63 + c64;
    expect[d] = upto - below[d];
    if (has && bucket[d] >= b_lo && bucket[d] <= b_hi) {
      const unsigned pos = atomicAdd(&S->nlist[d], 1u);
      if (pos < 128u) S->list[d][pos] = key[d];
    }
    if (wslot >= 0 && tid == 0) {  // the next selection of this kind looks two buckets either side of these first
      const bool usable = n >= 256u && b_lo < 64u && b_hi < 64u;
      S->wlo[wslot][d] = b_lo >= 3u ? (unsigned long long)S->spl[d][b_lo - 3] << 32 : 0ull;
      S->whi[wslot][d] = b_hi + 2u < 64u ? ((unsigned long long)S->spl[d][b_hi + 2] << 32) | 0xffffffffull : 0xfffffffffffffffeull;
      if (d == 0) S->wvalid[wslot] = usable ? 1u : 0u;
      else if (!usable) S->wvalid[wslot] = 0u;
      S->wpos[wslot][d] = 0xffffffffu;
    }
  }
  __syncthreads();
  SEL_STAMP(3);
  const unsigned cnt0 = S->nlist[0], cnt1 = S->nlist[1];
  const bool bad = cnt0 > 128u || cnt0 != expect[0] || cnt1 > 128u || cnt1 != expect[1];  // the same in every thread
  if (!bad) {  // listed key e is ranked by the 8 lanes (e, 0..7), each against every 8th listed key
    const unsigned cmax = cnt0 > cnt1 ? cnt0 : cnt1;
    for (unsigned slot = tid; slot < 8u * cmax; slot += B) {  // (whole 8-lane groups)
      const unsigned e = slot >> 3, c = slot & 7;
      const bool in0 = e < cnt0, in1 = e < cnt1;
      const unsigned long long ke0 = S->list[0][in0 ? e : 0], ke1 = S->list[1][in1 ? e : 0];
      unsigned acc0 = 0, acc1 = 0;  // keys below in the low half, equal keys in the high half (at most 128 each)
      for (unsigned j = c; j < cmax; j += 8) {
        const unsigned long long kj0 = S->list[0][j < cnt0 ? j : 0], kj1 = S->list[1][j < cnt1 ? j : 0];
        if (j < cnt0) acc0 += (unsigned)(kj0 < ke0) + ((unsigned)(kj0 == ke0) << 16);
        if (j < cnt1) acc1 += (unsigned)(kj1 < ke1) + ((unsigned)(kj1 == ke1) << 16);
      }
      acc0 = dpp_sum8(acc0);
      acc1 = dpp_sum8(acc1);
      if (c == 0) {
        if (in0) {
          const unsigned less = acc0 & 0xffffu, eq = acc0 >> 16, r_lo = lo_rank - below[0], r_hi = hi_rank - below[0];
          if (less <= r_lo && r_lo < less + eq) S->out[0][0] = ke0;
          if (less <= r_hi && r_hi < less + eq) S->out[0][1] = ke0;
        }
        if (in1) {
          const unsigned less = acc1 & 0xffffu, eq = acc1 >> 16, r_lo = lo_rank - below[1], r_hi = hi_rank - below[1];
          if (less <= r_lo && r_lo < less + eq) S->out[1][0] = ke1;
          if (less <= r_hi && r_hi < less + eq) S->out[1][1] = ke1;
        }
      }
    }
  }
  __syncthreads();
  SEL_STAMP(4);
  return !bad;
}

// The same two order statistics from a WINDOW (round 4): consecutive evaluations of a registration see almost the
// same residuals, so the keys between the previous selection's neighbours of the middle ranks are listed directly --
// every thread compares its key with the window's ends, the keys below the window are counted (ballot + one LDS
// atomic per wave), those inside are listed -- and ranked exactly as tiny_select ranks its buckets: three barriers
// instead of five, no sampling, no splitter search.  Exact whenever it answers: it answers only if both middle ranks
// fall among the listed keys (count below <= rank < count below + listed, at most 128 listed); otherwise false, with
// the window dropped, and the caller runs tiny_select (which sets a fresh one).  The next window is cut from this
// one's ranking: the keys `margin` ranks below / above the middle ranks (dropped if either side is short).
template <unsigned B>
__device__ __forceinline__ bool tiny_select_window(unsigned long long k0, unsigned long long k1, bool has, unsigned n,
                                                   TinySel *S, int wslot, unsigned long long *sp = nullptr) {
#ifdef ICP_TINY_PROFILE
  unsigned long long st_ = __builtin_amdgcn_s_memtime();
#endif
  asm volatile("" : "+s"(n));
  const unsigned tid = threadIdx.x, lane = tid & 63;
  const unsigned lo_rank = (n - 1) / 2, hi_rank = n / 2;
  const unsigned long long key[2] = {k0, k1};
  if (!S->wvalid[wslot]) return false;  // (uniform: written behind a barrier of the previous selection)
  const unsigned long long wl[2] = {S->wlo[wslot][0], S->wlo[wslot][1]}, wh[2] = {S->whi[wslot][0], S->whi[wslot][1]};
  __syncthreads();  // (everybody has read the window and the previous selection's S->out)
  if (tid < 2) {
    S->hist[tid][0] = 0;
    S->nlist[tid] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const bool under = has && key[d] < wl[d];
    const unsigned long long mb = __ballot(under);
    if (lane == 0 && mb) atomicAdd(&S->hist[d][0], (unsigned)__popcll(mb));
    if (has && !under && key[d] <= wh[d]) {
      const unsigned pos = atomicAdd(&S->nlist[d], 1u);
      if (pos < 128u) S->list[d][pos] = key[d];
    }
  }
  __syncthreads();
  SEL_STAMP(5);
  const unsigned below[2] = {S->hist[0][0], S->hist[1][0]};
  const unsigned cnt0 = S->nlist[0], cnt1 = S->nlist[1];
  const bool bad = cnt0 > 128u || cnt1 > 128u || lo_rank < below[0] || hi_rank >= below[0] + cnt0 || lo_rank < below[1] ||
                   hi_rank >= below[1] + cnt1;  // the same in every thread
  if (bad) {
    __syncthreads();  // (every thread has read the counts tiny_select is about to reset)
    if (tid == 0) S->wvalid[wslot] = 0u;
    return false;
  }
  // the next window: the keys `margin` ranks either side of the middle ranks in this list, margin = twice the drift
  // this selection saw (how far the lower middle rank landed from where the window was cut for it) + 4; a side
  // that cannot give half of it drops the window
  bool keep = true;
  unsigned t_lo[2], t_hi[2], margin = kTinyWinMarginFirst;
  {
    unsigned drift = 0;
    bool known = true;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const unsigned r_lo = lo_rank - below[d], exp_pos = S->wpos[wslot][d];
      known = known && exp_pos != 0xffffffffu;
      const unsigned dd = r_lo > exp_pos ? r_lo - exp_pos : exp_pos - r_lo;
      drift = dd > drift ? dd : drift;
    }
    if (known) {
      margin = 2u * drift + 4u;
      margin = margin < kTinyWinMarginMin ? kTinyWinMarginMin : (margin > kTinyWinMarginMax ? kTinyWinMarginMax : margin);
    }
  }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const unsigned r_lo = lo_rank - below[d], r_hi = hi_rank - below[d], c = d ? cnt1 : cnt0;
    t_lo[d] = r_lo > margin ? r_lo - margin : 0u;
    t_hi[d] = r_hi + margin < c ? r_hi + margin : c - 1u;
    keep = keep && r_lo >= margin / 2 && r_hi + margin / 2 < c;
  }
  __syncthreads();  // (everybody has read wpos)
  if (tid < 2) S->wpos[wslot][tid] = (lo_rank - below[tid]) - t_lo[tid];
  {
    const unsigned cmax = cnt0 > cnt1 ? cnt0 : cnt1;
    for (unsigned slot = tid; slot < 8u * cmax; slot += B) {  // (whole 8-lane groups)
      const unsigned e = slot >> 3, c = slot & 7;
      const bool in0 = e < cnt0, in1 = e < cnt1;
      const unsigned long long ke0 = S->list[0][in0 ? e : 0], ke1 = S->list[1][in1 ? e : 0];
      unsigned acc0 = 0, acc1 = 0;
      for (unsigned j = c; j < cmax; j += 8) {
        const unsigned long long kj0 = S->list[0][j < cnt0 ? j : 0], kj1 = S->list[1][j < cnt1 ? j : 0];
        if (j < cnt0) acc0 += (unsigned)(kj0 < ke0) + ((unsigned)(kj0 == ke0) << 16);
        if (j < cnt1) acc1 += (unsigned)(kj1 < ke1) + ((unsigned)(kj1 == ke1) << 16);
      }
      acc0 = dpp_sum8(acc0);
      acc1 = dpp_sum8(acc1);
      if (c == 0) {
        if (in0) {
          const unsigned less = acc0 & 0xffffu, eq = acc0 >> 16, r_lo = lo_rank - below[0], r_hi = hi_rank - below[0];
          if (less <= r_lo && r_lo < less + eq) S->out[0][0] = ke0;
          if (less <= r_hi && r_hi < less + eq) S->out[0][1] = ke0;
          if (less <= t_lo[0] && t_lo[0] < less + eq) S->wlo[wslot][0] = ke0;
          if (less <= t_hi[0] && t_hi[0] < less + eq) S->whi[wslot][0] = ke0;
        }
        if (in1) {
          const unsigned less = acc1 & 0xffffu, eq = acc1 >> 16, r_lo = lo_rank - below[1], r_hi = hi_rank - below[1];
          if (less <= r_lo && r_lo < less + eq) S->out[1][0] = ke1;
          if (less <= r_hi && r_hi < less + eq) S->out[1][1] = ke1;
          if (less <= t_lo[1] && t_lo[1] < less + eq) S->wlo[wslot][1] = ke1;
          if (less <= t_hi[1] && t_hi[1] < less + eq) S->whi[wslot][1] = ke1;
        }
      }
    }
    if (tid == 0 && !keep) S->wvalid[wslot] = 0u;
  }
  __syncthreads();
  SEL_STAMP(6);
  return true;
}

// (TinyResult and the size limits kTinyMax*: common.hpp, shared with the batch call's host side, api_batch.hip)

// The gate's words of a gated registration (k_tiny_estimate_gated_batch): a record per kept pair,
// in pair order -- the moved point (x | y, f64) and the sorted position of its match -- and the 16 wave counts.  They
// lie in the sorting path's buffers (p), which nobody uses between an outer iteration's search and its first
// selection: a record is written and read once, in between.
constexpr size_t kTinySortBufBytes = sizeof(unsigned long long) * 2 * 2 * 1024;
constexpr size_t tiny_gate_bytes(unsigned threads) {
  return (size_t)threads * (2 * sizeof(double) + sizeof(uint32_t)) + 16 * sizeof(uint32_t);
}
template <unsigned B>
struct TinyGate {
  double *qx, *qy;
  uint32_t *nb, *cnt;
  __device__ __forceinline__ explicit TinyGate(unsigned char *p)
      : qx(reinterpret_cast<double *>(p)), qy(qx + B), nb(reinterpret_cast<uint32_t *>(qy + B)), cnt(nb + B) {}
};

template <int DIM, unsigned B>
__global__ __launch_bounds__(B) void k_tiny_estimate(const double *__restrict__ src, unsigned n,
                                                        const double *__restrict__ dst, unsigned m, Pose T0,
                                                        unsigned max_iter, double cx, double cy, double cz, double scale,
                                                        TinyResult *res, uint32_t *inner_out, uint32_t *idx_out) {
  constexpr bool GATED = false;
  constexpr double r2 = 0.;
  constexpr uint32_t *inl_out = nullptr;
#include "tiny_estimate_body.inc"
}

// the LDS plan of a workgroup whose targets number at most m; the same with and without the gate
static constexpr size_t tiny_lds_bytes(int dim, unsigned m) {
  const size_t mp = (m + 63u) & ~63u;
  size_t b = mp * (size_t)dim * sizeof(double) + (mp + 4) * sizeof(float4) + 16;
  b += kTinySortBufBytes;
  b += (sizeof(TinySel) + 15) & ~size_t(15);
  b += sizeof(double) * 18 * (kNSum + 1);
  b += 512;  // Ctl
  return b;
}
static_assert(tiny_gate_bytes(512) == 10304 && tiny_gate_bytes(768) == 15424 && tiny_gate_bytes(1024) == 20544 &&
                  tiny_gate_bytes(1024) <= kTinySortBufBytes,
              "the gate's words of every workgroup size fit in the sorting path's buffers: nothing on top of the plan");
static_assert(kTinyMaxN == 1024 && kTinyMaxM == 2048, "the corners below");
static_assert(tiny_lds_bytes(2, 1) == 1024 + 68 * 16 + 16 + kTinySortBufBytes + ((sizeof(TinySel) + 15) & ~size_t(15)) + 2880 + 512 &&
                  tiny_lds_bytes(3, 1) == tiny_lds_bytes(2, 1) + 512 && tiny_lds_bytes(3, 1) <= 64 * 1024,
              "m = 1, every workgroup size, gated or not: below what needs a grant");
static_assert(tiny_lds_bytes(2, kTinyMaxM) == tiny_lds_bytes(2, 1) + (2048 - 64) * 32 &&
                  tiny_lds_bytes(3, kTinyMaxM) == tiny_lds_bytes(3, 1) + (2048 - 64) * 40 &&
                  tiny_lds_bytes(3, kTinyMaxM) <= 124 * 1024 && tiny_lds_bytes(3, kTinyMaxM) <= kTinyLdsGrant,
              "m = 2048, every workgroup size, gated or not: about 120 KB of the grant");

// Icp{2,3}d::estimate for a small cloud in one launch.  *status: 0 done, 3 NaN, -1 not served (too large,
// no bounding box, disabled, or the kernel handed the call back): the caller runs the general path.
hipError_t launch_tiny_estimate(icp_handle *h, const double *d_src, size_t n, const Pose &T0, size_t max_iter,
                                Pose *out, uint32_t *d_last_idx, uint32_t *inner_iters, int *status) {
  *status = -1;
  if (!h->single_launch || n < 1 || n > kTinyMaxN || h->m < 1 || h->m > kTinyMaxM || max_iter < 1 || max_iter > kTinyMaxIter ||
      !h->grid.built || h->nn_mode == ICP_NN_GRID)
    return hipSuccess;
  Workspace &w = h->ws;
  hipError_t e;
  // the 160 KB of dynamic LDS are granted once per process; if the runtime refuses, small clouds simply take the
  // general path (*status stays -1)
  static TinyLdsGrant grant;
  if (!grant.ask({reinterpret_cast<const void *>(&k_tiny_estimate<2, 512>), reinterpret_cast<const void *>(&k_tiny_estimate<2, 768>),
                  reinterpret_cast<const void *>(&k_tiny_estimate<2, 1024>), reinterpret_cast<const void *>(&k_tiny_estimate<3, 512>),
                  reinterpret_cast<const void *>(&k_tiny_estimate<3, 768>), reinterpret_cast<const void *>(&k_tiny_estimate<3, 1024>)},
                 kTinyLdsGrant))
    return hipSuccess;
  if (!w.h_tiny &&
      (e = hipHostMalloc(&w.h_tiny, sizeof(TinyResult) + kTinyMaxIter * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess)
    return e;
  TinyResult *res = reinterpret_cast<TinyResult *>(w.h_tiny);
  uint32_t *inner = reinterpret_cast<uint32_t *>(res + 1);
  const GridParams &g = h->grid.p;
  const double cx = 0.5 * (g.lo[0] + g.hi[0]), cy = 0.5 * (g.lo[1] + g.hi[1]), cz = 0.5 * (g.lo[2] + g.hi[2]);
  const size_t lds = tiny_lds_bytes(h->dim, (unsigned)h->m);
  // the smallest workgroup with a thread per source point: fewer waves per barrier, and registers
  // enough (1024 threads leave 128 per thread, and spill)
  const unsigned threads = n <= 512 ? 512u : (n <= 768 ? 768u : 1024u);
#define ICP_TINY_LAUNCH(D, BB)                                                                                       \
  hipLaunchKernelGGL((k_tiny_estimate<D, BB>), dim3(1), dim3(BB), lds, h->stream, d_src, (unsigned)n, h->d_dst, \
                     (unsigned)h->m, T0, (unsigned)max_iter, cx, cy, cz, g.scale, res, inner, d_last_idx)
  if (h->dim == 3) {
    if (threads == 512u) ICP_TINY_LAUNCH(3, 512);
    else if (threads == 768u) ICP_TINY_LAUNCH(3, 768);
    else ICP_TINY_LAUNCH(3, 1024);
  } else {
    if (threads == 512u) ICP_TINY_LAUNCH(2, 512);
    else if (threads == 768u) ICP_TINY_LAUNCH(2, 768);
    else ICP_TINY_LAUNCH(2, 1024);
  }
#undef ICP_TINY_LAUNCH
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return e;
  *status = res->status;
  if (res->status == 0) {
    *out = res->pose;
    if (inner_iters)
      for (size_t i = 0; i < max_iter; ++i) inner_iters[i] = inner[i];
    w.tiny_evals += res->evals;
    w.tiny_sorted += res->sorted;
#ifdef ICP_TINY_PROFILE
    if (getenv("ICP_TINY_PRINT"))
      fprintf(stderr, "[tiny] evals %u sorted %u; cycles: setup %llu search %llu select %llu sums %llu step %llu all %llu; "
              "selection phases (keys, sample ranks, buckets, scan+list, ranks): %llu %llu %llu %llu %llu; window selections "
              "(count + list, ranks): %llu %llu\n",
              res->evals, res->sorted, res->t[0], res->t[1], res->t[2], res->t[3], res->t[4], res->t[5], res->ts[0], res->ts[1],
              res->ts[2], res->ts[3], res->ts[4], res->ts[5], res->ts[6]);
#endif
  }
  return hipSuccess;
}

// =======================================================================================
// Batched small registrations (an extension beyond the reference, which has no batch call): one workgroup per item, the
// body above unchanged.  A single call gets its targets' box from the handle's grid; an item has no handle, so its
// workgroup first finds the box of its own targets (tiny_device.hpp: tiny_batch_box; a box that is not finite reports -1,
// not served, as a single call whose handle builds no grid takes the general path).  Items are independent: no barrier,
// flag or atomic across workgroups.
// (the head of both batch kernels, in a macro: behind a function of its own k_tiny_estimate_batch loses its instruction
// stream.  It puts in scope what tiny_estimate_body.inc names, but for GATED, r2 and inl_out)
#define ICP_TINY_BATCH_ITEM_HEAD                                                                                      \
  const TinyBatchItem &item = items[blockIdx.x]; /* (read in place: a copy of the pose would live in scratch) */     \
  const unsigned n = item.n, m = item.m;                                                                              \
  const double *__restrict__ src = src_all + item.src_first * DIM;                                                    \
  const double *__restrict__ dst = dst_all + item.dst_first * DIM;                                                    \
  TinyResult *res = res_all + item.slot;                                                                              \
  uint32_t *inner_out = inner_all ? inner_all + (size_t)item.slot * max_iter : nullptr;                               \
  uint32_t *idx_out = idx_all ? idx_all + item.idx_first : nullptr;                                                   \
  const Pose &T0 = item.init;                                                                                         \
  double cx, cy, cz, scale;                                                                                           \
  extern __shared__ unsigned char lds_raw[]; /* (its start is the box's scratch; the body carves it up afterwards) */ \
  if (!tiny_batch_box<DIM, B>(dst, m, reinterpret_cast<double *>(lds_raw), &cx, &cy, &cz, &scale)) {                  \
    if (threadIdx.x == 0) res->status = -1;                                                                           \
    return;                                                                                                           \
  }

template <int DIM, unsigned B>
__global__ __launch_bounds__(B) void k_tiny_estimate_batch(const double *__restrict__ src_all,
                                                              const double *__restrict__ dst_all,
                                                              const TinyBatchItem *__restrict__ items, unsigned max_iter,
                                                              TinyResult *res_all, uint32_t *inner_all, uint32_t *idx_all) {
  ICP_TINY_BATCH_ITEM_HEAD
  constexpr bool GATED = false;
  constexpr double r2 = 0.;
  constexpr uint32_t *inl_out = nullptr;
#include "tiny_estimate_body.inc"
}

// EXTENSION (include/icp_mi355x.h section 21): the same with the gate of icp_estimate_gated
// (section 10) in every item's outer iterations.  r2 = max_dist^2, formed in f64 by the caller; inl_all: count x max_iter
// kept counts, laid out like inner_all, or null.
template <int DIM, unsigned B>
__global__ __launch_bounds__(B) void k_tiny_estimate_gated_batch(const double *__restrict__ src_all,
                                                                 const double *__restrict__ dst_all,
                                                                 const TinyBatchItem *__restrict__ items,
                                                                 unsigned max_iter, double r2, TinyResult *res_all,
                                                                 uint32_t *inner_all, uint32_t *idx_all,
                                                                 uint32_t *inl_all) {
  ICP_TINY_BATCH_ITEM_HEAD
  constexpr bool GATED = true;
  uint32_t *inl_out = inl_all ? inl_all + (size_t)item.slot * max_iter : nullptr;
#include "tiny_estimate_body.inc"
}
#undef ICP_TINY_BATCH_ITEM_HEAD

size_t tiny_lds_bytes_of(int dim, unsigned m) { return tiny_lds_bytes(dim, m); }

// One launch of a family of six such kernels, k[DIM - 2][workgroup size: 512 | 768 | 1024], behind the family's grant
// (the same grant as the single kernels', asked for the six once per process).
template <class... P, class... A>
static hipError_t launch_tiny_batch(TinyLdsGrant &grant, void (*const (&k)[2][3])(P...), int dim, unsigned threads,
                                    unsigned m_max, unsigned count, hipStream_t stream, bool *granted, A... args) {
  *granted = grant.ask({reinterpret_cast<const void *>(k[0][0]), reinterpret_cast<const void *>(k[0][1]),
                        reinterpret_cast<const void *>(k[0][2]), reinterpret_cast<const void *>(k[1][0]),
                        reinterpret_cast<const void *>(k[1][1]), reinterpret_cast<const void *>(k[1][2])},
                       kTinyLdsGrant);
  if (!*granted || count == 0) return hipSuccess;
  hipLaunchKernelGGL(k[dim == 3 ? 1 : 0][threads == 512u ? 0 : (threads == 768u ? 1 : 2)], dim3(count), dim3(threads),
                     tiny_lds_bytes(dim, m_max), stream, args...);
  return hipGetLastError();
}

hipError_t launch_tiny_estimate_batch(int dim, unsigned threads, unsigned m_max, const double *d_src, const double *d_dst,
                                      const TinyBatchItem *d_items, unsigned count, unsigned max_iter, TinyResult *res,
                                      uint32_t *inner, uint32_t *d_idx, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;
  static constexpr decltype(&k_tiny_estimate_batch<2, 512>) k[2][3] = {
      {&k_tiny_estimate_batch<2, 512>, &k_tiny_estimate_batch<2, 768>, &k_tiny_estimate_batch<2, 1024>},
      {&k_tiny_estimate_batch<3, 512>, &k_tiny_estimate_batch<3, 768>, &k_tiny_estimate_batch<3, 1024>}};
  return launch_tiny_batch(grant, k, dim, threads, m_max, count, stream, granted, d_src, d_dst, d_items, max_iter, res,
                           inner, d_idx);
}

hipError_t launch_tiny_estimate_gated_batch(int dim, unsigned threads, unsigned m_max, const double *d_src,
                                            const double *d_dst, const TinyBatchItem *d_items, unsigned count,
                                            unsigned max_iter, double r2, TinyResult *res, uint32_t *inner, uint32_t *d_idx,
                                            uint32_t *inliers, hipStream_t stream, bool *granted) {
  static TinyLdsGrant grant;  // (these kernels' own)
  static constexpr decltype(&k_tiny_estimate_gated_batch<2, 512>) k[2][3] = {
      {&k_tiny_estimate_gated_batch<2, 512>, &k_tiny_estimate_gated_batch<2, 768>, &k_tiny_estimate_gated_batch<2, 1024>},
      {&k_tiny_estimate_gated_batch<3, 512>, &k_tiny_estimate_gated_batch<3, 768>, &k_tiny_estimate_gated_batch<3, 1024>}};
  return launch_tiny_batch(grant, k, dim, threads, m_max, count, stream, granted, d_src, d_dst, d_items, max_iter, r2, res,
                           inner, d_idx, inliers);
}

hipError_t launch_weighted_gn_fast(icp_handle *h, const double *d_a, const double *d_b, size_t n_, const Pose &T) {
  Workspace &w = h->ws;
  const unsigned n = (unsigned)n_;
  if (n <= 1024u) {
    int blocks, threads;
    reduce_geometry(n_, &blocks, &threads);
    if (threads == 512 && blocks <= 2) {  // the geometry k_tiny_eval reproduces
      hipLaunchKernelGGL(k_tiny_eval, dim3(1), dim3(1024), 0, h->stream, (const double2 *)d_a, (const double2 *)d_b, n,
                         T, blocks, w.h_res, ++w.seq);
      return hipGetLastError();
    }
  }
  return launch_weighted_gn_pull(h, d_a, d_b, n_, T);
}

}  // namespace icp
