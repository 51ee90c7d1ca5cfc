// The exact selection behind every evaluation a window cannot serve, and the unweighted pass.
//
// One inner Gauss-Newton evaluation (src/lib.rs:218-261 + :45-50) needs the exact median and MAD of the
// residuals (src/stats.rs:11-60): an MSD radix select over order-preserving 64-bit keys, 12-bit digits,
// LDS histograms flushed with integer atomics => exact and independent of arrival order.  The two middle
// order statistics of an even-length input are searched together (problem "lo" and problem "hi" share a
// histogram while they share a prefix).  Sums use a fixed tree (DESIGN.md "GN reduction order"): no float
// atomics, run-to-run bit-identical.
//
// ONE "pull" pipeline, the digit count a parameter of its launcher (launch_pull):
//   2 digits (3 beyond 4M pairs) + candidate lists -- the short pipeline, seven (nine) launches,
//     H(median, digit 0)  H(median, digit 1)  C(median)  H(MAD, digit 0)  H(MAD, digit 1)  C(MAD)  A
//     C appends the keys that share the resolved prefix to a list of at most kSelCap, the next launch ranks
//     them; more keys than that (duplicates at the order statistic) and the evaluation reports `overflow`.
//   6 digits, 12+12+12+12+12+4 bits -- the full key, fifteen launches,
//     H x 6  K(median)  H x 6  K(MAD)  A
//     the prefix then IS the key, so duplicates cannot hurt: it always answers.  K hands the key on as a
//     candidate list of length one, so H and A consume a stage exactly as they do behind C.  Without A
//     (launch_stddevs: callers that accumulate themselves read GnScalars::sigma) the second K does A's
//     clean-up, fourteen launches.
// Nobody waits for a last workgroup: the NEXT launch resolves the previous launch's output in its prologue,
// redundantly in every workgroup (a 2 x 4096-bin histogram or a <= 1024-key candidate list is a few us of
// L2-resident reads, all workgroups in parallel): the kernel boundary is the only synchronisation, and
// workgroup 0 records the resolved state for the launch after next.  (In the first, "push" version every
// selection launch ended with a serial tail -- arrival ticket -> one workgroup scans the histograms / ranks
// the candidates: 3.5-8 us per launch by in-kernel stamps.)  Only A, which must produce ONE sum, keeps a
// last-workgroup tail.  Every pipeline leaves the scratch in its rest state (k_sel_init's), whatever it found -- but
// for the flag of a NaN, which the host answers with Workspace::gn_dirty.
#include "common.hpp"
#include "gn_device.hpp"

namespace icp {

// the rest state of the selection scratch: every histogram role, ticket and counter zero, no flag set
__global__ void k_sel_init(SelState *sel, GnScalars *scal, uint32_t *hist, SelCtl *ctl, unsigned n) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  for (unsigned i = t; i < kSelRolesAll * kSelProblems * kSelBins; i += gridDim.x * blockDim.x) hist[i] = 0;
  if (t < sizeof(SelCtl) / sizeof(unsigned)) reinterpret_cast<unsigned *>(ctl)[t] = 0;
  if (t < kSelProblems) {
    const bool hi = t & 1;
    sel[t].prefix = 0;
    sel[t].rank = hi ? (n / 2) : ((n - 1) / 2);  // src/stats.rs:18-27
    sel[t].alias = hi ? (int)(t - 1) : -1;
    sel[t].pad = 0;
  }
  if (t == 0) {
    scal->nan_flag = 0;
    scal->overflow = 0;
    scal->median[0] = scal->median[1] = 0.;
    scal->sigma[0] = scal->sigma[1] = 0.;
  }
}

constexpr int kPullThreads = 1024;
constexpr int kPullBatch = 4;
constexpr int kPullPad = kSelBins + kSelBins / 64;  // bin + bin/64: conflict-free column sums

__device__ __forceinline__ void init_state(SelState (&st)[kSelProblems], unsigned n) {
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) {
    const bool hi = p & 1;
    st[p].prefix = 0;
    st[p].rank = hi ? (n / 2) : ((n - 1) / 2);  // src/stats.rs:18-27
    st[p].alias = hi ? p - 1 : -1;
    st[p].pad = 0;
  }
}

// Descend one radix digit for all problems from the histograms another launch produced.
// Executed by every workgroup (1024 threads); `lds` holds kSelProblems * kPullPad words.
__device__ __forceinline__ void resolve_hist(uint32_t *lds, const uint32_t *__restrict__ hist,
                                             SelState (&st)[kSelProblems], int pass, bool check_cap,
                                             bool &over) {
  __shared__ unsigned found_bin[kSelProblems], found_below[kSelProblems], found_cnt[kSelProblems];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool live[kSelProblems];
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) live[p] = st[p].alias < 0;
  constexpr int PER = (kSelProblems * kSelBins) / kPullThreads;
  unsigned v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = tid + kPullThreads * u, p = j / kSelBins;
    v[u] = live[p] ? hist[j] : 0u;
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int j = tid + kPullThreads * u, p = j / kSelBins, bin = j % kSelBins;
    lds[p * kPullPad + bin + (bin >> 6)] = v[u];
  }
  __syncthreads();
  if (wave < kSelProblems) {
    const int p = wave;
    int src = p;
    unsigned rank = 0;
#pragma unroll
    for (int pp = 0; pp < kSelProblems; ++pp)
      if (pp == p) {
        src = st[pp].alias >= 0 ? st[pp].alias : pp;
        rank = (unsigned)st[pp].rank;
      }
    const uint32_t *img = lds + src * kPullPad;
    unsigned tot = 0;
#pragma unroll 16
    for (int j = 0; j < 64; ++j) tot += img[lane * 65 + j];
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(inc, off);
      if (lane >= off) inc += t;
    }
    const unsigned excl = inc - tot;
    const unsigned long long owners = __ballot(excl <= rank && rank < excl + tot);
    if (owners) {
      const int L = __ffsll((long long)owners) - 1;
      const unsigned base = __shfl(excl, L);
      const unsigned c = img[L * 65 + lane];
      unsigned inc2 = c;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(inc2, off);
        if (lane >= off) inc2 += t;
      }
      const unsigned below = base + inc2 - c;
      if (c > 0 && below <= rank && rank < below + c) {
        found_bin[p] = L * 64 + lane;
        found_below[p] = below;
        found_cnt[p] = c;
      }
    }
  }
  __syncthreads();
  const int shift = pass_shift(pass);
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) {
    st[p].prefix |= (unsigned long long)found_bin[p] << shift;
    st[p].rank -= found_below[p];
    over |= check_cap && found_cnt[p] > (unsigned)kSelCap;
  }
#pragma unroll
  for (int p = 1; p < kSelProblems; p += 2)
    if (st[p].alias >= 0 && st[p].prefix != st[p - 1].prefix) st[p].alias = -1;
  __syncthreads();  // the caller reuses `lds`
}

// The order statistics themselves, from the candidate lists another launch appended.
// Executed by every workgroup (any blockDim); out[p] = key of problem p.
__device__ __forceinline__ void resolve_cand(unsigned long long *keys, const unsigned long long *__restrict__ cand,
                                             const unsigned *__restrict__ cand_cnt,
                                             const SelState (&st)[kSelProblems],
                                             unsigned long long (&out)[kSelProblems], bool &over) {
  __shared__ unsigned long long result[kSelProblems];
  const unsigned tid = threadIdx.x, nt = blockDim.x;
  if (tid < kSelProblems) result[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int l = 0; l < kSelProblems; ++l) {
    if (st[l].alias >= 0) continue;  // reads its partner's list
    unsigned c = cand_cnt[l];
    if (c > (unsigned)kSelCap) {
      over = true;
      c = kSelCap;
    }
    for (unsigned i = tid; i < c; i += nt) keys[i] = cand[l * kSelCap + i];
    __syncthreads();
    for (unsigned i = tid; i < c; i += nt) {
      const unsigned long long ki = keys[i];
      unsigned less = 0, eq = 0;
      for (unsigned j = 0; j < c; ++j) {
        const unsigned long long kj = keys[j];
        less += kj < ki;
        eq += kj == ki;
      }
#pragma unroll
      for (int p = l; p < kSelProblems; ++p) {
        if (p != l && st[p].alias != l) continue;
        const unsigned long long rank = st[p].rank;
        if ((unsigned long long)less <= rank && rank < (unsigned long long)less + eq) result[p] = ki;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) out[p] = result[p];
  __syncthreads();
}

__device__ __forceinline__ double middle(unsigned n, unsigned long long klo, unsigned long long khi) {
  const double lo = k2f(klo), hi = k2f(khi);
  return (n & 1) ? lo : (lo + hi) / 2.;  // src/stats.rs:18-27
}

// the element stream shared by H and C: MODE 0 computes and stores the residuals
// (residual(), src/lib.rs:34-36), MODE 1 re-reads them, MODE 2 keys |r - median| (stats.rs:35)
template <int MODE, typename F>
__device__ __forceinline__ void stream_keys(const double2 *__restrict__ a, const double2 *__restrict__ b,
                                            const Pose &T, double *__restrict__ rx, double *__restrict__ ry,
                                            unsigned n, double med0, double med1, bool &saw_nan, F &&f) {
  const unsigned G = gridDim.x * blockDim.x;
  for (unsigned base = blockIdx.x * blockDim.x + threadIdx.x; base < n; base += G * kPullBatch) {
    double v0[kPullBatch], v1[kPullBatch];
    double2 s[kPullBatch], d[kPullBatch];
#pragma unroll
    for (int u = 0; u < kPullBatch; ++u) {
      const unsigned i = base + u * G;
      if (i < n) {
        if (MODE == 0) {
          s[u] = a[i];
          d[u] = b[i];
        } else {
          v0[u] = rx[i];
          v1[u] = ry[i];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kPullBatch; ++u) {
      const unsigned i = base + u * G;
      if (i < n) {
        if (MODE == 0) {
          v0[u] = ((T.r00 * s[u].x + T.r01 * s[u].y) + T.tx) - d[u].x;
          v1[u] = ((T.r10 * s[u].x + T.r11 * s[u].y) + T.ty) - d[u].y;
          rx[i] = v0[u];
          ry[i] = v1[u];
          saw_nan |= (v0[u] != v0[u]) | (v1[u] != v1[u]);
        } else if (MODE == 2) {
          v0[u] = fabs(v0[u] - med0);
          v1[u] = fabs(v1[u] - med1);
        }
        f(f2k(v0[u]), f2k(v1[u]));
      }
    }
  }
}

// H: histogram of digit `pass` of the keys that match the prefix resolved so far.
//   MODE 0: median stage, digit 0.   MODE 1: median stage, digit 1 (resolves digit 0 first).
//   MODE 2: MAD stage; pass 0 first turns the median candidates into the median, pass 1
//           resolves digit 0 of the MAD search.
template <int MODE>
__global__ __launch_bounds__(kPullThreads) void k_pull_hist(const double2 *__restrict__ a,
                                                            const double2 *__restrict__ b, Pose T,
                                                            double *__restrict__ rx, double *__restrict__ ry,
                                                            unsigned n, int pass, const SelState *sel_in,
                                                            SelState *sel_out, GnScalars *scal,
                                                            const uint32_t *__restrict__ hist_prev,
                                                            uint32_t *hist_out,
                                                            const unsigned long long *__restrict__ cand_prev,
                                                            SelCtl *ctl) {
  __shared__ uint32_t lh[kSelProblems * kPullPad];
  SelState st[kSelProblems];
  bool over = false;
  double med0 = 0., med1 = 0.;
  if (MODE == 2 && pass == 0) {
    // the median: rank the candidates the previous launch collected (state of the median search in `sel`)
#pragma unroll
    for (int p = 0; p < kSelProblems; ++p) st[p] = sel_in[p];
    unsigned long long key[kSelProblems];
    resolve_cand(reinterpret_cast<unsigned long long *>(lh), cand_prev, ctl->cand_cnt_pull[0], st, key, over);
    med0 = middle(n, key[0], key[1]);
    med1 = middle(n, key[2], key[3]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      scal->median[0] = med0;
      scal->median[1] = med1;
    }
    init_state(st, n);
  } else {
    if (MODE == 2) {
      med0 = scal->median[0];
      med1 = scal->median[1];
    }
    if (pass >= 2) {  // third digit (large n): continue from the state the previous launch recorded
#pragma unroll
      for (int p = 0; p < kSelProblems; ++p) st[p] = sel_in[p];
    } else {
      init_state(st, n);
    }
    if (pass >= 1) {
      resolve_hist(lh, hist_prev, st, pass - 1, false, over);
      if (blockIdx.x == 0 && threadIdx.x == 0)
#pragma unroll
        for (int p = 0; p < kSelProblems; ++p) sel_out[p] = st[p];
    } else if (blockIdx.x == 0 && threadIdx.x < kSelProblems) {
      ctl->cand_cnt_pull[1][threadIdx.x] = 0;  // MAD candidates of the previous evaluation: A has read them
    }
  }
  if (over && blockIdx.x == 0 && threadIdx.x == 0) scal->overflow = 1;

  bool active[kSelProblems];
  unsigned long long prefix[kSelProblems];
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) {
    active[p] = st[p].alias < 0;
    prefix[p] = st[p].prefix;
  }
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p)
    if (active[p])
      for (unsigned i = threadIdx.x; i < kSelBins; i += kPullThreads) lh[p * kSelBins + i] = 0;
  __syncthreads();

  const int shift = pass_shift(pass);
  const unsigned mask = (1u << pass_bits(pass)) - 1u;
  const int hs = shift + pass_bits(pass);  // bits above the current digit (64 at pass 0)
  bool saw_nan = false;
  stream_keys<MODE>(a, b, T, rx, ry, n, med0, med1, saw_nan, [&](unsigned long long k0, unsigned long long k1) {
#pragma unroll
    for (int p = 0; p < kSelProblems; ++p) {
      if (!active[p]) continue;
      const unsigned long long key = (p < 2) ? k0 : k1;
      const bool match = (hs >= 64) || ((key >> hs) == (prefix[p] >> hs));
      if (match) atomicAdd(&lh[p * kSelBins + ((unsigned)(key >> shift) & mask)], 1u);
    }
  });
  if (MODE == 0 && saw_nan) atomicOr(&scal->nan_flag, 1);
  __syncthreads();
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p)
    if (active[p])
      for (unsigned i = threadIdx.x; i < kSelBins; i += kPullThreads) {
        const uint32_t c = lh[p * kSelBins + i];
        if (c) atomicAdd(&hist_out[p * kSelBins + i], c);
      }
}

// C: resolve the last digit (the 2nd, or the 3rd for large n), then append the keys sharing the
// 24- resp. 36-bit prefix to the candidate lists
template <int MODE>
__global__ __launch_bounds__(kPullThreads) void k_pull_compact(const double2 *__restrict__ a,
                                                               const double2 *__restrict__ b, Pose T,
                                                               double *__restrict__ rx, double *__restrict__ ry,
                                                               unsigned n, int stage, int digits,
                                                               const SelState *sel_in, SelState *sel_out,
                                                               GnScalars *scal,
                                                               const uint32_t *__restrict__ hist_prev,
                                                               unsigned long long *cand, SelCtl *ctl) {
  __shared__ uint32_t lh[kSelProblems * kPullPad];
  SelState st[kSelProblems];
  bool over = false;
  double med0 = 0., med1 = 0.;
  if (MODE == 2) {
    med0 = scal->median[0];
    med1 = scal->median[1];
  }
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) st[p] = sel_in[p];
  resolve_hist(lh, hist_prev, st, digits - 1, true, over);
  // the resolved state goes to the OTHER half of the state buffer: workgroups of this launch
  // that start later must still read the input state
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < kSelProblems; ++p) sel_out[p] = st[p];
    if (over) scal->overflow = 1;
  }
  bool active[kSelProblems];
  unsigned long long prefix[kSelProblems];
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) {
    active[p] = st[p].alias < 0;
    prefix[p] = st[p].prefix;
  }
  bool saw_nan = false;
  const int cshift = 64 - 12 * digits;  // keys sharing the digits resolved so far
  unsigned *cnt = ctl->cand_cnt_pull[stage];
  stream_keys<MODE>(a, b, T, rx, ry, n, med0, med1, saw_nan, [&](unsigned long long k0, unsigned long long k1) {
#pragma unroll
    for (int p = 0; p < kSelProblems; ++p) {
      if (!active[p]) continue;
      const unsigned long long key = (p < 2) ? k0 : k1;
      if ((key >> cshift) == (prefix[p] >> cshift)) {
        const unsigned pos = atomicAdd(&cnt[p], 1u);
        if (pos < (unsigned)kSelCap) cand[p * kSelCap + pos] = key;
      }
    }
  });
}

// K: ends a full-key stage.  One workgroup resolves the sixth digit -- the prefix is then the key itself -- and
// hands each problem's key on as a candidate list of length one with rank 0, which H<2> (the median) and A (sigma)
// rank as they rank C's lists.  It also leaves the stage's statistic in `scal` (sigma: for callers that accumulate
// themselves) and clears the stage's roles of digits 3..5: it is the last reader of the sixth digit's, and the
// launches that read the other two have finished.  `cleanup`: no A follows -- the rest of what A would clear.
__global__ __launch_bounds__(kPullThreads) void k_pull_key(unsigned n, int stage, bool cleanup, const SelState *sel_in,
                                                           SelState *sel_out, GnScalars *scal, uint32_t *hist,
                                                           unsigned long long *cand, SelCtl *ctl) {
  __shared__ uint32_t lh[kSelProblems * kPullPad];
  constexpr unsigned kRole = kSelProblems * kSelBins;
  uint32_t *late = hist + (kSelRoles + 3 * stage) * kRole;  // this stage's roles of digits 3, 4, 5
  SelState st[kSelProblems];
  bool over = false;
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) st[p] = sel_in[p];
  resolve_hist(lh, late + 2 * kRole, st, kSelPasses - 1, false, over);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < kSelProblems; ++p) {
      cand[p * kSelCap] = st[p].prefix;
      sel_out[p] = SelState{st[p].prefix, 0ull, -1, 0};
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double mid = middle(n, st[2 * j].prefix, st[2 * j + 1].prefix);
      if (stage == 0) scal->median[j] = mid;
      else scal->sigma[j] = ICP_PPF34 * mid;  // src/stats.rs:42-46
    }
  }
  // (write-through, as in A: the next evaluation may run on the handle's other stream)
  for (unsigned i = threadIdx.x; i < 3 * kRole; i += kPullThreads)
    __hip_atomic_store(&late[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (cleanup)
    for (unsigned i = threadIdx.x; i < kSelRoles * kRole; i += kPullThreads)
      __hip_atomic_store(&hist[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x < kSelProblems) {
    unsigned(*cnt)[kSelProblems] = ctl->cand_cnt_pull;
    __hip_atomic_store(&cnt[stage][threadIdx.x], cleanup ? 0u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cleanup) __hip_atomic_store(&cnt[stage ^ 1][threadIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// A: sigma from the MAD candidates, then src/lib.rs:238-255 (+ :45-50) in the fixed tree; the
// last workgroup folds the block sums and publishes to the host.
__global__ __launch_bounds__(kReduceThreads) void k_pull_accumulate(const double2 *__restrict__ a,
                                                                    const double *__restrict__ rx,
                                                                    const double *__restrict__ ry,
                                                                    unsigned n, Pose T, const SelState *sel,
                                                                    GnScalars *scal,
                                                                    const unsigned long long *__restrict__ cand,
                                                                    double *partials, uint32_t *hist,
                                                                    SelCtl *ctl, GnResult *res, unsigned seq) {
  __shared__ unsigned long long keys[kSelCap];
  SelState st[kSelProblems];
#pragma unroll
  for (int p = 0; p < kSelProblems; ++p) st[p] = sel[p];
  bool over = false;
  unsigned long long key[kSelProblems];
  resolve_cand(keys, cand, ctl->cand_cnt_pull[1], st, key, over);
  const double sig[2] = {ICP_PPF34 * middle(n, key[0], key[1]),  // src/stats.rs:42-46
                         ICP_PPF34 * middle(n, key[2], key[3])};
  double acc[kNSum];
#pragma unroll
  for (int k = 0; k < kNSum; ++k) acc[k] = 0.;
  accumulate_points(a, rx, ry, n, T, acc);
  block_reduce_store<kNSum, true>(acc, partials + (size_t)blockIdx.x * (kNSum + 1));
  // clear what the next evaluation accumulates into (nobody reads these in this launch)
  const unsigned G = gridDim.x * kReduceThreads;
  // (write-through: the next evaluation may run on the handle's other stream before this
  // kernel's end-of-kernel write-back, see gn_win.hip)
  for (unsigned i = blockIdx.x * kReduceThreads + threadIdx.x;
       i < (unsigned)(kSelRoles * kSelProblems * kSelBins); i += G)
    __hip_atomic_store(&hist[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (blockIdx.x == 0 && threadIdx.x < kSelProblems)
    __hip_atomic_store(&ctl->cand_cnt_pull[0][threadIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  if (!last_block_arrives(&ctl->t[2])) return;
  const int nan_flag = scal->nan_flag, overflow = scal->overflow | (over ? 1 : 0);
  const double med[2] = {scal->median[0], scal->median[1]};
  if (threadIdx.x == 0) __hip_atomic_store(&scal->overflow, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  publish_result(partials, res, seq, sig, med, nan_flag, overflow);
}

// ---------------------------------------------------------------- launchers ------
hipError_t launch_sel_init(icp_handle *h, size_t n) {
  Workspace &w = h->ws;
  hipLaunchKernelGGL(k_sel_init, dim3(64), dim3(256), 0, h->stream, w.d_sel, w.d_scal, w.d_hist, w.d_ctl,
                     (unsigned)n);
  return hipGetLastError();
}

// One selection pipeline: per stage `digits` histogram launches, then C (candidate lists; digits < kSelPasses) or K
// (the full key); `sums`: A behind them.
static hipError_t launch_pull(icp_handle *h, const double *d_a, const double *d_b, size_t n_, const Pose &T, int digits,
                              bool sums) {
  Workspace &w = h->ws;
  const unsigned n = (unsigned)n_;
  const unsigned per = kPullThreads * kPullBatch;
  unsigned hb = (n + per - 1) / per;
  if (hb > 256) hb = 256;  // one workgroup per CU
  const unsigned hb1 = hb / 2 > 0 ? hb / 2 : 1;  // later digits flush dense histograms: fewer, fatter workgroups
  const bool full = digits == kSelPasses;
  const double2 *a = (const double2 *)d_a, *b = (const double2 *)d_b;
  hipStream_t s = h->stream;
  const size_t role = (size_t)kSelProblems * kSelBins;
  // d_hist: roles [3 stage + digit] for digits 0..2 (what A clears), [kSelRoles + 3 stage + digit - 3] for digits 3..5
  // (what the stage's K clears)
  auto H = [&](int stage, int digit) {
    return w.d_hist + (size_t)(digit < 3 ? 3 * stage + digit : kSelRoles + 3 * stage + digit - 3) * role;
  };
  const dim3 bt(kPullThreads);
  SelState *S[2] = {w.d_sel, w.d_sel + kSelProblems};  // ping-pong: a launch never rewrites what it reads
  const unsigned long long *no_cand = nullptr;
  const uint32_t *no_hist = nullptr;
  int cur = 1;  // S[cur] = what the next launch reads, S[cur ^ 1] = what it records
  for (int stage = 0; stage < 2; ++stage) {  // median, MAD (whose first launch turns the median candidates into the median)
    unsigned long long *C = w.d_cand + (size_t)stage * kSelProblems * kSelCap;
    hipLaunchKernelGGL(stage == 0 ? k_pull_hist<0> : k_pull_hist<2>, dim3(hb), bt, 0, s, a, b, T, w.d_rx, w.d_ry, n, 0,
                       (const SelState *)S[cur], S[cur ^ 1], w.d_scal, no_hist, H(stage, 0),
                       stage == 0 ? no_cand : (const unsigned long long *)w.d_cand, w.d_ctl);
    for (int pass = 1; pass < digits; ++pass) {
      hipLaunchKernelGGL(stage == 0 ? k_pull_hist<1> : k_pull_hist<2>, dim3(hb1), bt, 0, s, a, b, T, w.d_rx, w.d_ry, n,
                         pass, (const SelState *)S[cur], S[cur ^ 1], w.d_scal, (const uint32_t *)H(stage, pass - 1),
                         H(stage, pass), no_cand, w.d_ctl);
      cur ^= 1;
    }
    if (full)
      hipLaunchKernelGGL(k_pull_key, dim3(1), bt, 0, s, n, stage, stage == 1 && !sums, (const SelState *)S[cur],
                         S[cur ^ 1], w.d_scal, w.d_hist, C, w.d_ctl);
    else
      hipLaunchKernelGGL(stage == 0 ? k_pull_compact<1> : k_pull_compact<2>, dim3(hb), bt, 0, s, a, b, T, w.d_rx,
                         w.d_ry, n, stage, digits, (const SelState *)S[cur], S[cur ^ 1], w.d_scal,
                         (const uint32_t *)H(stage, digits - 1), C, w.d_ctl);
    cur ^= 1;
  }
  if (sums) {
    int blocks, threads;
    reduce_geometry(n_, &blocks, &threads);
    hipLaunchKernelGGL(k_pull_accumulate, dim3(blocks), dim3(threads), 0, s, a, w.d_rx, w.d_ry, n, T,
                       (const SelState *)S[cur], w.d_scal,
                       (const unsigned long long *)(w.d_cand + (size_t)kSelProblems * kSelCap), w.d_partials, w.d_hist,
                       w.d_ctl, w.h_res, ++w.seq);
  }
  return hipGetLastError();
}

hipError_t launch_weighted_gn_pull(icp_handle *h, const double *d_a, const double *d_b, size_t n, const Pose &T) {
  // two 12-bit digits leave ~1e-4 n keys per prefix; beyond a few million points a third digit
  // keeps the candidate lists short (n <= 2^32)
  constexpr size_t kThreeDigitsFrom = (size_t)4 << 20;
  return launch_pull(h, d_a, d_b, n, T, n > kThreeDigitsFrom ? 3 : 2, true);
}

hipError_t launch_weighted_gn_full(icp_handle *h, const double *d_a, const double *d_b, size_t n, const Pose &T) {
  return launch_pull(h, d_a, d_b, n, T, kSelPasses, true);
}

hipError_t launch_stddevs(icp_handle *h, const double *d_a, const double *d_b, size_t n, const Pose &T) {
  return launch_pull(h, d_a, d_b, n, T, kSelPasses, false);
}

// ------------------------------------------------------------ the plain pass -----
// gauss_newton_update (src/lib.rs:191-216), error (:38-43), huber_error (:45-50)
__global__ __launch_bounds__(kReduceThreads) void k_plain_accumulate(const double2 *__restrict__ a,
                                                          const double2 *__restrict__ b, unsigned n,
                                                          Pose T, double *__restrict__ partials) {
  double acc[kNAcc + 1];
#pragma unroll
  for (int k = 0; k < kNAcc + 1; ++k) acc[k] = 0.;
  const unsigned G = gridDim.x * kReduceThreads;
  for (unsigned i = blockIdx.x * kReduceThreads + threadIdx.x; i < n; i += G) {
    const double2 s = a[i], d = b[i];
    const double r0 = ((T.r00 * s.x + T.r01 * s.y) + T.tx) - d.x;
    const double r1 = ((T.r10 * s.x + T.r11 * s.y) + T.ty) - d.y;
    const double a0 = -s.y, a1 = s.x;
    const double b0 = T.r00 * a0 + T.r01 * a1;
    const double b1 = T.r10 * a0 + T.r11 * a1;
    const double J0[3] = {T.r00, T.r01, b0}, J1[3] = {T.r10, T.r11, b1};
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[9 + k] = acc[9 + k] + (J0[k] * r0 + J1[k] * r1);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[3 * p + q] = acc[3 * p + q] + (J0[p] * J0[q] + J1[p] * J1[q]);
    const double e = r0 * r0 + r1 * r1;
    acc[12] = acc[12] + huber_rho(e);
    acc[13] = acc[13] + e;
  }
  block_reduce_store<kNAcc + 1>(acc, partials + (size_t)blockIdx.x * (kNAcc + 1));
}

// second stage: one block over the block sums; hands the result to the host
__global__ __launch_bounds__(kReduceThreads) void k_final_reduce(const double *__restrict__ partials, int blocks,
                                                      int nacc, const GnScalars *__restrict__ scal,
                                                      GnResult *__restrict__ res) {
  double acc[kNAcc + 1];
#pragma unroll
  for (int k = 0; k < kNAcc + 1; ++k) acc[k] = 0.;
  for (int i = threadIdx.x; i < blocks; i += kReduceThreads)
#pragma unroll
    for (int k = 0; k < kNAcc + 1; ++k)
      if (k < nacc) acc[k] = acc[k] + partials[(size_t)i * (kNAcc + 1) + k];
  block_reduce_store<kNAcc + 1>(acc, res->acc);
  if (threadIdx.x == 0) {
    res->sigma[0] = scal->sigma[0];
    res->sigma[1] = scal->sigma[1];
    res->nan_flag = scal->nan_flag;
    res->overflow = 0;
  }
}

hipError_t launch_plain_gn(icp_handle *h, const double *d_a, const double *d_b, size_t n_, const Pose &T) {
  Workspace &w = h->ws;
  const unsigned n = (unsigned)n_;
  int blocks, threads;
  reduce_geometry(n_, &blocks, &threads);
  hipLaunchKernelGGL(k_plain_accumulate, dim3(blocks), dim3(threads), 0, h->stream, (const double2 *)d_a,
                     (const double2 *)d_b, n, T, w.d_partials);
  hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(kReduceThreads), 0, h->stream, w.d_partials, blocks, kNAcc + 1,
                     w.d_scal, w.h_res);
  return hipGetLastError();
}

}  // namespace icp
