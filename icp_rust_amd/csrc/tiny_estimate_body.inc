// The body of the one-workgroup registration (Icp{2,3}d::estimate of up to 1024 source / 2048 target points), textually
// included by the kernels that run it -- k_tiny_estimate (one problem per launch), k_tiny_estimate_batch and
// k_tiny_estimate_gated_batch (one problem per workgroup), gn_fast.hip -- so that they cannot drift apart.  The pieces
// k_line_estimate_batch (p2line_batch.hip) runs too are functions of tiny_device.hpp.  The including function has in
// scope, under these names:
//   DIM, B                 template parameters (dimension; threads per workgroup, a multiple of 64)
//   src, n                 the source points (DIM doubles each) and their count, 1 <= n <= B
//   dst, m                 the target points and their count, 1 <= m <= 2048
//   T0, max_iter           initial pose, outer iterations (>= 1)
//   cx, cy, cz, scale      centre of the targets' box, and a bound at least build_grid's GridParams::scale (the f32
//                          screen's margin; a larger bound only sends more candidates to the exact f64 test)
//   res, inner_out, idx_out  the result (thread 0), inner counts (max_iter entries, nullable), indices (n, nullable)
//   GATED, r2, inl_out     constexpr bool: the gate of icp_estimate_gated (include/icp_mi355x.h section 10) between the
//                          search and the inner loop; then the squared bound and where the pairs kept per outer
//                          iteration go (max_iter entries, nullable).  Not GATED: neither is read
// and dynamic LDS of tiny_lds_bytes(DIM, m).  Not a header: no include guard, included inside a function body.
  extern __shared__ unsigned char lds_raw[];
  // ---- LDS carve-up ----  (targets are kept SORTED BY x: position j below is not the target's index)
  const unsigned mp = (m + 63u) & ~63u;
  double *tx = reinterpret_cast<double *>(lds_raw);
  double *ty = tx + mp;
  double *tz = ty + mp;  // (DIM == 2: unused, zero length below)
  unsigned char *p = reinterpret_cast<unsigned char *>(tz + (DIM == 3 ? mp : 0));
  float4 *g4 = reinterpret_cast<float4 *>(p);  // {x, y, z relative to the box centre as f32, original index}
  p += sizeof(float4) * (mp + 4);
  unsigned long long(*sbuf)[2][1024] = reinterpret_cast<unsigned long long(*)[2][1024]>(p);  // sorting path
  // (GATED: an outer iteration's kept pairs pass through the same bytes, between its search and its first selection)
  const TinyGate<B> gate(p);
  p += sizeof(unsigned long long) * 2 * 2 * 1024;
  TinySel *S = reinterpret_cast<TinySel *>(p);
  p += (sizeof(TinySel) + 15) & ~size_t(15);
  double(*sm)[kNSum + 1] = reinterpret_cast<double(*)[kNSum + 1]>(p);
  p += sizeof(double) * 16 * (kNSum + 1);
  double(*part)[kNSum + 1] = reinterpret_cast<double(*)[kNSum + 1]>(p);
  p += sizeof(double) * 2 * (kNSum + 1);
  struct Ctl : TinyCtl {
    double s_mad[2][2];
    unsigned sorted;
  };
  Ctl *C = reinterpret_cast<Ctl *>(p);
  const TinyTargets tg = {tx, ty, tz, g4, m};

  const unsigned tid = threadIdx.x;
  const int wave = tid >> 6;
  const bool has = tid < n;
#ifdef ICP_TINY_PROFILE
  unsigned long long tp[6] = {0, 0, 0, 0, 0, 0}, t_last = __builtin_amdgcn_s_memtime();
  unsigned long long tsel[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long t_begin = t_last;
#define TINY_STAMP(slot)                                         \
  do {                                                           \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    tp[slot] += now_ - t_last;                                   \
    t_last = now_;                                               \
  } while (0)
#else
#define TINY_STAMP(slot) ((void)0)
#endif
  // (the sorting path's buffers hold the target sort's keys meanwhile: 4096 slots, room for 2048 keys)
  tiny_sort_targets<DIM, B>(dst, cx, cy, cz, &sbuf[0][0][0], tg, [](unsigned, unsigned, double, double) {});
  double px = 0., py = 0., pz = 0.;
  if (has) {
    px = src[(size_t)tid * DIM];
    py = src[(size_t)tid * DIM + 1];
    if (DIM == 3) pz = src[(size_t)tid * DIM + 2];
  }
  if (tid == 0) {
    C->T = T0;
    C->nan = C->bail = 0;
    C->evals = C->sorted = 0;
    S->wvalid[0] = S->wvalid[1] = 0u;  // (no window yet: the first selections sample)
  }
  if (tid >= B / 64 && tid < 16) {  // the wave sums of the waves a smaller workgroup does not have
#pragma unroll
    for (int q = 0; q < kNSum + 1; ++q) sm[tid][q] = 0.;
  }

  __syncthreads();
  // the pairs the inner loop sees: all n, thread t its own; GATED: the kept ones, thread t the t-th of them
  unsigned cnt = n;
  bool hasp = has;
  int blocks = n > 512u ? 2 : 1;  // reduce_geometry(cnt) for cnt <= 1024: 512-thread blocks
  unsigned bi = 0xffffffffu;
  TINY_STAMP(0);
  for (unsigned it = 0; it < max_iter; ++it) {
    const Pose T = C->T;
    // ---- transform + exact nearest neighbour (src/lib.rs:113-124 / 156-167) ----
    double ax = 0., ay = 0., bx = 0., by = 0.;
    bool in = false;  // (GATED) the pair passes the gate
    if (has) {
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      const double qz = pz;
      unsigned nb, nbo;  // sorted position / original index of the nearest target
      tiny_nearest<DIM>(tg, qx, qy, qz, cx, cy, cz, scale, bi, &nb, &nbo);
      bi = nb;
      ax = qx;
      ay = qy;
      if (nb != 0xffffffffu) {
        bx = tx[nb];
        by = ty[nb];
      } else {  // no finite distance (NaN query): index 0, as a scan from 0 would
        bx = dst[0];
        by = dst[1];
        nbo = 0;
      }
      if constexpr (GATED) {  // k_gate_stage's expressions (gate.hip)
        const double ex = qx - bx, ey = qy - by;
        double d2 = ex * ex + ey * ey;
        if (DIM == 3) {
          const double ez = qz - (nb != 0xffffffffu ? tz[nb] : dst[2]);
          d2 = d2 + ez * ez;
        }
        in = d2 <= r2;  // (false for a NaN d2: a NaN query, paired with index 0 above, is dropped)
      }
      if (idx_out && it + 1 == max_iter) idx_out[tid] = nbo;
    }
    if constexpr (GATED) {
      // ---- the gate: the kept pairs in thread order (stable), pair t to thread t ----
      // rank = kept lanes before this one in its wave + the counts of the waves before it; the kept lanes of a wave
      // write consecutive records.  The warm start `bi` and the reported index stay with the source thread.
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
      // A kept pair's bi (= nb) is a sorted position, never 0xffffffff.  tiny_nearest answers 0xffffffff only where the
      // query's d is NaN against every target -- against dst[0] too, so the d2 formed above with dst[0] is NaN and `in`
      // is false.  An infinite query is no such case: its d is +inf against every target and the `d == best` branch
      // gives it a position.  Should a pair without a position ever be kept all the same, the bound of the read below
      // sends it to position 0 instead of outside the targets.
      if (in) {
        gate.qx[rank] = ax;
        gate.qy[rank] = ay;
        gate.nb[rank] = bi;
      }
      cnt = (unsigned)__builtin_amdgcn_readfirstlane((int)kept);  // (the same in every thread)
      hasp = tid < cnt;
      blocks = cnt > 512u ? 2 : 1;
      __syncthreads();
      ax = ay = bx = by = 0.;
      if (hasp) {
        unsigned g = gate.nb[tid];
        g = g < m ? g : 0u;  // (always < m: above)
        ax = gate.qx[tid];
        ay = gate.qy[tid];
        bx = tx[g];
        by = ty[g];
      }
      // (the barrier below: every record is read before the first selection writes its keys over them)
    }
    // ---- estimate_transform, src/lib.rs:59-84 ----
    if (tid == 0) {
      C->Ti = transform_identity();
      C->done = cnt < 2u ? 1 : 0;  // check_input_size, src/lib.rs:186-189
      C->applied = 0;
      C->prev_error = 1.7976931348623157e308;  // f64::MAX
    }
    __syncthreads();
    TINY_STAMP(1);
    for (int k = 0; k < ICP_INNER_MAX_ITER && !C->done; ++k) {
      const Pose Ti = C->Ti;
      double r0 = 0., r1 = 0.;
      if (hasp) {  // residual(), src/lib.rs:34-36
        r0 = ((Ti.r00 * ax + Ti.r01 * ay) + Ti.tx) - bx;
        r1 = ((Ti.r10 * ax + Ti.r11 * ay) + Ti.ty) - by;
        if ((r0 != r0) | (r1 != r1)) C->nan = 1;
      }
      double med[2], sig[2];
      // medians, then MADs (src/stats.rs:11-47)
#ifdef ICP_TINY_PROFILE
      unsigned long long *selp = tsel;
#else
      unsigned long long *selp = nullptr;
#endif
      const unsigned long long km0 = hasp ? f2k(r0) : ~0ull, km1 = hasp ? f2k(r1) : ~0ull;
      bool ok = tiny_select_window<B>(km0, km1, hasp, cnt, S, 0, selp) || tiny_select<B>(km0, km1, hasp, cnt, S, sbuf[0], selp, 0);
      if (ok) {
        med[0] = middle_of_host(cnt, S->out[0][0], S->out[0][1]);
        med[1] = middle_of_host(cnt, S->out[1][0], S->out[1][1]);
        // (S->out is next written behind the first barriers of the next selection)
        const unsigned long long kd0 = hasp ? f2k(fabs(r0 - med[0])) : ~0ull, kd1 = hasp ? f2k(fabs(r1 - med[1])) : ~0ull;
        ok = tiny_select_window<B>(kd0, kd1, hasp, cnt, S, 1, selp) || tiny_select<B>(kd0, kd1, hasp, cnt, S, sbuf[0], selp, 1);
        if (ok) {
          sig[0] = ICP_PPF34 * middle_of_host(cnt, S->out[0][0], S->out[0][1]);
          sig[1] = ICP_PPF34 * middle_of_host(cnt, S->out[1][0], S->out[1][1]);
        }
      }
      if (!ok) {  // (uniform: every thread saw the same list counts)
        if constexpr (B == 1024) {  // the sorting path of k_tiny_eval
          unsigned long long key[2] = {hasp ? f2k(r0) : ~0ull, hasp ? f2k(r1) : ~0ull};
          __syncthreads();
          tiny_bitonic_sort<1024, 2>(key, sbuf);
          __syncthreads();
          tiny_sorted_median_sigma<1024, 2>(key, sbuf[0], cnt, C->s_mad, med, sig);
          if (tid == 0) ++C->sorted;
        } else {  // the sorting path runs at 1024 threads only: hand the call back, the host-driven path serves
          med[0] = med[1] = sig[0] = sig[1] = 0.;
          if (tid == 0) C->bail = 1;
        }
      }
      TINY_STAMP(2);
      // weighted normal equations + Huber error (src/lib.rs:238-255, 45-50), one point per thread
      // the tree of reduce_geometry(cnt), exactly as k_tiny_eval folds it -- one dimension's sums at a time (half
      // the registers of all nineteen at once; the wave trees of different sums are independent)
      if ((unsigned)wave * 64u < cnt) {
        static_assert(kNSum == 19, "9 + 9 + 1");
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          double half[10];
#pragma unroll
          for (int q = 0; q < 10; ++q) half[q] = 0.;
          if (hasp) {
            accumulate_dim<false>(j, make_double2(ax, ay), j ? r1 : r0, Ti, half);
            if (j == 0) accumulate_rho<false>(r0, r1, &half[9]);
          }
          wave_tree<10>(half);
          if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 9; ++q) sm[wave][9 * j + q] = half[q];
            sm[wave][18 + j] = half[9];  // (the error; the pad sums to +0.0)
          }
        }
      } else if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kNSum + 1; ++q) sm[wave][q] = 0.;
      }
      __syncthreads();
      if (tid < 2 * (kNSum + 1)) {
        const int vb = tid / (kNSum + 1), q = tid % (kNSum + 1);
        double v = sm[8 * vb][q];
        for (int w = 1; w < 8; ++w) v = v + sm[8 * vb + w][q];
        part[vb][q] = v;
      }
      __syncthreads();
      TINY_STAMP(3);
      // the last level of the tree and g_x S_x + g_y S_y, one thread per entry (rows 0 and 1 of `sm` are free until
      // the next evaluation's wave sums; thread 0 alone with arrays in scratch memory cost 2.7 us per evaluation)
      if (tid < kNSum) {
        const double p0 = (0. + part[0][tid]) + 0.;
        const double p1 = blocks > 1 ? (0. + part[1][tid]) + 0. : 0.;
        sm[0][tid] = (p0 + p1) + 0.;
      }
      __syncthreads();
      if (tid < kNAcc) sm[1][tid] = combine_sum(sm[0], (int)tid, sig);
      __syncthreads();
      if (tid == 0) tiny_inner_decide(C, sm[1]);
      __syncthreads();
      TINY_STAMP(4);
    }
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
    res->sorted = C->sorted;
    res->status = C->nan ? 3 : (C->bail ? -1 : 0);
#ifdef ICP_TINY_PROFILE
    tp[5] = __builtin_amdgcn_s_memtime() - t_begin;
    for (int q = 0; q < 6; ++q) res->t[q] = tp[q];
    for (int q = 0; q < 8; ++q) res->ts[q] = tsel[q];
#endif
  }
#undef TINY_STAMP
