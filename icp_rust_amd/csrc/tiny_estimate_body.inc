// The body of the one-workgroup registration (Icp{2,3}d::estimate of up to 1024 source / 2048 target points), textually
// included by both kernels that run it -- k_tiny_estimate (one problem per launch) and k_tiny_estimate_batch (one problem
// per workgroup), gn_fast.hip -- so that the two cannot drift apart and the single kernel compiles exactly as it did when
// the body was written inline.  The including function has in scope, under these names:
//   DIM, B                 template parameters (dimension; threads per workgroup, a multiple of 64)
//   src, n                 the source points (DIM doubles each) and their count, 1 <= n <= B
//   dst, m                 the target points and their count, 1 <= m <= 2048
//   T0, max_iter           initial pose, outer iterations (>= 1)
//   cx, cy, cz, scale      centre of the targets' box, and a bound at least build_grid's GridParams::scale (the f32
//                          screen's margin; a larger bound only sends more candidates to the exact f64 test)
//   res, inner_out, idx_out  the result (thread 0), inner counts (max_iter entries, nullable), indices (n, nullable)
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
  p += sizeof(unsigned long long) * 2 * 2 * 1024;
  TinySel *S = reinterpret_cast<TinySel *>(p);
  p += (sizeof(TinySel) + 15) & ~size_t(15);
  double(*sm)[kNSum + 1] = reinterpret_cast<double(*)[kNSum + 1]>(p);
  p += sizeof(double) * 16 * (kNSum + 1);
  double(*part)[kNSum + 1] = reinterpret_cast<double(*)[kNSum + 1]>(p);
  p += sizeof(double) * 2 * (kNSum + 1);
  struct Ctl {
    Pose Ti, T;
    double s_mad[2][2];
    int done, nan, bail, fixed;
    unsigned applied, evals, sorted;
  };
  Ctl *C = reinterpret_cast<Ctl *>(p);

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
  // Targets sorted by x (once per call): keys = (order-preserving bits of fl32(x - cx), index), bitonic
  // sort of the next power of two in LDS.  A sweep then visits only targets whose x lies within the
  // current best distance of the query's -- a few of them instead of all m (sweep and prune; exact:
  // a target with |dx| > sqrt(best) is strictly farther).
  {
    unsigned long long *keys = &sbuf[0][0][0];  // 4096 slots: room for 2048 keys
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
        for (unsigned t = tid; t < (P >> 1); t += B) {
          const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
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
        tx[j] = x;
        ty[j] = y;
        if (DIM == 3) tz[j] = z;
        g4[j] = make_float4((float)(x - cx), (float)(y - cy), DIM == 3 ? (float)(z - cz) : 0.f, __uint_as_float(k));
      } else {  // pads: beyond every bound
        g4[j] = make_float4(__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf(), __uint_as_float(0xffffffffu));
      }
    }
    __syncthreads();
  }
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
  const int blocks = n > 512u ? 2 : 1;  // reduce_geometry(n) for n <= 1024: 512-thread blocks
  const unsigned lo_rank = (n - 1) / 2, hi_rank = n / 2;
  unsigned bi = 0xffffffffu;
  TINY_STAMP(0);
  for (unsigned it = 0; it < max_iter; ++it) {
    const Pose T = C->T;
    // ---- transform + exact nearest neighbour (src/lib.rs:113-124 / 156-167) ----
    double ax = 0., ay = 0., bx = 0., by = 0.;
    if (has) {
      const double qx = (T.r00 * px + T.r01 * py) + T.tx;  // Transform::transform, src/transform.rs:22-24
      const double qy = (T.r10 * px + T.r11 * py) + T.ty;
      const double qz = pz;
      const double ox = qx - cx, oy = qy - cy, oz = DIM == 3 ? qz - cz : 0.;
      const float hx = (float)ox, hy = (float)oy, hz = (float)oz;
      const double ec = (fmax(fmax(fabs(ox), fabs(oy)), fabs(oz)) + 2. * scale) * 1.2e-7 * 1.7320508075688774;
      double best = __builtin_huge_val();
      float thr = __builtin_huge_valf();
      unsigned nb = 0xffffffffu, nbo = 0xffffffffu;  // sorted position / original index of the best so far
      auto exact = [&](unsigned j, unsigned orig) {
        const double dx = qx - tx[j], dy = qy - ty[j];
        double d = dx * dx + dy * dy;
        if (DIM == 3) {
          const double dz = qz - tz[j];
          d = d + dz * dz;
        }
        if (d < best || (d == best && orig < nbo)) {  // ties -> lowest ORIGINAL index
          best = d;
          nb = j;
          nbo = orig;
          const double rr = sqrt(d) + ec;
          thr = (float)(rr * rr * 1.000004) * 1.000001f + 1e-37f;  // rounded up (nn_brute.hip)
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
      if (idx_out && it + 1 == max_iter) idx_out[tid] = nbo;
    }
    // ---- estimate_transform, src/lib.rs:59-84 ----
    if (tid == 0) {
      C->Ti = transform_identity();
      C->done = n < 2u ? 1 : 0;  // check_input_size, src/lib.rs:186-189
      C->applied = 0;
    }
    double prev_error = 1.7976931348623157e308;  // f64::MAX (thread 0 only)
    __syncthreads();
    TINY_STAMP(1);
    for (int k = 0; k < ICP_INNER_MAX_ITER && !C->done; ++k) {
      const Pose Ti = C->Ti;
      double r0 = 0., r1 = 0.;
      if (has) {  // residual(), src/lib.rs:34-36
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
      const unsigned long long km0 = has ? f2k(r0) : ~0ull, km1 = has ? f2k(r1) : ~0ull;
      bool ok = tiny_select_window<B>(km0, km1, has, n, S, 0, selp) || tiny_select<B>(km0, km1, has, n, S, sbuf[0], selp, 0);
      if (ok) {
        med[0] = middle_of_host(n, S->out[0][0], S->out[0][1]);
        med[1] = middle_of_host(n, S->out[1][0], S->out[1][1]);
        // (S->out is next written behind the first barriers of the next selection)
        const unsigned long long kd0 = has ? f2k(fabs(r0 - med[0])) : ~0ull, kd1 = has ? f2k(fabs(r1 - med[1])) : ~0ull;
        ok = tiny_select_window<B>(kd0, kd1, has, n, S, 1, selp) || tiny_select<B>(kd0, kd1, has, n, S, sbuf[0], selp, 1);
        if (ok) {
          sig[0] = ICP_PPF34 * middle_of_host(n, S->out[0][0], S->out[0][1]);
          sig[1] = ICP_PPF34 * middle_of_host(n, S->out[1][0], S->out[1][1]);
        }
      }
      if (!ok) {  // (uniform: every thread saw the same list counts)
        if constexpr (B == 1024) {  // the sorting path of k_tiny_eval
          unsigned long long ka = has ? f2k(r0) : ~0ull, kb = has ? f2k(r1) : ~0ull;
          __syncthreads();
          bitonic_sort2_1024(ka, kb, sbuf);
          __syncthreads();
          sbuf[0][0][tid] = ka;
          sbuf[0][1][tid] = kb;
          __syncthreads();
          const double xl = k2f(sbuf[0][0][lo_rank]), xh = k2f(sbuf[0][0][hi_rank]);
          const double yl = k2f(sbuf[0][1][lo_rank]), yh = k2f(sbuf[0][1][hi_rank]);
          med[0] = (n & 1) ? xl : (xl + xh) / 2.;
          med[1] = (n & 1) ? yl : (yl + yh) / 2.;
          mad_ranks(sbuf[0][0], n, med[0], lo_rank, hi_rank, C->s_mad[0]);
          mad_ranks(sbuf[0][1], n, med[1], lo_rank, hi_rank, C->s_mad[1]);
          __syncthreads();
          sig[0] = ICP_PPF34 * ((n & 1) ? C->s_mad[0][0] : (C->s_mad[0][0] + C->s_mad[0][1]) / 2.);
          sig[1] = ICP_PPF34 * ((n & 1) ? C->s_mad[1][0] : (C->s_mad[1][0] + C->s_mad[1][1]) / 2.);
          if (tid == 0) ++C->sorted;
        } else {  // the sort is written for 1024 threads: hand the call back, the host-driven path serves
          med[0] = med[1] = sig[0] = sig[1] = 0.;
          if (tid == 0) C->bail = 1;
        }
      }
      TINY_STAMP(2);
      // weighted normal equations + Huber error (src/lib.rs:238-255, 45-50), one point per thread
      // the tree of reduce_geometry(n), exactly as k_tiny_eval folds it -- one dimension's sums at a time (half
      // the registers of all nineteen at once; the wave trees of different sums are independent)
      if ((unsigned)wave * 64u < n) {
        static_assert(kNSum == 19, "9 + 9 + 1");
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          double half[10];
#pragma unroll
          for (int q = 0; q < 10; ++q) half[q] = 0.;
          if (has) {
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
      if (tid == 0) {
        const double *tot = sm[1];
        ++C->evals;
        double delta[3];
        if (C->nan | C->bail) {
          C->done = 1;
        } else if (!solve_update(tot, tot + 9, delta)) {
          C->done = 1;  // None, src/lib.rs:67-69
        } else if ((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2] < ICP_DELTA_NORM_THRESHOLD) {
          C->done = 1;  // src/lib.rs:71-73
        } else if (tot[12] > prev_error) {
          C->done = 1;  // src/lib.rs:75-78
        } else {
          prev_error = tot[12];
          bool in_range;
          const Pose D = transform_new_in_range(delta, &in_range);
          if (!in_range) {
            C->bail = 1;  // a rotation beyond the restated range of sin / cos: the host-driven path serves
            C->done = 1;
          } else {
            C->Ti = transform_mul(D, Ti);  // src/lib.rs:81
            ++C->applied;
          }
        }
      }
      __syncthreads();
      TINY_STAMP(4);
    }
    if (tid == 0) {
      if (inner_out) inner_out[it] = C->applied;
      C->T = transform_mul(C->Ti, T);  // src/lib.rs:127, 170
      // An outer iteration that leaves the pose as it found it, bit for bit, is a fixed point of the loop: every
      // later iteration repeats it (correspondences and updates are functions of the pose and the two clouds).  Only
      // the last one still runs -- it is the one that reports the correspondences.
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
    res->sorted = C->sorted;
    res->status = C->nan ? 3 : (C->bail ? -1 : 0);
#ifdef ICP_TINY_PROFILE
    tp[5] = __builtin_amdgcn_s_memtime() - t_begin;
    for (int q = 0; q < 6; ++q) res->t[q] = tp[q];
    for (int q = 0; q < 8; ++q) res->ts[q] = tsel[q];
#endif
  }
#undef TINY_STAMP
