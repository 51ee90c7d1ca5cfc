// What the one-workgroup estimators with a normal-based residual share (p2line_batch.hip: k_line_estimate_batch,
// k_line_estimate_gated_batch; p2plane_batch.hip: k_plane_estimate_batch, k_plane_estimate_gated_batch; their body is
// normal_batch_device.hpp: normal_estimate_item): the inner loop on the pairs of one outer
// iteration -- api_normal.hip: p2pl_loop_on_pairs, with k_p2pl_accumulate's statement -- ONE copy, so that the line and the
// plane residual cannot drift apart.  A line pair is a plane pair with nz = dz = +0.0.
#pragma once
#include "common.hpp"
#include "gn_device.hpp"
#include "p2plane_device.hpp"
#include "tiny_device.hpp"

namespace icp {

constexpr int kPairSums = kNAcc;  // jtj[9], jtr[3], huber error: what k_p2pl_accumulate folds

struct PairCtl : TinyCtl {
  double mad[1][2];
  unsigned pos0;  // the sorted position of the target of original index 0
};

// p2pl_loop_on_pairs on the cnt pairs of the workgroup, thread t the t-th of them (hasp = t < cnt; pr: its pair),
// summed in the tree of reduce_geometry(cnt): blocks = 1 or 2 blocks of 512.  Every thread of the workgroup calls it.
// load_pair() runs behind the loop's first barrier, for a caller whose pairs wait in LDS (the gate).  On return C->Ti is
// the loop's pose and C->applied the updates applied (thread 0's writes, behind a barrier where the loop ran at all).
//   sbuf  LDS, [3][1][B]: two sort buffers, then the sorted keys
//   sm    LDS, [16][kPairSums]: the wave sums (those of the waves a 512-thread workgroup does not have stay +0.0)
//   tot   LDS, [16]
template <unsigned B, class LoadPair>
__device__ __forceinline__ void tiny_pair_loop(PlanePair &pr, bool hasp, unsigned cnt, int blocks, PairCtl *C,
                                               unsigned long long (*sbuf)[1][B], double (*sm)[kPairSums], double *tot,
                                               LoadPair load_pair) {
  const unsigned tid = threadIdx.x;
  const int wave = tid >> 6;
  if (tid == 0) {
    C->Ti = transform_identity();
    C->done = cnt < 2u ? 1 : 0;  // fewer than two pairs: the identity, no update
    C->applied = 0;
    C->prev_error = 1.7976931348623157e308;  // DBL_MAX
  }
  __syncthreads();
  load_pair();
  for (int k = 0; k < ICP_INNER_MAX_ITER && !C->done; ++k) {
    const Pose Ti = C->Ti;
    double r = 0.;
    if (hasp) {
      r = plane_residual(pr, Ti);
      if (r != r) C->nan = 1;
    }
    // exact median and MAD of r (launch_stddevs on ((r, 0), (0, 0)) under the identity: dimension 0's statistics of
    // ((1 r + 0 0) + 0) - 0 = r, which plane_residual's trailing + nz dz = + 0.0 has already rid of a -0.0 for a line
    // pair; a plane pair's r can be -0.0 where that statistic is +0.0: only the sign of a zero median can differ, and
    // |r - med|, sigma and every sum below are the same numbers)
    unsigned long long key[1] = {hasp ? f2k(r) : ~0ull};
    double med[1], sig[1];
    tiny_bitonic_sort<B, 1>(key, sbuf);
    tiny_sorted_median_sigma<B, 1>(key, sbuf[2], cnt, C->mad, med, sig);  // (a third buffer: no barrier behind the sort)
    const double sigma = sig[0];
    // k_p2pl_accumulate's terms, one pair per thread, folded as block_reduce_store folds a 512-thread block
    {
      double acc[kPairSums];
#pragma unroll
      for (int q = 0; q < kPairSums; ++q) acc[q] = 0.;
      if (hasp) {
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
      wave_tree<kPairSums>(acc);
      if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kPairSums; ++q) sm[wave][q] = acc[q];
      }
    }
    __syncthreads();
    // the blocks' left folds of their eight wave sums, then k_final_reduce over the block sums: thread b of its one
    // 512-thread block holds 0 + sum_b, every other lane and wave +0.0, so its tree leaves (0 + sum_0) + (0 + sum_1)
    if (tid < (unsigned)kPairSums) {
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
    if (tid == 0) tiny_inner_decide(C, tot);
    __syncthreads();
  }
}

}  // namespace icp
