// csm_score_sink.hpp — what every scoring kernel does with a candidate once
// its beams are summed: the fixed-point sum as the reference's fp64 sum, and
// where the penalised score goes. The kernels differ in how a lane enumerates
// its candidates and in which LDS is free for the fused finish; the rest is
// stated here once.
#pragma once

#include <hip/hip_runtime.h>

#include "csm_device.hpp"
#include "csm_tail.hpp"

namespace csm {
namespace dev {

// The reference's sequential fp64 sum of n_used cells from their exact
// fixed-point sum: gridi holds (value - outside) * 2^E, so outside comes back
// n_used times before the scale 2^-E.
__device__ __forceinline__ double fixed_point_acc(const LevelWork& L, int64_t sum, int32_t n_used) {
  return (double)(sum + (int64_t)n_used * L.outside_i) * L.int_scale;
}

// The wave's best (score, lowest flat index among equals), left in lane 0.
__device__ __forceinline__ void wave_best(double& bs, int64_t& bf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_down(bs, o, 64);
    const int64_t of = __shfl_down(bf, o, 64);
    if (better(os, of, bs, bf)) {
      bs = os;
      bf = of;
    }
  }
}

// A lane's scores on their way out. BEST: the lane's best candidate, then the
// wave's as one BestPartial. Otherwise every score is stored and the lane keeps
// what the fused finish (csm_tail.hpp) asks of it: its max and whether any
// score was NaN.
template <bool BEST>
struct ScoreSink {
  double bs = -1.0e300;
  int64_t bf = INT64_MAX;
  double lmax = -INFINITY;
  bool lnan = false;

  // Candidate `flat` of window S scored `score`.
  __device__ __forceinline__ void add(const LevelWork& L, const ScanWork& S, double* __restrict__ out, int64_t flat,
                                      double score) {
    if constexpr (BEST) {
      if (better(score, flat, bs, bf)) {
        bs = score;
        bf = flat;
      }
    } else {
      tail::store_score(L, out + S.out_off + flat, score);
      lnan |= score != score;
      lmax = (score > lmax) ? score : lmax;
    }
  }

  // Every candidate of the wave is in (all lanes of the wave call this).
  // BEST: lane 0 writes the wave's best to *slot. Otherwise, in a launch that
  // finishes its windows (L.tail.on: one wave per (window, angle a)), the fused
  // finish with ldsA / ldsB, tail::kBytesA / kBytesB of LDS the kernel no
  // longer reads. The fallback kernels (csm_kernels.hip) never run with
  // tail.on: in all mode their stores are the end and they do not call this
  // (the finisher inlined behind a flag that is never set cost them registers
  // and, six of them, an occupancy step).
  __device__ __forceinline__ void done(const LevelWork& L, const ScanWork& S, const AngleEntry* __restrict__ angles,
                                       const double* __restrict__ out, int a, BestPartial* slot, char* ldsA,
                                       char* ldsB) {
    if constexpr (BEST) {
      wave_best(bs, bf);
      if ((threadIdx.x & 63) == 0) *slot = BestPartial{bs, bf};
    } else {
      if (L.tail.on) tail::finish(L, S, angles, out, a, lmax, lnan, ldsA, ldsB);
    }
  }
};

}  // namespace dev
}  // namespace csm
