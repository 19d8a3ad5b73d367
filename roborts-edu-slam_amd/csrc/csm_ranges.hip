// csm_ranges.hip — scan endpoints built on the device from raw laser ranges
// (csm_load_ranges / csm_load_ranges_async).
//
// SlamNode::BuildRangeDataContainer (roborts_slam_node.cpp:290-311) keeps beam
// i iff range_min < r_i < range_threshold (:300, compared in double) and makes
// it (cos a_i * r_i, sin a_i * r_i) (:303); RangeDataContainer::CreateFrom
// (sensor_data_manager.h:99-115) scales both by the map's factor (:111). The
// threshold and the per-beam (cos a_i, sin a_i) table come from the host
// (csm_ranges_host.hpp: the running angle sum and glibc's sincos); the device
// repeats the two comparisons and the two separately rounded multiplies per
// coordinate (-ffp-contract=off), so the points equal the host's bit for bit.
//
// Kept beams are compacted in beam order, scans back to back, in three passes:
//   ranges_count_kernel    one wave per scan: kept beams per scan
//   ranges_offsets_kernel  one workgroup: exclusive scan of the counts (int64)
//   ranges_points_kernel   one wave per scan: the keep test again (the ranges
//                          are in L2/MALL), each kept beam's rank among the
//                          wave's 64 from the ballot, one 16-byte store each
// A scan of 1081 beams is 17 chunks of 64 lanes, each chunk one coalesced
// 256-byte read; the stores of a chunk are contiguous (rank order = lane order).
#include <hip/hip_runtime.h>

#include "csm_internal.hpp"

namespace csm {

namespace {

constexpr int kWavesPerBlock = 4;  // scans per 256-thread block
constexpr int kScanChunk = 1024;   // counts per pass of the offsets kernel (one per thread)

// roborts_slam_node.cpp:300
__device__ __forceinline__ bool range_kept(float r, double range_min, double threshold, double* d) {
  *d = (double)r;
  return *d > range_min && *d < threshold;
}

}  // namespace

__global__ __launch_bounds__(256) void ranges_count_kernel(const float* __restrict__ ranges, int32_t n_scans,
                                                           int32_t n_beams, double range_min, double threshold,
                                                           int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int32_t s = (int32_t)blockIdx.x * kWavesPerBlock + (int32_t)(threadIdx.x >> 6);  // the wave's scan
  if (s >= n_scans) return;
  const float* r = ranges + (int64_t)s * n_beams;
  int32_t n = 0;
  for (int64_t b0 = 0; b0 < n_beams; b0 += 64) {  // (64-bit: b0 + 64 may pass INT32_MAX)
    const int64_t i = b0 + lane;
    double d;
    const bool keep = i < n_beams && range_kept(r[i], range_min, threshold, &d);
    n += __popcll(__ballot(keep));
  }
  if (lane == 0) counts[s] = n;
}

// offsets[s] = counts[0] + ... + counts[s - 1], offsets[n_scans] = the total.
__global__ __launch_bounds__(kScanChunk) void ranges_offsets_kernel(const int32_t* __restrict__ counts,
                                                                    int32_t n_scans,
                                                                    int64_t* __restrict__ offsets) {
  __shared__ long long wave_sum[kScanChunk / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  long long carry = 0;  // the chunks before this one
  for (int64_t base = 0; base < n_scans; base += kScanChunk) {
    const int64_t i = base + t;
    const long long v = i < n_scans ? (long long)counts[i] : 0;
    long long x = v;  // inclusive scan within the wave
    for (int o = 1; o < 64; o <<= 1) {
      const long long y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wave_sum[w] = x;
    __syncthreads();
    long long before = 0, total = 0;
    for (int k = 0; k < kScanChunk / 64; ++k) {
      const long long ws = wave_sum[k];
      before += k < w ? ws : 0;
      total += ws;
    }
    if (i < n_scans) offsets[i] = carry + before + (x - v);
    carry += total;
    __syncthreads();  // wave_sum is rewritten by the next chunk
  }
  if (t == 0) offsets[n_scans] = carry;
}

__global__ __launch_bounds__(256) void ranges_points_kernel(const float* __restrict__ ranges, int32_t n_scans,
                                                            int32_t n_beams, double range_min, double threshold,
                                                            double factor, const double2* __restrict__ cos_sin,
                                                            const int64_t* __restrict__ offsets,
                                                            double2* __restrict__ pts) {
  const int lane = threadIdx.x & 63;
  const int32_t s = (int32_t)blockIdx.x * kWavesPerBlock + (int32_t)(threadIdx.x >> 6);
  if (s >= n_scans) return;
  const float* r = ranges + (int64_t)s * n_beams;
  double2* out = pts + offsets[s];
  int32_t base = 0;  // kept beams of the chunks before (wave-uniform)
  for (int64_t b0 = 0; b0 < n_beams; b0 += 64) {  // (64-bit: b0 + 64 may pass INT32_MAX)
    const int64_t i = b0 + lane;
    double d = 0.0;
    const bool keep = i < n_beams && range_kept(r[i], range_min, threshold, &d);
    const unsigned long long m = __ballot(keep);
    if (keep) {
      // kept lanes below this one
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const double2 cs = cos_sin[i];
      const double x = cs.x * d, y = cs.y * d;  // :303
      double2 p;
      p.x = x * factor;                         // sensor_data_manager.h:111
      p.y = y * factor;
      out[base + (int32_t)rank] = p;
    }
    base += __popcll(m);
  }
}

hipError_t launch_ranges_count(const float* ranges, int32_t n_scans, int32_t n_beams, double range_min,
                               double threshold, int32_t* counts, hipStream_t stream) {
  if (n_scans <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n_scans - 1) / kWavesPerBlock + 1);
  hipLaunchKernelGGL(ranges_count_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, stream, ranges, n_scans,
                     n_beams, range_min, threshold, counts);
  return hipGetLastError();
}

hipError_t launch_ranges_offsets(const int32_t* counts, int32_t n_scans, int64_t* offsets, hipStream_t stream) {
  hipLaunchKernelGGL(ranges_offsets_kernel, dim3(1), dim3(kScanChunk), 0, stream, counts, n_scans, offsets);
  return hipGetLastError();
}

hipError_t launch_ranges_points(const float* ranges, int32_t n_scans, int32_t n_beams, double range_min,
                                double threshold, double factor, const double* cos_sin, const int64_t* offsets,
                                double* pts, hipStream_t stream) {
  if (n_scans <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n_scans - 1) / kWavesPerBlock + 1);
  hipLaunchKernelGGL(ranges_points_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, stream, ranges, n_scans,
                     n_beams, range_min, threshold, factor, reinterpret_cast<const double2*>(cos_sin), offsets,
                     reinterpret_cast<double2*>(pts));
  return hipGetLastError();
}

}  // namespace csm
