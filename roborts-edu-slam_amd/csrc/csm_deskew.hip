// csm_deskew.hip — motion de-skew of raw laser scans on the device
// (csm_load_ranges_deskewed*), in front of the ranges ingest (csm_ranges.hip).
//
// LaserDataProcessor::Process (laser_data_processor.cpp:43-120) re-projects
// every beam through the odometry poses interpolated over the scan time
// (BeamsUpdate :231-314, Transform2d util/transform.h:52-103) and re-bins the
// beams into the message (:109-116). The host (csm_deskew.cpp) hands over each
// segment's interpolation and each scan's base transform (their divisions and
// the base's sincos are done once there), the per-beam (cos, sin) of the
// float-arithmetic beam angles, and the interior closing beams whole: those are
// transformed twice, the second time from the exact atan2 of the first, and
// the device library's atan2 is not the host libm's bit for bit.
//
// Every other beam is one lane's work: the two products, the mid frame (three
// multiply-adds, separately rounded: -ffp-contract=off), glibc's sincos
// restated (libm_sincos.hpp) of the mid yaw, the two transforms with their
// identity branches (csm_deskew_host.hpp, shared with the host), a correctly
// rounded sqrt, and D = atan2 with the bin quotient q = (D - angle_min) /
// angle_increment. Everything but D equals the host's bits; D is within 2^-44
// of the host's (tests/test_gpu_deskew.py measures it), which moves q by less
// than 2^-30 under the queue-time bounds (|angle_increment| >= 2^-12,
// |angle_min| <= 8, n_beams <= 8000). So trunc(q) is the host's unless q lies within 2^-30 of a nonzero
// integer (zero is no boundary of a truncation toward zero) or is not finite:
// such a beam flags its scan, and the host de-skews that scan when the batch
// is taken.
//
// One 256-thread workgroup per scan. Process writes out[j] = range_i for i
// ascending, so the last beam of a bin wins: each beam does a 64-bit LDS
// atomicMax of ((i + 1) << 32 | float bits) into slot j, and the winners (or
// 0) are written out coalesced. The two undefined behaviours of the reference
// (j >= n_beams, a quotient of magnitude >= 2^31 or not finite) drop the beam,
// as on the host.
#include <hip/hip_runtime.h>

#include "csm_deskew_host.hpp"
#include "csm_internal.hpp"
#include "libm_sincos.hpp"

namespace csm {

namespace {

constexpr int kDeskewThreads = 256;
constexpr double kBinGuard = 9.31322574615478515625e-10;  // 2^-30

}  // namespace

__global__ __launch_bounds__(kDeskewThreads) void deskew_kernel(
    const float* __restrict__ raw, int32_t n_scans, int32_t n_beams, float angle_min, float angle_increment,
    const DeskewScan* __restrict__ scans, const DeskewSeg* __restrict__ segs, const double2* __restrict__ beam_cs,
    const double* __restrict__ trig_tab, float* __restrict__ out, int32_t* __restrict__ flags) {
  // n_beams bin slots, then the scan's flag (all LDS in the dynamic region: its base stays 8-byte aligned)
  extern __shared__ __attribute__((aligned(16))) unsigned long long slots[];
  const int32_t s = (int32_t)blockIdx.x;
  const DeskewScan sc = scans[s];
  const float* in = raw + (int64_t)s * n_beams;
  float* o = out + (int64_t)s * n_beams;
  if (sc.n_seg == 0) {  // Process :104 false: the message goes on as it came
    for (int32_t i = (int32_t)threadIdx.x; i < n_beams; i += kDeskewThreads) o[i] = in[i];
    return;
  }
  for (int32_t i = (int32_t)threadIdx.x; i < n_beams; i += kDeskewThreads) slots[i] = 0ull;
  if (threadIdx.x == 0) slots[n_beams] = 0ull;
  __syncthreads();
  const DeskewSeg* sg = segs + sc.seg_off;
  const deskew::T2 base{sc.r00, sc.r01, sc.r10, sc.r11, sc.tx, sc.ty};
  const double amin = (double)angle_min, inc = (double)angle_increment;
  bool flagged = false;
  for (int32_t i = (int32_t)threadIdx.x; i < n_beams; i += kDeskewThreads) {
    // beam i's segment: the first whose closing beam is not below i
    int32_t lo = 0, hi = sc.n_seg - 1;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (sg[mid].first + sg[mid].cnt - 1 >= i)
        hi = mid;
      else
        lo = mid + 1;
    }
    const DeskewSeg g = sg[lo];
    int32_t j = -1;
    float rf = 0.0f;
    if (i == g.first + g.cnt - 1 && g.host_bin != -2) {  // an interior closing beam: the host's
      j = g.host_bin;
      rf = g.host_range;
    } else {
      const double r = deskew::sanitised_range(in[i]);
      const double2 cs = beam_cs[i];
      const double x = r * cs.x, y = r * cs.y;  // :281-282
      const double md = (double)(i - g.first);
      const double myaw = g.ya + g.det_yaw * md, mx = g.x0 + g.det_x * md, my = g.y0 + g.det_y * md;  // :269-271
      double sn = 0.0, cn = 1.0;
      if (!(mx == 0.0 && my == 0.0 && myaw == 0.0)) libm::sincos(myaw, trig_tab, &sn, &cn);
      const deskew::T2 tm = deskew::mid_transform(mx, my, myaw, sn, cn);
      double ox, oy, bx, by;
      deskew::apply(tm, x, y, &ox, &oy);
      deskew::apply(base, ox, oy, &bx, &by);
      const double rr = sqrt(bx * bx + by * by);  // :295
      const double D = atan2(by, bx);             // :297 (the device library's)
      const double q = (D - amin) / inc;          // :113
      if (!isfinite(q)) {
        flagged = true;
      } else {
        const double rq = rint(q);
        if (rq != 0.0 && fabs(q - rq) < kBinGuard) flagged = true;
        if (fabs(q) < 2147483648.0) {
          const int32_t t = (int32_t)q;
          if (t >= 0 && t < n_beams) j = t;
        }
      }
      rf = (float)rr;
    }
    if (j >= 0)  // (j < n_beams: checked above, and by the host for its beams)
      atomicMax(&slots[j], ((unsigned long long)(uint32_t)(i + 1) << 32) | (unsigned long long)__float_as_uint(rf));
  }
  if (flagged) slots[n_beams] = 1ull;
  __syncthreads();
  for (int32_t i = (int32_t)threadIdx.x; i < n_beams; i += kDeskewThreads) {
    const unsigned long long v = slots[i];
    o[i] = v ? __uint_as_float((uint32_t)v) : 0.0f;  // :109-111: empty bins stay 0
  }
  if (threadIdx.x == 0 && slots[n_beams]) {
    flags[s] = 1;
    atomicAdd(&flags[n_scans], 1);
  }
}

__global__ __launch_bounds__(256) void atan2_kernel(const double* __restrict__ y, const double* __restrict__ x,
                                                    int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = atan2(y[i], x[i]);
}

__global__ __launch_bounds__(256) void sqrt_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = sqrt(x[i]);
}

hipError_t launch_deskew(const float* raw, int32_t n_scans, int32_t n_beams, float angle_min, float angle_increment,
                         const DeskewScan* scans, const DeskewSeg* segs, const double* beam_cs,
                         const double* trig_tab, float* out, int32_t* flags, hipStream_t stream) {
  if (n_scans <= 0) return hipSuccess;
  if (n_beams < 1 || n_beams > kDeskewMaxBeams) return hipErrorInvalidValue;
  hipLaunchKernelGGL(deskew_kernel, dim3((unsigned)n_scans), dim3(kDeskewThreads),
                     ((size_t)n_beams + 1) * sizeof(unsigned long long), stream, raw, n_scans, n_beams, angle_min,
                     angle_increment, scans, segs, reinterpret_cast<const double2*>(beam_cs), trig_tab, out, flags);
  return hipGetLastError();
}

hipError_t launch_atan2(const double* y, const double* x, int64_t n, double* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(atan2_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, y, x, n, out);
  return hipGetLastError();
}

hipError_t launch_sqrt(const double* x, int64_t n, double* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256;
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sqrt_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, n, out);
  return hipGetLastError();
}

}  // namespace csm
