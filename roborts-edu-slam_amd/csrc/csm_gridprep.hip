// csm_gridprep.hip — grid and batch preparation kernels, none of them on the
// scoring path: the bound on a batch's points (csm_load_scans_async), the
// analysis of a grid and its exact fixed-point copy (csm_set_grid), and the
// incremental refresh of a resident grid (csm_update_grid_cells).
#include <hip/hip_runtime.h>

#include "csm_internal.hpp"

#pragma clang fp contract(off)

namespace csm {

// max |x| + |y| over a batch's points (csm_load_scans_async): the bound
// int_mode_ok needs, found on the device while the batch uploads instead of
// by the host reading every point. Non-negative doubles order like their
// bits, and a NaN's bits exceed +inf's, so an integer max keeps NaN.
__global__ __launch_bounds__(256) void points_maxabs_kernel(const double2* __restrict__ p, int64_t n,
                                                            unsigned long long* __restrict__ out) {
  unsigned long long m = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double2 q = p[i];
    const double a = fabs(q.x) + fabs(q.y);
    const unsigned long long b = __builtin_bit_cast(unsigned long long, a);
    m = b > m ? b : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(m, o, 64);
    m = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

hipError_t launch_points_maxabs(const double* pts, int64_t n, unsigned long long* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024;
  hipLaunchKernelGGL(points_maxabs_kernel, dim3((unsigned)blocks), dim3(256), 0, stream,
                     reinterpret_cast<const double2*>(pts), n, out);
  return hipGetLastError();
}

// ---- grid analysis / fixed-point copy (csm_set_grid) -----------------------
namespace {

// Per cell: finite? smallest power of two the value is a multiple of, and |v|.
// Pass 1: each block reduces its cells in registers, then across its waves in
// LDS, and writes one partial (no atomics: thousands of same-address atomics
// serialised the old version at ~0.3 ms for a 3000 x 3000 map).
__global__ __launch_bounds__(256) void analyze_grid_kernel(const float* __restrict__ g, int64_t n,
                                                           GridStats* __restrict__ partials) {
  int min_g = INT32_MAX;
  uint32_t max_bits = 0;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t u = __float_as_uint(g[i]) & 0x7FFFFFFFu;
    const uint32_t e = u >> 23, m = u & 0x7FFFFFu;
    if (e == 0xFF) {
      bad = 1;
      continue;
    }
    if (u == 0) continue;
    const uint32_t mm = (e == 0) ? m : (m | 0x800000u);
    const int gexp = ((e == 0) ? -149 : (int)e - 150) + __builtin_ctz(mm);
    min_g = min(min_g, gexp);
    max_bits = max(max_bits, u);
  }
  for (int off = 32; off > 0; off >>= 1) {
    min_g = min(min_g, __shfl_down(min_g, off, 64));
    max_bits = max(max_bits, (uint32_t)__shfl_down((int)max_bits, off, 64));
    bad |= __shfl_down(bad, off, 64);
  }
  __shared__ GridStats w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = GridStats{min_g, max_bits, bad, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    GridStats r = w[0];
    for (int k = 1; k < 4; ++k) {
      r.min_gexp = min(r.min_gexp, w[k].min_gexp);
      r.max_abs_bits = max(r.max_abs_bits, w[k].max_abs_bits);
      r.nonfinite |= w[k].nonfinite;
    }
    partials[blockIdx.x] = r;
  }
}

// Pass 2: one block folds the partials into st[0].
__global__ __launch_bounds__(256) void analyze_reduce_kernel(const GridStats* __restrict__ partials, int np,
                                                             GridStats* __restrict__ st) {
  int min_g = INT32_MAX;
  uint32_t max_bits = 0;
  int bad = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) {
    const GridStats p = partials[i];
    min_g = min(min_g, p.min_gexp);
    max_bits = max(max_bits, p.max_abs_bits);
    bad |= p.nonfinite;
  }
  for (int off = 32; off > 0; off >>= 1) {
    min_g = min(min_g, __shfl_down(min_g, off, 64));
    max_bits = max(max_bits, (uint32_t)__shfl_down((int)max_bits, off, 64));
    bad |= __shfl_down(bad, off, 64);
  }
  __shared__ GridStats w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = GridStats{min_g, max_bits, bad, 0};
  __syncthreads();
  if (threadIdx.x == 0) {
    GridStats r = w[0];
    for (int k = 1; k < 4; ++k) {
      r.min_gexp = min(r.min_gexp, w[k].min_gexp);
      r.max_abs_bits = max(r.max_abs_bits, w[k].max_abs_bits);
      r.nonfinite |= w[k].nonfinite;
    }
    st[0] = r;
  }
}

// gi = (g - outside) * 2^E, exact when the host accepted E.
// gi[y * pitch + x] = (g[y * sx + x] - outside) * 2^E; pad cells (x >= sx)
// and the appended zero row y = sy (what DMA reads for rows off the grid) = 0.
__global__ __launch_bounds__(256) void fixed_point_kernel(const float* __restrict__ g, int32_t sx,
                                                          int32_t sy, int32_t pitch, float outside,
                                                          double scale, int32_t* __restrict__ gi,
                                                          int32_t pad_rows) {
  const int64_t n = (int64_t)pitch * (sy + pad_rows);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = i / pitch;
    const int x = (int)(i - y * pitch);
    gi[i] = (x < sx && y < sy) ? (int32_t)(((double)g[y * sx + x] - (double)outside) * scale) : 0;
  }
}

}  // namespace

hipError_t launch_analyze_grid(const float* g, int64_t n, GridStats* d_stats, hipStream_t stream) {
  // d_stats holds 1 + kAnalyzeBlocks entries: the result, then the partials
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kAnalyzeBlocks));
  hipLaunchKernelGGL(analyze_grid_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, n, d_stats + 1);
  hipLaunchKernelGGL(analyze_reduce_kernel, dim3(1), dim3(256), 0, stream, d_stats + 1, (int)blocks, d_stats);
  return hipGetLastError();
}

hipError_t launch_fixed_point(const float* g, int32_t sx, int32_t sy, int32_t pitch, float outside,
                              int int_exp, int32_t* gi, hipStream_t stream, bool pad) {
  const int32_t pad_rows = pad ? kGridiPadRows : 0;
  const int64_t n = (int64_t)pitch * (sy + pad_rows);
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(fixed_point_kernel, dim3((unsigned)std::max<int64_t>(blocks, 1)), dim3(256), 0,
                     stream, g, sx, sy, pitch, outside, ldexp(1.0, int_exp), gi, pad_rows);
  return hipGetLastError();
}

namespace {
// Incremental refresh of a resident grid (csm_update_grid_cells): each entry
// rewrites one fp32 cell and, when the exact fixed-point copy exists, its
// int32 image with the fixed_point_kernel's expression. Duplicate indices
// carry the same value, so their order does not matter.
__global__ __launch_bounds__(256) void update_cells_kernel(const CellUpdate* __restrict__ u, int64_t n,
                                                           float* __restrict__ g, int32_t sx,
                                                           int32_t* __restrict__ gi, int32_t pitch,
                                                           float outside, double scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const CellUpdate c = u[i];
    g[c.index] = c.value;
    if (gi) {
      const int32_t y = c.index / sx;
      const int32_t x = c.index - y * sx;
      gi[(int64_t)y * pitch + x] = (int32_t)(((double)c.value - (double)outside) * scale);
    }
  }
}
}  // namespace

hipError_t launch_update_cells(const CellUpdate* d_updates, int64_t n, float* g, int32_t sx, int32_t* gi,
                               int32_t pitch, float outside, int int_exp, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(update_cells_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_updates, n, g, sx, gi,
                     pitch, outside, ldexp(1.0, int_exp));
  return hipGetLastError();
}

}  // namespace csm
