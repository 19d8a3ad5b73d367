// csm_optimize.hip — the Gauss-Newton scan matcher on the device
// (BasedOptimizeScanMatch, optimize_scan_matcher.h:68-221; SURVEY.md 8f row
// f3) for gfx950: UpdateCost alone (optimize_cost_kernel, one launch per
// iteration, the loop on the host) and the whole solve (optimize_solve_kernel,
// the loop in the kernel).
//
// One workgroup per scan. Per UpdateCost the 256 lanes project, gather and
// differentiate points in parallel (4 corner reads per point from the
// resident fp32 grid, no LDS staging: 16 B per point is nothing next to the
// launch latency), write each point's ten terms (cost, six lower-triangle
// entries of J^T J, three of -J^T e) to LDS, and ten lanes then add them up
// one accumulator each in point order. That order is the reference's loop
// order, so every sum is the reference's fp64 sum bit for bit; a tree
// reduction would not be. Between two UpdateCosts come glibc's cos/sin of the
// angle, the 3x3 LDLT solve and the step (csm_optimize_step.hpp): on the host
// for optimize_cost_kernel (csm_optimize_host.cpp), in lane 0 for
// optimize_solve_kernel (libm_sincos.hpp).
#include <hip/hip_runtime.h>

#include "csm_internal.hpp"
#include "csm_optimize_step.hpp"
#include "libm_sincos.hpp"

#pragma clang fp contract(off)

namespace csm {
namespace {

constexpr int kOptChunk = 512;  // points per LDS pass (10 x 4 KB of terms)
constexpr int kOptTerms = 10;   // cost, six of J^T J, three of -J^T e
constexpr int kOptAhead = 8;    // terms a summing lane loads before it adds them
constexpr int kOptCountLane = 64;  // counts the points in the map: wave 1, beside the summing lanes of wave 0

__device__ __forceinline__ double opt_cell(const float* g, int32_t sx, int64_t ncell, float outside, int x, int y) {
  // GetCell's flat index (grid_map_base.h:352-354); past the array: outside
  const int64_t idx = (int64_t)y * sx + x;
  return (idx >= 0 && idx < ncell) ? (double)g[idx] : (double)outside;
}

// One point's ten terms (UpdateCost's loop body, optimize_scan_matcher.h:
// 165-217) into row i of `terms`; ok[i] = the point is in the map.
__device__ __forceinline__ void opt_point_terms(const float* g, int32_t size_x, int64_t ncell, float outside, double fsx,
                                                double fsy, const OptScan& sc, double lx, double ly,
                                                double (*terms)[kOptTerms], int32_t* ok, int i) {
  // rotation * local_point + translation (:94-97, :167)
  const double x = (sc.c * lx + (-sc.s) * ly) + sc.tx;
  const double y = (sc.s * lx + sc.c * ly) + sc.ty;
  const bool in = x > 0 && x < fsx && y > 0 && y < fsy;  // PointInMap (grid_map_base.h:330-337)
  ok[i] = in ? 1 : 0;
  if (!in) return;
  const double x0 = floor(x), y0 = floor(y), x1 = ceil(x), y1 = ceil(y);
  const double p00 = opt_cell(g, size_x, ncell, outside, (int)x0, (int)y0);
  const double p01 = opt_cell(g, size_x, ncell, outside, (int)x0, (int)y1);
  const double p10 = opt_cell(g, size_x, ncell, outside, (int)x1, (int)y0);
  const double p11 = opt_cell(g, size_x, ncell, outside, (int)x1, (int)y1);
  double r = ((y - y0) * (p11 * (x - x0) + p01 * (x1 - x)) + (y1 - y) * (p10 * (x - x0) + p00 * (x1 - x)));
  r = (r >= 0) ? ((r <= 1) ? r : 1.0) : 0.0;
  const double e = 1 - r;
  const double ds02 = ((-sc.s) * lx - sc.c * ly);  // de_s (:200-201)
  const double ds12 = (sc.c * lx - sc.s * ly);
  const double dm0 = ((y - y0) * (p11 - p01) + (y1 - y) * (p10 - p00));  // de_m (:203-204)
  const double dm1 = ((x - x0) * (p11 - p10) + (x1 - x) * (p01 - p00));
  const double n0 = -dm0, n1 = -dm1;  // J = -de_m * de_s (:207)
  const double j0 = n0 * 1.0 + n1 * 0.0;
  const double j1 = n0 * 0.0 + n1 * 1.0;
  const double j2 = n0 * ds02 + n1 * ds12;
  terms[i][0] = e * e;
  terms[i][1] = j0 * j0;
  terms[i][2] = j1 * j0;
  terms[i][3] = j1 * j1;
  terms[i][4] = j2 * j0;
  terms[i][5] = j2 * j1;
  terms[i][6] = j2 * j2;
  terms[i][7] = (-j0) * e;
  terms[i][8] = (-j1) * e;
  terms[i][9] = (-j2) * e;
}

// One UpdateCost over a scan's n points at p0, by the whole block: lanes 0-9
// return their sum in *acc (one accumulator each, in point order), lane
// kOptCountLane the points in the map in *cnt. Ends on a barrier: the LDS is
// free again. The sums are chains of dependent fp64 adds, one LDS read each:
// a point's ten terms lie side by side (the ten lanes read ten banks' worth,
// not one bank ten times) and a lane loads kOptAhead terms before it adds
// them, so the reads' latency is paid once per group. A point outside the map
// keeps the sum as it is (a select, not an add of zero: -0.0 stays -0.0).
__device__ __forceinline__ void opt_update_cost(const float* g, int32_t size_x, int32_t size_y, float outside,
                                                const double* pts, int64_t p0, int64_t n, const OptScan& sc,
                                                double (*terms)[kOptTerms], int32_t* ok, double* acc, int32_t* cnt) {
  const int64_t ncell = (int64_t)size_x * size_y;
  const double fsx = (double)size_x, fsy = (double)size_y;
  const int tid = threadIdx.x;
  *acc = 0.0;
  *cnt = 0;
  for (int64_t base = 0; base < n; base += kOptChunk) {
    const int m = (int)((n - base < kOptChunk) ? (n - base) : kOptChunk);
    for (int i = tid; i < m; i += kBlock) {
      const double2 lp = reinterpret_cast<const double2*>(pts)[p0 + base + i];
      opt_point_terms(g, size_x, ncell, outside, fsx, fsy, sc, lp.x, lp.y, terms, ok, i);
    }
    __syncthreads();
    if (tid < kOptTerms) {
      double a = *acc;
      int i = 0;
      for (; i + kOptAhead <= m; i += kOptAhead) {
        double t[kOptAhead];
        int32_t in[kOptAhead];
#pragma unroll
        for (int j = 0; j < kOptAhead; ++j) {
          t[j] = terms[i + j][tid];
          in[j] = ok[i + j];
        }
#pragma unroll
        for (int j = 0; j < kOptAhead; ++j) a = in[j] ? a + t[j] : a;
      }
      for (; i < m; ++i)
        if (ok[i]) a = a + terms[i][tid];
      *acc = a;
    } else if (tid == kOptCountLane) {
      for (int i = 0; i < m; ++i) *cnt += ok[i];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void optimize_cost_kernel(OptArgs A) {
  const int s = blockIdx.x;
  const OptScan sc = A.scans[s];
  if (!sc.active) return;  // uniform over the block
  const int64_t p0 = A.offsets[s];
  const int64_t n = A.offsets[s + 1] - p0;
  __shared__ double terms[kOptChunk][kOptTerms];
  __shared__ int32_t ok[kOptChunk];
  const int tid = threadIdx.x;
  double acc;
  int32_t cnt;
  opt_update_cost(A.grid + (int64_t)sc.grid * ((int64_t)A.size_x * A.size_y), A.size_x, A.size_y, A.outside, A.pts, p0,
                  n, sc, terms, ok, &acc, &cnt);
  if (tid < kOptTerms) A.out[s].v[tid] = acc;
  if (tid == kOptCountLane) A.out[s].valid = cnt;
}

// The whole Gauss-Newton solve of one scan per workgroup
// (BasedOptimizeScanMatch::ScanMatch's loop, optimize_scan_matcher.h:84-124):
// per iteration lane 0 takes glibc's sincos of the angle (libm_sincos.hpp),
// the block evaluates UpdateCost as optimize_cost_kernel does, and lane 0
// takes the step (csm_optimize_step.hpp). Pose and state reach the other
// lanes through LDS; the two state words alternate, so lane 0 writing the
// next one never races a lane still reading the last.
__global__ __launch_bounds__(kBlock) void optimize_solve_kernel(OptSolveArgs A) {
  const int s = blockIdx.x;
  if (A.scans[s].state != opt::kRun) return;  // uniform over the block
  const int64_t p0 = A.offsets[s];
  const int64_t n = A.offsets[s + 1] - p0;
  const float* g = A.grid + (A.grid_index ? (int64_t)A.grid_index[s] : 0) * ((int64_t)A.size_x * A.size_y);
  __shared__ double terms[kOptChunk][kOptTerms];
  __shared__ int32_t ok[kOptChunk];
  __shared__ double sums[10];
  __shared__ int32_t valid;
  __shared__ OptScan pose;
  __shared__ int32_t state_trig, state_step;
  const int tid = threadIdx.x;
  double est[3] = {0.0, 0.0, 0.0}, cost = 0.0;  // lane 0's
  int32_t iters = 0, state = opt::kRun;
  if (tid == 0) {
    est[0] = A.scans[s].est[0];
    est[1] = A.scans[s].est[1];
    est[2] = A.scans[s].est[2];
  }
  for (int iter = 0; iter < A.iterate_max_times; ++iter) {
    if (tid == 0) {
      if (libm::sincos_device_ok(est[2])) {
        OptScan o;
        libm::sincos(est[2], A.tab, &o.s, &o.c);  // rotation (:96-97), de_s (:200-201)
        o.tx = est[0];
        o.ty = est[1];
        o.active = 1;
        o.grid = 0;
        pose = o;
      } else {
        state = opt::kHost;  // outside the restated domain: the host loop runs this scan
      }
      state_trig = state;
    }
    __syncthreads();
    if (state_trig != opt::kRun) break;  // uniform
    const OptScan sc = pose;
    double acc;
    int32_t cnt;
    opt_update_cost(g, A.size_x, A.size_y, A.outside, A.pts, p0, n, sc, terms, ok, &acc, &cnt);
    if (tid < kOptTerms) sums[tid] = acc;
    if (tid == kOptCountLane) valid = cnt;
    __syncthreads();
    if (tid == 0) {
      double v[10];
      for (int k = 0; k < 10; ++k) v[k] = sums[k];
      state = opt::step(v, valid, iter, A.P, est, &cost);
      iters = iter + 1;
      state_step = state;
    }
    __syncthreads();
    if (state_step != opt::kRun) break;  // uniform
  }
  if (tid == 0) {
    OptSolveScan& o = A.scans[s];
    o.est[0] = est[0];
    o.est[1] = est[1];
    o.est[2] = est[2];
    o.cost = cost;
    o.iters = iters;
    o.state = (state == opt::kRun) ? (int32_t)opt::kDone : state;  // out of iterations
  }
}

}  // namespace

hipError_t launch_optimize_cost(const OptArgs& A, int32_t n_scans, hipStream_t stream) {
  if (n_scans <= 0) return hipSuccess;
  hipLaunchKernelGGL(optimize_cost_kernel, dim3((unsigned)n_scans), dim3(kBlock), 0, stream, A);
  return hipGetLastError();
}

hipError_t launch_optimize_solve(const OptSolveArgs& A, int32_t n_scans, hipStream_t stream) {
  if (n_scans <= 0) return hipSuccess;
  hipLaunchKernelGGL(optimize_solve_kernel, dim3((unsigned)n_scans), dim3(kBlock), 0, stream, A);
  return hipGetLastError();
}

}  // namespace csm
