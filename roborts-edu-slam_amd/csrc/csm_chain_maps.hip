// csm_chain_maps.hip — the kernels of the stack builder
// (include/csm_chain_maps.h): every submap of a query drawn from its chain's
// kept scans into the matcher's grid stack. The host plan they read is
// csm_chain_maps.hpp; paths cited are relative to the reference root.
//
// The mode built is ScanMatchMaps with just_update_occu_ and the Gaussian
// blur: SetCellOccuBlur (map/occu_grid_map.h:531-576) only ever raises a
// ProbabilityCell to a maximum (SetGridProbability, map/grid_map_cell.h:361-365)
// and never writes update_index_, so raises applied in any order, across the
// points of a scan, the scans of a chain and all chains at once, give the
// sequential result bit for bit. A cell's value is then a function of the SET
// of end cells of its grid alone: how many points, of which scans, end in a
// cell does not matter. The splat is therefore two kernels:
//
//   chain_mark_kernel   one lane per (placement, point): the point's end cell
//                       by the reference's arithmetic, the start-cell and
//                       in-map tests, and a plain byte store of 1 into the
//                       grid's hit mask (every writer stores the same value)
//   chain_raise_kernel  waves sweep the mask four cells a lane; a hit cell
//                       raises its centre to 1 and its (2 hk + 1)^2 kernel
//                       cells to the table's values, a lane each: integer atomicMax on the
//                       float's bits (probabilities are never negative: the
//                       maximum of the bits is the maximum of the values)
//                       behind a plain pre-check, as raise_prob of
//                       csm_gridmap.hip
//
// One lane per (point, kernel cell) raising straight into the grids, as
// blur_splat_kernel does within one map, measured 5.2 ms for config 3's 512
// chains x 11 scans (148 M raises at 29 G a second: the scans of a chain see
// the same walls and run at the same time, so nearly every raise passes the
// pre-check and becomes an atomic, scattered over 13 rows a wave — the slow
// shape for global atomics on this chip, an order of magnitude under the rate
// of contiguous 256-byte wave instructions). Through the mask the 5.9 M points
// collapse to the distinct end cells before anything is raised.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "csm_chain_maps_launch.hpp"

#pragma clang fp contract(off)

namespace csm {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ void raise_cell(float* cell, float p) {
  if (*cell < p) atomicMax(reinterpret_cast<unsigned int*>(cell), __float_as_uint(p));
}

// (int)(v + 0.5) where the cast is defined; false for a NaN, an infinity or a
// value the host's cast is undefined for. No such cell lies inside a grid
// (grids hold fewer than 2^31 cells), so the point is skipped either way.
__device__ __forceinline__ bool cell_of(double v, int* out) {
  const double r = v + 0.5;
  if (!(r > -2147483648.0 && r < 2147483647.0)) return false;
  *out = (int)r;
  return true;
}

// A block belongs to one placement (its pose is wave-uniform): blocks_per
// blocks cover the placement's points.
__global__ __launch_bounds__(kThreads) void chain_mark_kernel(const ChainPlacement* __restrict__ place,
                                                               int first_place, int blocks_per,
                                                               const double* __restrict__ pts, double inv_res,
                                                               uint8_t* __restrict__ hits, int size_x, int size_y,
                                                               int hk) {
  const ChainPlacement P = place[first_place + (int)(blockIdx.x / (unsigned)blocks_per)];
  const int b = (int)(blockIdx.x % (unsigned)blocks_per) * kThreads + threadIdx.x;
  if (b >= P.n_points) return;
  // CreateFrom(raw, 1 / resolution) (sensor_data_manager.h:99-115): one rounding per coordinate
  const double px = pts[2 * (P.pt_begin + b)] * inv_res, py = pts[2 * (P.pt_begin + b) + 1] * inv_res;
  // Affine2d(Translation2d(t) * Rotation2Dd(th)) * p, as pose_apply (csm_gridmap.cpp)
  const double ex = (P.c * px + (-P.s) * py) + P.tx;
  const double ey = (P.s * px + P.c * py) + P.ty;
  int x1, y1;
  if (!cell_of(ex, &x1) || !cell_of(ey, &y1)) return;
  // the start cell: the sensor origin (0, 0) through the same transform (occu_grid_map.h:312)
  const double sx = (P.c * 0.0 + (-P.s) * 0.0) + P.tx, sy = (P.s * 0.0 + P.c * 0.0) + P.ty;
  int x0, y0;
  if (cell_of(sx, &x0) && cell_of(sy, &y0) && x0 == x1 && y0 == y1) return;
  // PointInMap(x1, y1, half_kernel_size_ + 1) (:476-478, grid_map_base.h:344-352): keeps
  // every x1 +- hk, y1 +- hk inside this grid
  const int tol = hk + 1;
  if (!(x1 > tol && x1 < size_x - tol && y1 > tol && y1 < size_y - tol)) return;
  hits[(int64_t)P.grid * ((int64_t)size_x * size_y) + ((int64_t)y1 * size_x + x1)] = 1;
}

// hits4: the mask of all grids back to back, a dword (four cells) a lane; n4
// dwords cover the n_cells cells (the bytes past n_cells are zero). A wave
// takes its hit cells one after the other and spreads each one's kernel cells
// over its lanes: one load and one atomic instruction a hit, where a lane that
// walked its own hit's kernel cells made (2 hk + 1)^2 round trips to memory.
// The centre lane raises to 1: SetGridProbability(center, 1.0f) (:544) comes
// before the centre's own kernel value, which is drawn only when <= 1.
__global__ __launch_bounds__(kThreads) void chain_raise_kernel(const uint32_t* __restrict__ hits4, int64_t n4,
                                                                float* __restrict__ grids, int size_x, int size_y,
                                                                int hk, const float* __restrict__ ktab) {
  const int ks = 2 * hk + 1, k2 = ks * ks, centre = hk + ks * hk;
  const int lane = threadIdx.x & 63;
  const int64_t ncell = (int64_t)size_x * size_y;
  // base: the wave's first dword, the same in all its lanes
  for (int64_t base = (int64_t)blockIdx.x * kThreads + (threadIdx.x - lane); base < n4;
       base += (int64_t)gridDim.x * kThreads) {
    const uint32_t mine = base + lane < n4 ? hits4[base + lane] : 0u;
    for (unsigned long long have = __ballot(mine != 0); have != 0; have &= have - 1) {
      const int src = __ffsll((long long)have) - 1;
      const uint32_t m = (uint32_t)__shfl((int)mine, src);
      for (int byte = 0; byte < 4; ++byte) {
        if (!((m >> (8 * byte)) & 0xFFu)) continue;
        const int64_t cell = 4 * (base + src) + byte, g = cell / ncell, rest = cell - g * ncell;
        const int y1 = (int)(rest / size_x), x1 = (int)(rest - (int64_t)y1 * size_x);
        float* grid = grids + g * ncell;
        for (int k = lane; k < k2; k += 64) {
          const int i = k % ks - hk, j = k / ks - hk;      // kernel_index = (i+hk) + ks*(j+hk) :563
          const float p = k == centre ? 1.0f : ktab[k];    // (float)(kernel_value * offset) :567
          if (p <= 1.0f) raise_cell(grid + ((int64_t)(y1 + j) * size_x + (x1 + i)), p);
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_chain_fill(float* grids, uint8_t* hits, int64_t n_cells, float value, hipStream_t s) {
  if (n_cells <= 0) return hipSuccess;
  int bits;
  static_assert(sizeof(bits) == sizeof(value), "a cell is one dword");
  __builtin_memcpy(&bits, &value, sizeof(bits));
  const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)grids, bits, (size_t)n_cells, s);
  return e != hipSuccess ? e : hipMemsetAsync(hits, 0, chain_hits_bytes(n_cells), s);
}

hipError_t launch_chain_splat(const ChainPlacement* place, int32_t n_place, int32_t max_points, const double* pts,
                              double inv_res, float* grids, uint8_t* hits, int64_t n_cells, int32_t size_x,
                              int32_t size_y, int32_t hk, const float* ktab, hipStream_t s) {
  if (n_place <= 0 || max_points <= 0 || n_cells <= 0) return hipSuccess;
  const int64_t per = ((int64_t)max_points + kThreads - 1) / kThreads;
  // at most 2^30 blocks a launch: whole placements each
  const int64_t step = std::max<int64_t>(1, ((int64_t)1 << 30) / per);
  for (int64_t first = 0; first < n_place; first += step) {
    const int64_t n = std::min<int64_t>(step, n_place - first);
    hipLaunchKernelGGL(chain_mark_kernel, dim3((unsigned)(n * per)), dim3(kThreads), 0, s, place, (int)first, (int)per,
                       pts, inv_res, hits, size_x, size_y, hk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int64_t n4 = (int64_t)(chain_hits_bytes(n_cells) / 4);
  const int64_t blocks = std::min<int64_t>((n4 + kThreads - 1) / kThreads, 16384);
  hipLaunchKernelGGL(chain_raise_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s,
                     reinterpret_cast<const uint32_t*>(hits), n4, grids, size_x, size_y, hk, ktab);
  return hipGetLastError();
}

}  // namespace csm
