// csm_palette.hip — the palette copy of the fixed-point grid, read by the v10
// palette box kernel (csm_box.hip).
//
// A scan-match grid holds a handful of distinct cell values: the unknown
// value (0 in gridi, which stores value - outside), the occupied value and
// the levels of the blur splat (occu_grid_map.h:83-105,531-576: a cell keeps
// the max of kernel * offset). The palette is those values, 0 first then
// ascending, and the copy holds every cell's index into it, one byte per cell
// in gridi's own layout (same pitch, same zero columns and rows). A grid with
// more than kPalMax distinct values has no palette (the box kernels read
// gridi itself).
//
//   pal_collect_kernel  each block dedupes its slice of cells in an LDS hash
//                       and lists its values (or marks an overflow)
//   pal_merge_kernel    one block merges the lists, sorts them, writes the
//                       palette and its size
//   pal_index_kernel    every cell's index by binary search in the palette
//   pal_strips_kernel   (palettes of at most kPairMaxPal values) the strip
//                       copies the v11 pair box kernel reads
//   istrips_kernel      the strip copies of gridi itself that the phase
//                       kernel reads (8-cell strips, two copies)
//   bg_hist_kernel,     (with the strips) the background index, the one most
//   bg_map_kernel       in-grid cells hold, and the map of box corners whose
//                       whole 13 x 13 box holds it, which the pair kernel
//                       reads to skip such beams
#include <hip/hip_runtime.h>

#include <cstdint>

#include "csm_internal.hpp"

namespace csm {
namespace {

constexpr int kPalHash = 1024;            // LDS hash slots (>= 2 * (kPalMax + 256))
constexpr int32_t kPalEmpty = INT32_MIN;  // never a gridi value (|value| < 2^26)
constexpr int kPalCollectBlocks = 1024;
constexpr int kPalList = kPalMax + 1;     // per block: count, then values

__device__ __forceinline__ uint32_t pal_hash(int32_t v) { return ((uint32_t)v * 2654435761u) >> 22; }

// Insert v (non-zero) into the LDS set; `count` counts the distinct values.
__device__ __forceinline__ void pal_insert(int32_t* key, int32_t* count, int32_t v) {
  if (v == 0 || *(volatile int32_t*)count > kPalMax) return;
  uint32_t h = pal_hash(v);
  for (int probe = 0; probe < kPalHash; ++probe) {
    const int32_t k = key[h];
    if (k == v) return;
    if (k == kPalEmpty) {
      const int32_t old = atomicCAS(&key[h], kPalEmpty, v);
      if (old == kPalEmpty) {
        atomicAdd(count, 1);
        return;
      }
      if (old == v) return;
    }
    h = (h + 1) & (kPalHash - 1);
  }
}

__global__ __launch_bounds__(256) void pal_collect_kernel(const int4* __restrict__ g, int64_t n4, int64_t per4,
                                                          int32_t* __restrict__ lists) {
  __shared__ int32_t key[kPalHash];
  __shared__ int32_t count, pos;
  for (int i = threadIdx.x; i < kPalHash; i += 256) key[i] = kPalEmpty;
  if (threadIdx.x == 0) {
    count = 0;
    pos = 0;
  }
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * per4, b1 = min(n4, b0 + per4);
  for (int64_t i = b0 + threadIdx.x; i < b1; i += 256) {
    const int4 v = g[i];
    pal_insert(key, &count, v.x);
    pal_insert(key, &count, v.y);
    pal_insert(key, &count, v.z);
    pal_insert(key, &count, v.w);
  }
  __syncthreads();
  int32_t* out = lists + (int64_t)blockIdx.x * kPalList;
  if (count > kPalMax) {
    if (threadIdx.x == 0) out[0] = kPalMax + 1;
    return;
  }
  for (int i = threadIdx.x; i < kPalHash; i += 256)
    if (key[i] != kPalEmpty) out[1 + atomicAdd(&pos, 1)] = key[i];
  if (threadIdx.x == 0) out[0] = count;
}

__global__ __launch_bounds__(256) void pal_merge_kernel(const int32_t* __restrict__ lists, int nb,
                                                        int32_t* __restrict__ vals, int32_t* __restrict__ state) {
  __shared__ int32_t key[kPalHash];
  __shared__ int32_t sorted[256];
  __shared__ int32_t count, pos, over;
  for (int i = threadIdx.x; i < kPalHash; i += 256) key[i] = kPalEmpty;
  if (threadIdx.x == 0) {
    count = 0;
    pos = 0;
    over = 0;
  }
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int32_t* in = lists + (int64_t)b * kPalList;
    const int32_t c = in[0];
    if (c > kPalMax) {
      if (threadIdx.x == 0) over = 1;
      break;  // uniform: every thread read the same count
    }
    for (int i = threadIdx.x; i < c; i += 256) pal_insert(key, &count, in[1 + i]);
  }
  __syncthreads();
  // index 0 is the zero value: at most kPalMax - 1 others
  if (over || count > kPalMax - 1) {
    if (threadIdx.x == 0) state[0] = kPalMax + 1;
    return;
  }
  sorted[threadIdx.x] = INT32_MAX;
  __syncthreads();
  for (int i = threadIdx.x; i < kPalHash; i += 256)
    if (key[i] != kPalEmpty) sorted[atomicAdd(&pos, 1)] = key[i];
  __syncthreads();
  // bitonic sort of the 256 slots (padding INT32_MAX sorts last)
  const int t = threadIdx.x;
  for (int size = 2; size <= 256; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int o = t ^ stride;
      if (o > t) {
        const bool up = (t & size) == 0;
        const int32_t x = sorted[t], y = sorted[o];
        if ((x > y) == up) {
          sorted[t] = y;
          sorted[o] = x;
        }
      }
      __syncthreads();
    }
  }
  if (t == 0) vals[0] = 0;
  if (t < count) vals[1 + t] = sorted[t];
  if (t == 0) state[0] = count + 1;
}

__global__ __launch_bounds__(256) void pal_index_kernel(const int4* __restrict__ g, int64_t n4,
                                                        const int32_t* __restrict__ vals,
                                                        const int32_t* __restrict__ state,
                                                        uint32_t* __restrict__ idx4) {
  __shared__ int32_t sv[kPalMax];
  const int m = state[0];
  if (m < 1 || m > kPalMax) return;  // no palette: nothing to index
  for (int i = threadIdx.x; i < m; i += 256) sv[i] = vals[i];
  __syncthreads();
  auto find = [&](int32_t v) -> uint32_t {
    if (v == 0) return 0u;
    int lo = 1, hi = m - 1;  // sv[1..m-1] ascending; v is one of them
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sv[mid] < v)
        lo = mid + 1;
      else
        hi = mid;
    }
    return (uint32_t)lo;
  };
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int4 v = g[i];
    idx4[i] = find(v.x) | (find(v.y) << 8) | (find(v.z) << 16) | (find(v.w) << 24);
  }
}

// The padded index image the pair kernel reads, at grid cell (x, y) of either
// sign: cells off the grid are index 0 but for column -1 and row -1, which
// repeat column 0 and row 0 (kStripPadLo). The strip copies and the map of
// uniform boxes are both made from it.
__device__ __forceinline__ uint32_t padded_index(const uint8_t* __restrict__ idx, int pitch, int sx, int sy, int x,
                                                 int y) {
  return (y >= -1 && y < sy && x >= -1 && x < sx) ? idx[(int64_t)max(y, 0) * pitch + max(x, 0)] : 0u;
}

// Histogram of the in-grid cells' palette indices (palettes of at most
// kPairMaxPal values), per grid of the stack (blockIdx.y).
__global__ __launch_bounds__(256) void bg_hist_kernel(const uint8_t* __restrict__ idx, int pitch, int sx, int sy,
                                                      int64_t idx_stride, int32_t* __restrict__ info) {
  __shared__ uint32_t h[kPairMaxPal];
  if (threadIdx.x < kPairMaxPal) h[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t* g = idx + (int64_t)blockIdx.y * idx_stride;
  const int64_t n = (int64_t)sx * sy;
  uint32_t mine[kPairMaxPal] = {};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / sx), x = (int)(i - (int64_t)y * sx);
    const uint32_t v = g[(int64_t)y * pitch + x] & (kPairMaxPal - 1);
#pragma unroll
    for (int k = 0; k < kPairMaxPal; ++k) mine[k] += v == (uint32_t)k;
  }
#pragma unroll
  for (int k = 0; k < kPairMaxPal; ++k)
    if (mine[k]) atomicAdd(&h[k], mine[k]);
  __syncthreads();
  if (threadIdx.x < kPairMaxPal && h[threadIdx.x])
    atomicAdd(reinterpret_cast<uint32_t*>(info) + (int64_t)blockIdx.y * kBgInfoInts + threadIdx.x, h[threadIdx.x]);
}

// The map of uniform boxes (csm_internal.hpp BgGeom): one thread per 8 x 8
// tile of padded corners. The background is the index with the largest count
// (the lowest of equal ones). Row r of the tile's (N + 7)^2 cells gives the
// eight corners' "N cells from here are background" bits; corner row j's byte
// is the AND of rows j .. j + N - 1.
template <int N>
__global__ __launch_bounds__(256) void bg_map_kernel(const uint8_t* __restrict__ idx, int pitch, int sx, int sy,
                                                     int64_t idx_stride, int tiles_x, int tiles_y,
                                                     int32_t* __restrict__ info, int set_at,
                                                     uint64_t* __restrict__ out) {
  static_assert(N >= 2 && N + 7 <= 32, "a tile row's cells in one 32-bit mask");
  int32_t* gi = info + (int64_t)blockIdx.y * kBgInfoInts;
  uint32_t bg = 0, best = 0;
  for (int k = 0; k < kPairMaxPal; ++k) {
    const uint32_t c = (uint32_t)gi[k];
    if (c > best) {
      best = c;
      bg = (uint32_t)k;
    }
  }
  const uint8_t* g = idx + (int64_t)blockIdx.y * idx_stride;
  const int64_t tiles = (int64_t)tiles_x * tiles_y;
  uint32_t nset = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tiles; i += (int64_t)gridDim.x * 256) {
    const int ty = (int)(i / tiles_x), tx = (int)(i - (int64_t)ty * tiles_x);
    const int x0 = 8 * tx - kStripPadLo, y0 = 8 * ty - kStripPadLo;
    uint32_t row[N + 7];
#pragma unroll
    for (int r = 0; r < N + 7; ++r) {
      uint32_t m = 0;
      for (int b = 0; b < N + 7; ++b) m |= (uint32_t)(padded_index(g, pitch, sx, sy, x0 + b, y0 + r) == bg) << b;
      uint32_t a = m;  // bit b: cells b .. b + N - 1 of the row are background
#pragma unroll
      for (int s = 1; s < N; ++s) a &= m >> s;
      row[r] = a & 0xFFu;
    }
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t a = row[j];
#pragma unroll
      for (int r = 1; r < N; ++r) a &= row[j + r];
      w |= (uint64_t)a << (8 * j);
    }
    out[(int64_t)blockIdx.y * tiles + i] = w;
    nset += (uint32_t)__popcll(w);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) gi[kBgInfoBg] = (int32_t)bg;
  if (nset) atomicAdd(reinterpret_cast<uint32_t*>(gi) + set_at, nset);
}

// Strip copies of the palette index grid (v11 pair box kernel): copy c holds
// cell x of row y at byte (x + kStripPadLo + kStripShift c) of its strip row,
// strips kStripW bytes wide with their rows contiguous (row y of strip t at
// (t * rows + kStripPadLo + y) * 16). One thread writes one 16-byte strip row;
// cells off the grid are index 0 but for column -1 and row -1, which repeat
// column 0 and row 0 (kStripPadLo).
__global__ __launch_bounds__(256) void pal_strips_kernel(const uint8_t* __restrict__ idx, int pitch, int sx,
                                                         int sy, int rows, int n_strips, int64_t idx_stride,
                                                         int64_t grid_bytes, int n_grids, uint4* __restrict__ out) {
  const int64_t per_copy = (int64_t)n_strips * rows;
  const int64_t total = (int64_t)n_grids * kStripCopies * per_copy;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t g = i / (kStripCopies * per_copy);
    const int64_t r = i - g * kStripCopies * per_copy;
    const int c = (int)(r / per_copy);
    const int64_t sr = r - (int64_t)c * per_copy;
    const int t = (int)(sr / rows);
    const int y = (int)(sr - (int64_t)t * rows) - kStripPadLo;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int x = kStripW * t + b - kStripShift * c - kStripPadLo;
      w[b >> 2] |= padded_index(idx + g * idx_stride, pitch, sx, sy, x, y) << (8 * (b & 3));
    }
    out[(g * grid_bytes + (int64_t)c * per_copy * kStripW) / 16 + sr] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// Strip copies of gridi (the phase kernel's strip form): copy c holds cell x
// of row y at cell x + kIStripPadLo + 4c of its 8-cell strip row, row y at
// strip row y + kIStripPadLo; column -1 repeats column 0 and row -1 row 0,
// other cells off the grid are 0 (the outside value). One thread per 16-byte
// half row.
__global__ __launch_bounds__(256) void istrips_kernel(const int32_t* __restrict__ gi, int pitch, int sx, int sy,
                                                      int rows, int n_strips, int64_t gi_stride, int64_t grid_ints,
                                                      int n_grids, int4* __restrict__ out) {
  const int64_t per_copy = (int64_t)n_strips * rows * 2;  // half rows
  const int64_t total = (int64_t)n_grids * kIStripCopies * per_copy;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t g = i / (kIStripCopies * per_copy);
    const int64_t r = i - g * kIStripCopies * per_copy;
    const int c = (int)(r / per_copy);
    const int64_t hr = r - (int64_t)c * per_copy;  // half row within the copy
    const int64_t sr = hr >> 1;
    const int t = (int)(sr / rows);
    const int y = (int)(sr - (int64_t)t * rows) - kIStripPadLo;
    const int x0 = kIStripCells * t + 4 * (int)(hr & 1) - 4 * c - kIStripPadLo;
    const int32_t* src = gi + g * gi_stride + (int64_t)max(y, 0) * pitch;
    int v[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int x = x0 + b;
      v[b] = (y >= -1 && y < sy && x >= -1 && x < sx) ? src[max(x, 0)] : 0;
    }
    out[(g * grid_ints + (int64_t)c * per_copy * 4) / 4 + hr] = make_int4(v[0], v[1], v[2], v[3]);
  }
}

}  // namespace

// (istrip_geom, strip_geom, bg_geom: the sizes of what these launchers fill,
// csm_grid_copies.hpp)

hipError_t launch_build_istrips(const int32_t* gridi, int pitch, int size_x, int size_y, int64_t gridi_stride,
                                int n_grids, int32_t* out, hipStream_t stream) {
  const StripGeom G = istrip_geom(size_x, size_y);
  if (!gridi || !out || n_grids < 1 || pitch < size_x) return hipErrorInvalidValue;
  const int64_t total = (int64_t)n_grids * kIStripCopies * G.n_strips * G.rows * 2;
  const int64_t blocks = (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
  hipLaunchKernelGGL(istrips_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, gridi, pitch, size_x, size_y,
                     G.rows, G.n_strips, gridi_stride, G.grid_bytes / 4, n_grids, reinterpret_cast<int4*>(out));
  return hipGetLastError();
}

hipError_t launch_build_strips(const uint8_t* idx, int pitch, int size_x, int size_y, int64_t idx_stride,
                               int n_grids, uint8_t* out, hipStream_t stream) {
  const StripGeom G = strip_geom(size_x, size_y);
  if (!idx || !out || n_grids < 1 || pitch < size_x) return hipErrorInvalidValue;
  const int64_t total = (int64_t)n_grids * kStripCopies * G.n_strips * G.rows;
  const int64_t blocks = (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
  hipLaunchKernelGGL(pal_strips_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, idx, pitch, size_x, size_y,
                     G.rows, G.n_strips, idx_stride, G.grid_bytes, n_grids, reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

hipError_t launch_build_bg_map(const uint8_t* idx, int pitch, int size_x, int size_y, int64_t idx_stride,
                               int n_grids, int32_t* info, uint8_t* out, uint8_t* out5, hipStream_t stream) {
  static_assert(kIStripPadLo == kStripPadLo, "one padded coordinate system for both maps");
  const BgGeom G = bg_geom(size_x, size_y);
  if (!idx || !info || !out || !out5 || n_grids < 1 || n_grids > 65535 || pitch < size_x) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(info, 0, (size_t)n_grids * kBgInfoInts * sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
  const int64_t cells = (int64_t)size_x * size_y, tiles = (int64_t)G.tiles_x * G.tiles_y;
  const int64_t hb = (cells + 4095) / 4096 < 1024 ? (cells + 4095) / 4096 : 1024;
  hipLaunchKernelGGL(bg_hist_kernel, dim3((unsigned)hb, (unsigned)n_grids), dim3(256), 0, stream, idx, pitch, size_x,
                     size_y, idx_stride, info);
  const int64_t mb = (tiles + 255) / 256 < 4096 ? (tiles + 255) / 256 : 4096;
  hipLaunchKernelGGL(bg_map_kernel<kPalMaxSpace>, dim3((unsigned)mb, (unsigned)n_grids), dim3(256), 0, stream, idx,
                     pitch, size_x, size_y, idx_stride, G.tiles_x, G.tiles_y, info, kBgInfoSet,
                     reinterpret_cast<uint64_t*>(out));
  hipLaunchKernelGGL(bg_map_kernel<kBgPhaseBox>, dim3((unsigned)mb, (unsigned)n_grids), dim3(256), 0, stream, idx,
                     pitch, size_x, size_y, idx_stride, G.tiles_x, G.tiles_y, info, kBgInfoSet5,
                     reinterpret_cast<uint64_t*>(out5));
  return hipGetLastError();
}

int64_t pal_scratch_ints(int64_t n) {
  const int64_t n4 = n / 4;
  const int64_t nb = n4 <= 0 ? 1 : (n4 + 4095) / 4096 < kPalCollectBlocks ? (n4 + 4095) / 4096 : kPalCollectBlocks;
  return nb * kPalList;
}

hipError_t launch_build_palette(const int32_t* gridi, int64_t n, int32_t* scratch, int32_t* vals, int32_t* state,
                                uint8_t* idx, hipStream_t stream) {
  if (n <= 0 || n % 4 != 0 || !gridi || !scratch || !vals || !state || !idx) return hipErrorInvalidValue;
  const int64_t n4 = n / 4;
  const int nb = (int)(pal_scratch_ints(n) / kPalList);
  const int64_t per4 = (n4 + nb - 1) / nb;
  const int4* g = reinterpret_cast<const int4*>(gridi);
  hipLaunchKernelGGL(pal_collect_kernel, dim3(nb), dim3(256), 0, stream, g, n4, per4, scratch);
  hipLaunchKernelGGL(pal_merge_kernel, dim3(1), dim3(256), 0, stream, scratch, nb, vals, state);
  const int64_t blocks = (n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192;
  hipLaunchKernelGGL(pal_index_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, n4, vals, state,
                     reinterpret_cast<uint32_t*>(idx));
  return hipGetLastError();
}

}  // namespace csm
