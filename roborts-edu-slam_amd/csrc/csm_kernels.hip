// csm_kernels.hip — CDNA4 (gfx950) kernels of the correlative scan matcher.
//
// Hot path replaced: the theta x X x Y x beam loops of
// MultiResolutionCorrelateScanMatcher::ScanMatch / GetResponse
// (correlate_scan_matcher.h:552-584, 637-662) plus PenalizeResponse (:718-745).
//
// The general-purpose scoring kernels, the fallbacks of the specialised
// families (csm_box.hip one-cell steps, csm_phase.hip sub-cell steps,
// csm_tiny.hip sub-cell spans, csm_split.hip few-window launches), and nothing
// else (grid and batch preparation: csm_gridprep.hip):
//   v2 score_cols_kernel   any window and any grid: lane = (theta, x) column,
//                          fp64 sums in the reference's beam order for any fp32
//                          grid, or exact fixed-point sums (INT mode)
//   v4 score_rowsd_kernel  INT mode, windows whose x-span fits a row segment:
//                          row segments staged in LDS by LDS-DMA
//   reduce_best_kernel     per-window argmax of the block partials
// (r03 retired v1, lane per candidate, and v3, register-staged row segments:
// every window they took, v2 or v4 takes, and no selection reached them.)
//
// Exactness: every double expression is evaluated in the reference's order
// with contraction disabled (pragma below + -ffp-contract=off), the cast to
// int truncates toward zero (v_cvt_i32_f64), and cos/sin come from the host.
#include <hip/hip_runtime.h>

#include "csm_internal.hpp"
#include "csm_score_sink.hpp"

#pragma clang fp contract(off)

namespace csm {

namespace {

// ---- v2: column kernel ------------------------------------------------------
// One wave per block; lane = one (theta, x) column of the window, KT rows of
// y per lane (KT == n_space for the front-end windows, so no row is wasted).
// Per beam a lane rotates the point once (LUT entry :179-180) and truncates
// the x index once (:647); only the y index (:648) is per candidate. The beam
// is wave-uniform (scalar load). The loop body has no branches: all KT loads
// of a beam are in flight together.
//
// INT mode: cells are read from an exact fixed-point copy holding
// (value - outside) * 2^E through a buffer descriptor; an out-of-grid offset
// fails the hardware range check and reads 0, i.e. exactly `outside`, which is
// added back as n_used * outside * 2^E at the end. Sums run in 32-bit chunks
// folded into 64-bit; csm_set_grid enables the mode only when that integer
// sum equals the reference's sequential fp64 sum bit for bit.
template <int KT, bool INT, bool BEST>
__global__ __launch_bounds__(64) void score_cols_kernel(
    LevelWork L, const ScanWork* __restrict__ scans, const double2* __restrict__ pts,
    const AngleEntry* __restrict__ angles, double* __restrict__ out,
    BestPartial* __restrict__ partials) {
  const int bid = dev::xcd_remap(blockIdx.x, gridDim.x);
  dev::clear_word(L);
  const int win = bid / L.blocks_per_scan;
  const int r = bid - win * L.blocks_per_scan;
  const int cb = r / L.ktiles;
  const int kt = r - cb * L.ktiles;
  const ScanWork S = scans[win];
  const int lane = threadIdx.x;
  const int col = cb * 64 + lane;
  const bool valid = col < L.n_cols;
  const int colc = valid ? col : 0;
  const int a = colc / L.n_space;
  const int j = colc - a * L.n_space;
  const AngleEntry ae = angles[S.angle_off + a];
  const double x = S.x0 + j * L.step_cells;  // :569
  const int k0 = kt * KT;
  double y[KT];
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) y[kk] = S.y0 + (k0 + kk) * L.step_cells;  // :572
  const int sx = L.size_x, sy = L.size_y;
  const int64_t gofs = (int64_t)S.grid_index * L.grid_stride;
  const double2* __restrict__ P = pts + S.pts_off;
  const int step = S.step;
  const int n_used = S.n_used;
  double accd[KT];
  int64_t acci[KT];
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) {
    accd[kk] = 0.0;
    acci[kk] = 0;
  }
  if (INT) {
    const int32_t* gi = L.gridi + (int64_t)S.grid_index * L.gridi_stride;
    const __amdgpu_buffer_rsrc_t rsrc = dev::uniform_rsrc(gi, (int)(L.gridi_stride * 4));
    const int sx4 = L.pitch * 4;  // row stride of gridi (bytes)
    // Cells of beam b for every row of this lane (KT buffer loads in flight).
    // The host guarantees |gy| * 4 * pitch < 2^30 for every candidate of the
    // window (run_windows), so gy * sx4 never wraps: a row outside [0, sy)
    // gives an offset < 0 or >= 4*pitch*sy, and an x outside [0, sx) adds -2^30;
    // both fail the descriptor's range check and read 0 (= `outside`).
    auto load_beam = [&](int b, int32_t (&v)[KT]) {
      const double2 p = P[(int64_t)b * step];
      const double lx = ae.cosine * p.x - ae.sine * p.y;
      const double ly = ae.sine * p.x + ae.cosine * p.y;
      const int gx = (int)((lx + x) + 0.5);
      const int gx4 = ((unsigned)gx < (unsigned)sx) ? gx * 4 : -(1 << 30);
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        const int gy = (int)((ly + y[kk]) + 0.5);
        v[kk] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, __mul24(gy, sx4) + gx4, 0, 0);
      }
    };
    constexpr int kFold = 32;  // 32 * 2^26 <= 2^31: int32 chunk sums cannot overflow
    // two register sets, beams alternate between them: beam b+1's loads are
    // in flight while beam b is summed, with no register copies in between
    int32_t va[KT], vb[KT];
    load_beam(0, va);
    for (int base = 0; base < n_used; base += kFold) {
      const int nb = min(kFold, n_used - base);
      int32_t part[KT];
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) part[kk] = 0;
      for (int b = 0; b < nb; b += 2) {
        load_beam(min(base + b + 1, n_used - 1), vb);
        // keep the sums below the next beam's loads: the waits then leave
        // those KT loads in flight (vmcnt(KT)) instead of draining them
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) part[kk] += va[kk];
        load_beam(min(base + b + 2, n_used - 1), va);
        __builtin_amdgcn_sched_barrier(0);
        if (b + 1 < nb) {
#pragma unroll
          for (int kk = 0; kk < KT; ++kk) part[kk] += vb[kk];
        }
      }
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) acci[kk] += part[kk];
      // kFold is even, so every chunk but the last ends with va holding beam
      // base + kFold, the next chunk's first; only the last chunk can be odd.
    }
  } else {
    const float* __restrict__ gf = L.grid + gofs;
    const float outside = L.outside;
    auto load_beam = [&](int b, float (&v)[KT]) {
      const double2 p = P[(int64_t)b * step];
      const double lx = ae.cosine * p.x - ae.sine * p.y;
      const double ly = ae.sine * p.x + ae.cosine * p.y;
      const int gx = (int)((lx + x) + 0.5);
      const bool inx = (unsigned)gx < (unsigned)sx;
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        const int gy = (int)((ly + y[kk]) + 0.5);
        const bool inb = inx & ((unsigned)gy < (unsigned)sy);
        const float g = gf[inb ? gy * sx + gx : 0];
        v[kk] = inb ? g : outside;  // :651
      }
    };
    float v[KT];
    load_beam(0, v);
    for (int b = 0; b < n_used; ++b) {
      float vn[KT];
      load_beam(min(b + 1, n_used - 1), vn);
#pragma unroll
      for (int kk = 0; kk < KT; ++kk) {
        accd[kk] += (double)v[kk];  // :652, beam order
        v[kk] = vn[kk];
      }
    }
  }
  const int krem = min(KT, L.n_space - k0);
  dev::ScoreSink<BEST> sink;
#pragma unroll
  for (int kk = 0; kk < KT; ++kk) {
    if (kk < krem && valid) {
      const double acc = INT ? dev::fixed_point_acc(L, acci[kk], n_used) : accd[kk];
      sink.add(L, S, out, ((int64_t)a * L.n_space + j) * L.n_space + (k0 + kk),
               dev::penalized(L, S, acc, x, y[kk], ae.angle));
    }
  }
  // all mode ends with the stores: a block's lanes span angles, so there is no
  // fused finish here (level_decide never sets tail.on for this kernel)
  if constexpr (BEST) sink.done(L, S, angles, out, a, partials + (int64_t)win * L.blocks_per_scan + r, nullptr, nullptr);
}

// ---- v4: row-segment kernel, LDS-DMA staging (INT mode) --------------------
// For one beam and one angle the endpoint cells of a window's candidates form
// a separable set: ix depends only on the x step j, iy only on the y step k
// (:647-648). With lane (theta, r) of an angle group of NS lanes:
//   * the group's NS grid rows iy_r are each needed over the same short x-span
//     [xs, xs + SEG) (SEG = 4*SQ cells > (n_space-1)*f + 1, chosen by the host),
//     so a wave fetches its R = G*NS row segments as R*SQ 16-byte pieces; the
//     pieces are dealt to lanes row-major (lane l of load instruction i takes
//     piece 64*i + l), so one instruction covers ~64/SQ whole row segments and
//     touches few cache lines (a lane-per-row deal made every lane hit its own
//     line: 64 lines per instruction, measured slower than v2). Each piece's
//     row address comes from its owner lane by ds_bpermute, and the pieces are
//     parked in an LDS tile, one row per segment;
//   * lane (theta, j = r) computes its exact ix_r (reference arithmetic) and
//     reads column ix_r - xs of each of its group's NS tile rows: NS LDS reads
//     at immediate offsets.
// Per beam a wave issues ceil(R*SQ/64) gathers for R*NS candidates (v2: NS
// gathers for 64 candidates; TA-busy ~85% there, profiles/r01). A cell outside
// the grid reads 0 (= `outside`, pre-subtracted): rows through the buffer range
// check, x through a zero pad column of the tile. A lane whose x-span ever
// exceeds SEG (impossible for the host's SEG; kept as a guard) is recomputed
// exactly after the loop.
//
// The 16-byte pieces go straight into LDS by global_load_lds_dwordx4 (dest =
// wave-uniform base + 16 * lane): no VGPR staging and no ds_write_b128 (13
// LDS cycles each, the largest LDS cost of r01's register-staged form). Pieces are dealt row-major, so the LDS image is [row][SEG] with rows
// contiguous; beams alternate between two images (DMA of beam b+1 in flight
// while beam b is summed, counted vmcnt). DMA has no range check: rows outside
// the grid point at the zero row the host appends to gridi, columns outside
// the grid read a zero block.
// BS waves per block split a window's beams into BS contiguous ranges (low
// wave counts per launch otherwise: the super-fine level is one wave per
// window); their integer sums meet in LDS, exact in any order.
template <int NS, int SQ, bool BEST, int BS>
__global__ __launch_bounds__(64 * BS) void score_rowsd_kernel(
    LevelWork L, const ScanWork* __restrict__ scans, const double2* __restrict__ pts,
    const AngleEntry* __restrict__ angles, double* __restrict__ out,
    BestPartial* __restrict__ partials) {
  constexpr int G = 64 / NS;           // angle groups per wave
  constexpr int R = G * NS;            // row segments per beam
  constexpr int SEG = 4 * SQ;          // cells per row segment
  constexpr int NP = R * SQ;           // 16-byte pieces per beam
  constexpr int NI = (NP + 63) / 64;   // DMA instructions per beam
  constexpr int IMG = NI * 256;        // ints per image
  typedef __attribute__((address_space(3))) int32_t lds_i32;
  // two images as distinct objects, so the compiler's LDS-DMA wait tracking
  // can tell a read of one from the DMA still writing the other
  __shared__ __attribute__((aligned(16))) int32_t img0_s[BS * IMG];
  __shared__ __attribute__((aligned(16))) int32_t img1_s[BS * IMG];
  __shared__ __attribute__((aligned(16))) int32_t img2_s[BS * IMG];
  __shared__ __attribute__((aligned(16))) int32_t zblk[NS * SEG];
  __shared__ int64_t xsum[(BS - 1) * 64 * NS + 1];  // waves 1.. -> wave 0
  const int bid = dev::xcd_remap(blockIdx.x, gridDim.x);
  dev::clear_word(L);
  const int win = bid / L.blocks_per_scan;
  const int blk = bid - win * L.blocks_per_scan;
  const ScanWork S = scans[win];
  const int lane = BS > 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int wv = BS > 1 ? (int)(threadIdx.x >> 6) : 0;  // BS == 1: images at fixed LDS addresses
  int32_t* const img0 = img0_s + wv * IMG;
  int32_t* const img1 = img1_s + wv * IMG;
  int32_t* const img2 = img2_s + wv * IMG;
  const int g = lane / NS;
  // idle lanes (g >= G) shadow lane (G-1, NS-1): identical LDS addresses
  // broadcast instead of adding bank conflicts
  const int ge = g < G ? g : G - 1;
  const int r = g < G ? lane - g * NS : NS - 1;
  const int a_raw = blk * G + ge;
  const bool valid = (g < G) && (a_raw < L.n_angles);
  const int a = a_raw < L.n_angles ? a_raw : 0;
  const AngleEntry ae = angles[S.angle_off + a];
  const double f = L.step_cells;
  const double x_0 = S.x0 + 0 * f;  // :569 at j = 0
  const double x_r = S.x0 + r * f;  // :569 at j = r
  const double y_r = S.y0 + r * f;  // :572 at k = r
  const int sx = L.size_x, sy = L.size_y;
  const int pitch = L.pitch;
  const int xs_max = sx - SEG;  // host: sx >= SEG
  const double2* __restrict__ P = pts + S.pts_off;
  const int step = S.step;
  const int n_used = S.n_used;
  const int b_lo = (int)((int64_t)n_used * wv / BS);  // this wave's beams
  const int b_hi = (int)((int64_t)n_used * (wv + 1) / BS);
  const int32_t* gi = L.gridi + (int64_t)S.grid_index * L.gridi_stride;
  const __amdgpu_buffer_rsrc_t rsrc = dev::uniform_rsrc(gi, (int)(L.gridi_stride * 4));
  const int pitch4 = pitch * 4;
  const int zero_off = sy * pitch4;  // byte offset of the appended zero row

  int src4[NI], qofs[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int p = i * 64 + lane;
    const bool act = p < NP;
    const int rho = act ? p / SQ : 0;
    src4[i] = rho * 4;
    qofs[i] = act ? 16 * (p - rho * SQ) : -1;  // bytes into the segment; -1: idle piece
  }
  for (int t = lane; t < NS * SEG; t += 64) zblk[t] = 0;
  __syncthreads();

  // Beam points, 64 at a time in registers (lane l holds beam pbase + l) and
  // broadcast by readlane: no scalar load (and its lgkmcnt(0) drain of the
  // LDS queue) per beam.
  double2 pw = P[(int64_t)max(0, min(b_lo + lane, b_hi - 1)) * step];
  int pbase = b_lo;
  auto point = [&](int b) {
    const int l = b - pbase;
    double2 p;
    p.x = dev::bcast_lane(pw.x, l);
    p.y = dev::bcast_lane(pw.y, l);
    return p;
  };

  auto image = [&](int buf) -> int32_t* { return buf == 0 ? img0 : (buf == 1 ? img1 : img2); };
  // Beam b into image buf: issue this lane's DMA pieces; return the LDS byte
  // address of this lane's column in its group's k = 0 row.
  auto prep = [&](int b, int buf, lds_i32*& rd, bool& bad) {
    const double2 p = point(b);
    const double lx = ae.cosine * p.x - ae.sine * p.y;  // :179
    const double ly = ae.sine * p.x + ae.cosine * p.y;  // :180
    const int ix0 = (int)((lx + x_0) + 0.5);
    const int ixr = (int)((lx + x_r) + 0.5);
    const int iyr = (int)((ly + y_r) + 0.5);
    const int xs = min(max(ix0, 0), xs_max);
    const int rowoff = ((unsigned)iyr < (unsigned)sy) ? __mul24(iyr, pitch4) + xs * 4 : zero_off;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int o = __builtin_amdgcn_ds_bpermute(src4[i], rowoff);
      dev::buffer_load_lds16(rsrc, (lds_i32*)(image(buf) + i * 256), qofs[i] < 0 ? zero_off : o + qofs[i]);
    }
    const int pos = ixr - xs;
    const bool inx = (unsigned)ixr < (unsigned)sx;
    bad |= inx & ((unsigned)pos >= (unsigned)SEG);
    lds_i32* row0 = (lds_i32*)(image(buf) + ge * NS * SEG);
    rd = inx ? row0 + pos : (lds_i32*)&zblk[0];
  };
  // The reads are inline asm: hipcc's wait insertion treats every LDS read as
  // aliasing any LDS-DMA in flight and drains vmcnt(0), serialising the
  // pipeline; the explicit vmcnt(NI) before these reads is the real fence.
  auto consume = [&](const lds_i32* rd, int32_t (&part)[NS]) {
    typedef int32_t v2i __attribute__((ext_vector_type(2)));
    v2i w[(NS + 1) / 2];  // rows 2h, 2h+1; untouched until the lgkmcnt(0) below
    const uint32_t a = (uint32_t)(uintptr_t)rd;
#pragma unroll
    for (int h = 0; h < (NS + 1) / 2; ++h) {
      const int k = 2 * h;
      if (k + 1 < NS && (k + 1) * SEG <= 255) {  // two rows per instruction (dword offsets)
        asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3"
                     : "=v"(w[h]) : "v"(a), "i"(k * SEG), "i"((k + 1) * SEG));
      } else if (k + 1 < NS) {
        asm volatile("ds_read_b32 %0, %2 offset:%3\n\tds_read_b32 %1, %2 offset:%4"
                     : "=&v"(w[h].x), "=&v"(w[h].y) : "v"(a), "i"(k * SEG * 4), "i"((k + 1) * SEG * 4));
      } else {
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(w[h].x) : "v"(a), "i"(k * SEG * 4));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int h = 0; h < (NS + 1) / 2; ++h) {
      asm volatile("" : "+v"(w[h]));
      part[2 * h] += w[h].x;
      if (2 * h + 1 < NS) part[2 * h + 1] += w[h].y;
    }
  };

  int64_t acci[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acci[k] = 0;
  bool bad = false;
  // Three images: beam b is summed while the DMAs of b+1 and b+2 are in
  // flight (vmcnt(2*NI)). Chunks of 30 beams keep beam -> image static
  // (30 * (2^26 - 1) < 2^31, ensure_int_grid).
  constexpr int kFold = 30;
  constexpr short kWait2 = (short)(0xF70 | (2 * NI));  // needs 2*NI < 16
  static_assert(2 * NI < 16, "vmcnt field");
  lds_i32 *r0 = nullptr, *r1 = nullptr, *r2 = nullptr;
  if (b_hi > b_lo) {
    prep(b_lo, 0, r0, bad);
    prep(min(b_lo + 1, b_hi - 1), 1, r1, bad);
  }
  for (int base = b_lo; base < b_hi; base += kFold) {
    const int nb = min(kFold, b_hi - base);
    if (base != pbase) {  // this chunk preps beams base+2 .. base+kFold+1
      pbase = base;
      pw = P[(int64_t)min(base + lane, b_hi - 1) * step];
    }
    int32_t part[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) part[k] = 0;
    for (int b = 0; b < nb; b += 3) {
      prep(min(base + b + 2, b_hi - 1), 2, r2, bad);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(kWait2);
      __builtin_amdgcn_sched_barrier(0);
      consume(r0, part);
      __builtin_amdgcn_sched_barrier(0);
      prep(min(base + b + 3, b_hi - 1), 0, r0, bad);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(kWait2);
      __builtin_amdgcn_sched_barrier(0);
      if (b + 1 < nb) consume(r1, part);
      __builtin_amdgcn_sched_barrier(0);
      prep(min(base + b + 4, b_hi - 1), 1, r1, bad);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(kWait2);
      __builtin_amdgcn_sched_barrier(0);
      if (b + 2 < nb) consume(r2, part);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) acci[k] += part[k];
  }
  __builtin_amdgcn_s_waitcnt(0xF70);  // vmcnt(0): no DMA outlives the workgroup
  if (bad) {  // guard (never taken for the host's SEG): exact per-cell recompute
#pragma unroll
    for (int k = 0; k < NS; ++k) acci[k] = 0;
    for (int b = b_lo; b < b_hi; ++b) {
      const double2 p = P[(int64_t)b * step];
      const double lx = ae.cosine * p.x - ae.sine * p.y;
      const double ly = ae.sine * p.x + ae.cosine * p.y;
      const int gx = (int)((lx + x_r) + 0.5);
      const bool inx = (unsigned)gx < (unsigned)sx;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int gy = (int)((ly + (S.y0 + k * f)) + 0.5);
        const bool in = inx && (unsigned)gy < (unsigned)sy;
        acci[k] += gi[in ? (int64_t)gy * pitch + gx : (int64_t)sy * pitch];
      }
    }
  }
  if constexpr (BS > 1) {  // the other waves' sums into wave 0
    if (wv > 0) {
#pragma unroll
      for (int k = 0; k < NS; ++k) xsum[((wv - 1) * NS + k) * 64 + lane] = acci[k];
    }
    __syncthreads();
    if (wv > 0) return;
#pragma unroll
    for (int w2 = 1; w2 < BS; ++w2)
#pragma unroll
      for (int k = 0; k < NS; ++k) acci[k] += xsum[((w2 - 1) * NS + k) * 64 + lane];
  }
  dev::ScoreSink<BEST> sink;  // wave 0 alone from here on
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    if (valid) {
      const double acc = dev::fixed_point_acc(L, acci[k], n_used);
      const double yk = S.y0 + k * f;  // :572
      sink.add(L, S, out, ((int64_t)a * NS + r) * NS + k, dev::penalized(L, S, acc, x_r, yk, ae.angle));
    }
  }
  // all mode ends with the stores: a wave holds several angles, so there is no
  // fused finish here (level_decide never sets tail.on for this kernel)
  if constexpr (BEST)
    sink.done(L, S, angles, out, a, partials + (int64_t)win * L.blocks_per_scan + blk, nullptr, nullptr);
}

__global__ __launch_bounds__(kBlock) void reduce_best_kernel(const BestPartial* __restrict__ in,
                                                             int32_t per, BestPartial* __restrict__ out) {
  __shared__ double red_s[kBlock / 64];
  __shared__ int64_t red_f[kBlock / 64];
  const int64_t w = blockIdx.x;
  double bs = -1.0e300;
  int64_t bf = INT64_MAX;
  for (int i = threadIdx.x; i < per; i += kBlock) {
    const BestPartial p = in[w * per + i];
    if (dev::better(p.score, p.flat, bs, bf)) {
      bs = p.score;
      bf = p.flat;
    }
  }
  dev::wave_best(bs, bf);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    red_s[wave] = bs;
    red_f[wave] = bf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBlock / 64; ++k)
      if (dev::better(red_s[k], red_f[k], bs, bf)) {
        bs = red_s[k];
        bf = red_f[k];
      }
    out[w] = BestPartial{bs, bf};
  }
}

}  // namespace

template <int KT>
static hipError_t launch_cols_kt(const LevelWork& L, const ScanWork* d_scans, const double2* d_pts,
                                 const AngleEntry* d_angles, double* d_out, BestPartial* d_partials,
                                 hipStream_t stream) {
  const int64_t nblk = (int64_t)L.blocks_per_scan * L.n_scans;
  if (nblk <= 0 || nblk > INT32_MAX) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nblk), block(64);
  if (d_partials) {
    if (L.int_mode)
      hipLaunchKernelGGL((score_cols_kernel<KT, true, true>), grid, block, 0, stream, L, d_scans, d_pts, d_angles, d_out, d_partials);
    else
      hipLaunchKernelGGL((score_cols_kernel<KT, false, true>), grid, block, 0, stream, L, d_scans, d_pts, d_angles, d_out, d_partials);
  } else {
    if (L.int_mode)
      hipLaunchKernelGGL((score_cols_kernel<KT, true, false>), grid, block, 0, stream, L, d_scans, d_pts, d_angles, d_out, d_partials);
    else
      hipLaunchKernelGGL((score_cols_kernel<KT, false, false>), grid, block, 0, stream, L, d_scans, d_pts, d_angles, d_out, d_partials);
  }
  return hipGetLastError();
}

hipError_t launch_score_cols(const LevelWork& L, const ScanWork* d_scans, const double* d_pts_raw,
                             const AngleEntry* d_angles, double* d_out, BestPartial* d_partials,
                             int kt, hipStream_t stream) {
  const double2* d_pts = reinterpret_cast<const double2*>(d_pts_raw);
#define CSM_KT_CASE(K) \
  case K: return launch_cols_kt<K>(L, d_scans, d_pts, d_angles, d_out, d_partials, stream);
  switch (kt) {
    CSM_KT_CASE(1) CSM_KT_CASE(2) CSM_KT_CASE(3) CSM_KT_CASE(4) CSM_KT_CASE(5) CSM_KT_CASE(6)
    CSM_KT_CASE(7) CSM_KT_CASE(8) CSM_KT_CASE(9) CSM_KT_CASE(10) CSM_KT_CASE(11)
    CSM_KT_CASE(12) CSM_KT_CASE(13) CSM_KT_CASE(14) CSM_KT_CASE(15) CSM_KT_CASE(16)
    default: return hipErrorInvalidValue;
  }
#undef CSM_KT_CASE
}

// Row-segment instantiations (n_space, SQ): the sim-YAML levels (13,4) (11,2)
// (3,1), param_config.h's coarse (9,5) and config 1's window (21,6) at 5 cm.
#define CSM_ROWS_LIST(X) X(13, 4) X(11, 2) X(3, 1) X(9, 5) X(21, 6)

int rows_pick_sq(int ns, int need_seg) {
#define CSM_ROWS_PICK(N, Q) \
  if (ns == N && 4 * Q >= need_seg) return Q;
  CSM_ROWS_LIST(CSM_ROWS_PICK)
#undef CSM_ROWS_PICK
  return 0;
}

// Waves per block of the LDS-DMA row kernel: launches of fewer than 4096
// blocks (the super-fine level: one block per window) split each window's
// beams over up to 8 waves, towards 16 waves per SIMD; at most 64 KB of LDS
// per block (three images and the cross-wave sums per wave). Measured on the
// fine level (6144 blocks), a 4-way split was 7% slower than none.
int rows_beam_split(int64_t blocks) {
  int bs = 1;
  if (blocks >= 4096) return 1;
  while (bs < 8 && blocks * bs < 16384) bs *= 2;
  return bs;
}
template <int NS, int SQ>
constexpr int rows_bs_cap() {
  constexpr int NP = (64 / NS) * NS * SQ;
  constexpr int IMG = (NP + 63) / 64 * 256;
  int bs = 8;
  while (bs > 1 && bs * (3 * IMG * 4 + NS * 64 * 8) > 64 * 1024) bs /= 2;
  return bs;
}
template <int NS, int SQ, int B>
hipError_t launch_rowsd(const LevelWork& L, const ScanWork* d_scans, const double2* d_pts,
                        const AngleEntry* d_angles, double* d_out, BestPartial* d_partials, dim3 grid,
                        hipStream_t stream) {
  if constexpr (B > rows_bs_cap<NS, SQ>()) {
    return launch_rowsd<NS, SQ, rows_bs_cap<NS, SQ>()>(L, d_scans, d_pts, d_angles, d_out, d_partials, grid,
                                                        stream);
  } else {
    if (d_partials)
      hipLaunchKernelGGL((score_rowsd_kernel<NS, SQ, true, B>), grid, dim3(64 * B), 0, stream, L, d_scans, d_pts,
                         d_angles, d_out, d_partials);
    else
      hipLaunchKernelGGL((score_rowsd_kernel<NS, SQ, false, B>), grid, dim3(64 * B), 0, stream, L, d_scans, d_pts,
                         d_angles, d_out, d_partials);
    return hipGetLastError();
  }
}

hipError_t launch_score_rows(const LevelWork& L, const ScanWork* d_scans, const double* d_pts_raw,
                             const AngleEntry* d_angles, double* d_out, BestPartial* d_partials,
                             int ns, int sq, hipStream_t stream) {
  const double2* d_pts = reinterpret_cast<const double2*>(d_pts_raw);
  const int64_t nblk = (int64_t)L.blocks_per_scan * L.n_scans;
  if (nblk <= 0 || nblk > INT32_MAX || !L.int_mode || L.size_x < 4 * sq) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nblk);
  const int bs = rows_beam_split(nblk);
#define CSM_ROWSD_LAUNCH(N, Q, B) \
  return launch_rowsd<N, Q, B>(L, d_scans, d_pts, d_angles, d_out, d_partials, grid, stream)
#define CSM_ROWS_CASE(N, Q)                     \
  if (ns == N && sq == Q) {                     \
    if (bs == 1) CSM_ROWSD_LAUNCH(N, Q, 1);     \
    if (bs == 2) CSM_ROWSD_LAUNCH(N, Q, 2);     \
    if (bs == 4) CSM_ROWSD_LAUNCH(N, Q, 4);     \
    CSM_ROWSD_LAUNCH(N, Q, 8);                  \
  }
  CSM_ROWS_LIST(CSM_ROWS_CASE)
#undef CSM_ROWS_CASE
#undef CSM_ROWSD_LAUNCH
  return hipErrorInvalidValue;
}

hipError_t launch_reduce_best(const BestPartial* d_partials, int32_t blocks_per_scan,
                              int32_t n_windows, BestPartial* d_out, hipStream_t stream) {
  if (n_windows <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(reduce_best_kernel, dim3(n_windows), dim3(kBlock), 0, stream, d_partials,
                     blocks_per_scan, d_out);
  return hipGetLastError();
}

}  // namespace csm
