// csm_deskew.cpp — motion de-skew of raw laser scans: csm_deskew_plan and
// csm_deskew_ranges on the host (csm_deskew_host.hpp: LaserDataProcessor::Process,
// laser_data_processor.cpp:43-314, operation for operation),
// csm_load_ranges_deskewed / _async on the device (csm_deskew.hip) in front of
// the ranges ingest (csm_ranges.cpp), and the test hooks csm_atan2_device /
// csm_sqrt_device.
//
// The device path's split (include/csm.h): the host does the interior closing
// beams, whose second pass reads the exact atan2 of the first, and every
// division and sincos that is per segment, per scan or per laser; the kernel
// does every other beam and flags the scans in which a beam's bin quotient is
// within 2^-30 of a nonzero integer. take_staged hands flagged scans to
// repair_deskewed, which de-skews them with the host restatement, uploads the
// rows and runs the ingest again. Without the device sincos (the libm table
// did not pass, CSM_DEVICE_TRIG=0) or with a mid yaw outside its domain, the
// whole batch is de-skewed on the host and goes through the plain ranges path.
#include <cstring>
#include <vector>

#include "csm_deskew_host.hpp"
#include "csm_host.hpp"
#include "csm_ranges_host.hpp"

namespace csmh {
namespace {

namespace dk = csm::deskew;

constexpr float kMinIncrement = 0.000244140625f;  // 2^-12: the guard's bound on the quotient's error
constexpr float kMaxAngleMin = 8.0f;              // ... and on its magnitude (a LaserScan's is at most pi)
constexpr double kYawDomain = 1.0e8;              // inside libm::sincos_device_ok's 105414350, with room for rounding

// The (cos, sin) of the float-arithmetic beam angles on the device and on the
// host, keyed and made ready as the laser table (csm_ranges.cpp).
int ensure_deskew_table(csm_ctx* c, const csm_laser& L, bool device) {
  uint32_t amin, ainc;
  std::memcpy(&amin, &L.angle_min, sizeof(amin));
  std::memcpy(&ainc, &L.angle_increment, sizeof(ainc));
  const bool same = c->deskew_tab_beams == L.n_beams && c->deskew_tab_amin == amin && c->deskew_tab_ainc == ainc &&
                    c->deskew_tab_host.size() == (size_t)L.n_beams * 2;
  if (same && (c->deskew_tab_ready || !device)) return CSM_OK;
  c->deskew_tab_ready = false;
  if (!same) {
    c->deskew_tab_host.resize((size_t)L.n_beams * 2);
    dk::beam_trig_table(L, c->deskew_tab_host.data());
    c->deskew_tab_beams = L.n_beams;
    c->deskew_tab_amin = amin;
    c->deskew_tab_ainc = ainc;
  }
  if (!device) return CSM_OK;
  const size_t bytes = c->deskew_tab_host.size() * sizeof(double);
  hipError_t e;
  // (the stream is drained before a larger table replaces the buffer a queued
  // batch's kernel may still read)
  if (bytes > c->deskew_tab.cap && (e = hipStreamSynchronize(c->stage_stream)) != hipSuccess)
    return c->hip_fail(e, "hipStreamSynchronize(stage)");
  if ((e = c->deskew_tab.ensure(bytes)) != hipSuccess) return c->hip_fail(e, "hipMalloc(deskew table)");
  if ((e = hipMemcpyAsync(c->deskew_tab.p, c->deskew_tab_host.data(), bytes, hipMemcpyHostToDevice,
                          c->stage_stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stage_stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(deskew table)");
  c->deskew_tab_ready = true;
  return CSM_OK;
}

// Scans [0, n) of `which` (null: every scan) de-skewed on the pool into rows
// (scan which[k], or k, at row k).
void host_deskew(csm_ctx* c, const csm_laser& L, const float* ranges, const int64_t* seg_off, const int32_t* seg_close,
                 const double* poses, const int32_t* which, int32_t n, float* rows) {
  const double* cs = c->deskew_tab_host.data();
  c->parallel_for(n, c->host_threads, [&](int k) {
    const int32_t s = which ? which[k] : k;
    std::vector<double> r((size_t)L.n_beams), a((size_t)L.n_beams);
    dk::deskew_batch_scan(L, cs, s, ranges, seg_off, seg_close, poses, r.data(), a.data(),
                          rows + (int64_t)k * L.n_beams);
  });
}

int queue_deskewed(csm_ctx* c, const csm_laser* laser, int32_t n_scans, const float* ranges, double factor,
                   const int64_t* seg_off, const int32_t* seg_close, const double* poses) {
  if (!laser) return c->fail(CSM_ERR_INVALID_ARG, "null laser");
  const csm_laser L = *laser;
  double threshold = 0.0;
  if (!csm::laser_threshold(L, &threshold))
    return c->fail(CSM_ERR_INVALID_ARG, "bad laser (n_beams <= 0, range_min >= range_max or a field not finite)");
  if (n_scans < 0 || (n_scans > 0 && !ranges)) return c->fail(CSM_ERR_INVALID_ARG, "bad ranges");
  if (!dk::plan_valid(L, n_scans, seg_off, seg_close, poses))
    return c->fail(CSM_ERR_INVALID_ARG,
                   "bad de-skew plan (n_beams < 2, angle_increment == 0, a pose not finite, closes not strictly "
                   "increasing or not ending at n_beams - 1)");
  // the guard's bounds: |D - angle_min| < 16 and |1 / angle_increment| <= 2^12 keep the quotient below 2^16 and
  // what atan2's 2^-44, the subtraction's and the division's roundings move it by below 2^-32 + 2^-38 + 2^-38
  if (L.n_beams > csm::kDeskewMaxBeams || !(std::fabs(L.angle_increment) >= kMinIncrement) ||
      !(std::fabs(L.angle_min) <= kMaxAngleMin))
    return c->fail(CSM_ERR_UNSUPPORTED,
                   "de-skew on the device needs n_beams <= 8000, |angle_increment| >= 2^-12 and |angle_min| <= 8");
  int st;
  csm_ctx::Staged* slot = nullptr;
  if ((st = open_stage_slot(c, &slot)) != CSM_OK) return st;
  csm_ctx::Staged& S = *slot;
  hipError_t e;
  hipStream_t s = c->stage_stream;
  const int64_t n_seg = seg_off[n_scans];
  const int64_t n_ranges = (int64_t)n_scans * L.n_beams;
  const size_t range_bytes = (size_t)n_ranges * sizeof(float);
  bool device = c->device_trig && libm_sincos_table() != nullptr;
  if ((st = ensure_deskew_table(c, L, device)) != CSM_OK) return st;
  if ((st = ranges_slot_prepare(c, S, L, n_scans)) != CSM_OK) return st;

  // the tables: DeskewScan[n_scans] then DeskewSeg[n_seg], pinned
  const size_t plan_bytes = ((size_t)n_scans + (size_t)n_seg) * 64;
  if (device) {
    if ((e = S.plan_h.ensure(std::max<size_t>(plan_bytes, 64))) != hipSuccess)
      return c->hip_fail(e, "hipHostMalloc(deskew plan)");
    csm::DeskewScan* hs = (csm::DeskewScan*)S.plan_h.p;
    csm::DeskewSeg* hg = (csm::DeskewSeg*)(hs + n_scans);
    const double* cs = c->deskew_tab_host.data();
    int out_of_domain = 0;
    c->parallel_for(n_scans, c->host_threads, [&](int sc) {
      const int64_t k0 = seg_off[sc];
      const int32_t K = (int32_t)(seg_off[sc + 1] - k0);
      csm::DeskewScan& H = hs[sc];
      std::memset(&H, 0, sizeof(H));
      H.seg_off = k0;
      H.n_seg = K;
      if (K == 0) return;
      const double* P = poses + (k0 + sc) * 3;
      const int32_t* close = seg_close + k0;
      const dk::T2 base = dk::base_transform(P[0], P[1], -P[2]);
      H.r00 = base.r00, H.r01 = base.r01, H.r10 = base.r10, H.r11 = base.r11, H.tx = base.tx, H.ty = base.ty;
      const float* in = ranges + (int64_t)sc * L.n_beams;
      bool bad = false;
      int32_t first = 0;
      for (int32_t k = 0; k < K; ++k) {
        const dk::Segment g = dk::make_segment(P + 3 * k, P + 3 * (k + 1), first, close[k] - first + 1);
        csm::DeskewSeg& G = hg[k0 + k];
        G.x0 = g.x0, G.det_x = g.det_x, G.y0 = g.y0, G.det_y = g.det_y, G.ya = g.ya, G.det_yaw = g.det_yaw;
        G.first = g.first, G.cnt = g.cnt;
        G.host_bin = -2;
        G.host_range = 0.0f;
        // every mid yaw lies between the segment's ends (up to rounding)
        const double yend = g.ya + g.det_yaw * (double)(g.cnt - 1);
        if (!(std::fabs(g.ya) < kYawDomain && std::fabs(yend) < kYawDomain)) bad = true;
        if (k < K - 1) dk::closing_beam(L, cs, in, k, close, P, base, &G.host_bin, &G.host_range);
        first = close[k];
      }
      if (bad) __atomic_store_n(&out_of_domain, 1, __ATOMIC_RELAXED);
    });
    if (out_of_domain) device = false;
  }

  if (!device) {  // fail closed: the whole batch on the host, then the plain ranges path
    if ((e = S.rows_h.ensure(std::max<size_t>(range_bytes, 4))) != hipSuccess)
      return c->hip_fail(e, "hipHostMalloc(deskew rows)");
    host_deskew(c, L, ranges, seg_off, seg_close, poses, nullptr, n_scans, (float*)S.rows_h.p);
    if (range_bytes > 0 &&
        (e = hipMemcpyAsync(S.ranges.p, S.rows_h.p, range_bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
      return c->hip_fail(e, "csm_load_ranges_deskewed(upload)");
    if ((st = ranges_ingest(c, S, L, threshold, n_scans, factor)) != CSM_OK) return st;
    c->account_count("deskew:host_batches", 1);
    commit_staged(c, S, csm_ctx::StagedKind::kRanges, n_scans);  // nothing left to repair
    return CSM_OK;
  }

  const size_t flag_bytes = ((size_t)n_scans + 1) * sizeof(int32_t);
  if ((e = S.raw.ensure(std::max<size_t>(range_bytes, 4))) != hipSuccess ||
      (e = S.plan_dev.ensure(std::max<size_t>(plan_bytes, 64))) != hipSuccess ||
      (e = S.flags_dev.ensure(flag_bytes)) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(deskew)");
  if ((e = S.flags_h.ensure(flag_bytes)) != hipSuccess) return c->hip_fail(e, "hipHostMalloc(deskew flags)");
  if ((st = ensure_trig_table(c, s)) != CSM_OK) return st;
  Event t0, t1;
  bool timed = c->profiling && !c->profile_first_level && t0.create(hipEventDefault) == hipSuccess &&
               t1.create(hipEventDefault) == hipSuccess;
  if ((e = hipMemsetAsync(S.flags_dev.p, 0, flag_bytes, s)) != hipSuccess ||
      (range_bytes > 0 && (e = hipMemcpyAsync(S.raw.p, ranges, range_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) ||
      (plan_bytes > 0 && (e = hipMemcpyAsync(S.plan_dev.p, S.plan_h.p, plan_bytes, hipMemcpyHostToDevice, s)) !=
                             hipSuccess))
    return c->hip_fail(e, "csm_load_ranges_deskewed(upload)");
  if (timed && hipEventRecord(t0, s) != hipSuccess) timed = false;
  const csm::DeskewScan* ds = (const csm::DeskewScan*)S.plan_dev.p;
  if ((e = csm::launch_deskew((const float*)S.raw.p, n_scans, L.n_beams, L.angle_min, L.angle_increment, ds,
                              (const csm::DeskewSeg*)(ds + n_scans), (const double*)c->deskew_tab.p,
                              (const double*)c->trig_tab.p, (float*)S.ranges.p, (int32_t*)S.flags_dev.p, s)) !=
      hipSuccess)
    return c->hip_fail(e, "deskew_kernel");
  if (timed && hipEventRecord(t1, s) != hipSuccess) timed = false;
  if ((e = hipMemcpyAsync(S.flags_h.p, S.flags_dev.p, flag_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
    return c->hip_fail(e, "csm_load_ranges_deskewed(flags)");
  if ((st = ranges_ingest(c, S, L, threshold, n_scans, factor)) != CSM_OK) return st;
  if (timed && hipEventSynchronize(t1) == hipSuccess) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t0, t1) == hipSuccess) c->account("deskew", ms, 2.0 * (double)range_bytes, 0.0);
  }
  // what a repair needs (take_staged): the plan is the caller's only during this call
  S.laser = L;
  S.factor = factor;
  S.threshold = threshold;
  S.src_ranges = ranges;
  S.seg_off.assign(seg_off, seg_off + n_scans + 1);
  S.seg_close.assign(seg_close, seg_close + n_seg);
  if (n_seg > 0)
    S.seg_poses.assign(poses, poses + (n_seg + n_scans) * 3);
  else
    S.seg_poses.clear();
  commit_staged(c, S, csm_ctx::StagedKind::kDeskewed, n_scans);
  return CSM_OK;
}

}  // namespace

// take_staged, after S.ready: the scans the kernel flagged are de-skewed by the
// host restatement, their rows uploaded over the device's, and the ingest run
// again (its results replace the first run's before anything has read them).
int repair_deskewed(csm_ctx* c, csm_ctx::Staged& S) {
  const int32_t n_scans = S.batch.n_scans;
  const int32_t* flags = (const int32_t*)S.flags_h.p;
  const int32_t total = n_scans > 0 ? flags[n_scans] : 0;
  c->account_count("deskew:host_scans", total);
  if (total <= 0) return CSM_OK;
  const csm_laser& L = S.laser;
  std::vector<int32_t> which;
  which.reserve((size_t)total);
  for (int32_t s = 0; s < n_scans; ++s)
    if (flags[s]) which.push_back(s);
  hipError_t e;
  const size_t row_bytes = (size_t)L.n_beams * sizeof(float);
  if ((e = S.rows_h.ensure(which.size() * row_bytes)) != hipSuccess)
    return c->hip_fail(e, "hipHostMalloc(deskew rows)");
  int st;
  if ((st = ensure_deskew_table(c, L, false)) != CSM_OK) return st;
  host_deskew(c, L, S.src_ranges, S.seg_off.data(), S.seg_close.data(), S.seg_poses.data(), which.data(),
              (int32_t)which.size(), (float*)S.rows_h.p);
  hipStream_t s = c->stage_stream;
  for (size_t k = 0; k < which.size();) {  // runs of consecutive scans in one copy
    size_t k1 = k + 1;
    while (k1 < which.size() && which[k1] == which[k1 - 1] + 1) ++k1;
    if ((e = hipMemcpyAsync((float*)S.ranges.p + (int64_t)which[k] * L.n_beams,
                            (const float*)S.rows_h.p + (int64_t)k * L.n_beams, (k1 - k) * row_bytes,
                            hipMemcpyHostToDevice, s)) != hipSuccess)
      return c->hip_fail(e, "csm_load_ranges_deskewed(repair upload)");
    k = k1;
  }
  // (a batch queued since with another laser replaced the context's (cos, sin) table: this batch's again, behind
  // that batch's kernels on the stream; the slot's buffers are large enough already)
  if ((st = ranges_slot_prepare(c, S, L, n_scans)) != CSM_OK) return st;
  if ((st = ranges_ingest(c, S, L, S.threshold, n_scans, S.factor)) != CSM_OK) return st;
  if ((e = hipEventSynchronize(S.ready)) != hipSuccess) return c->hip_fail(e, "hipEventSynchronize(stage)");
  return CSM_OK;
}

// csm_atan2_device / csm_sqrt_device: one device function over n host doubles.
int unary_device(csm_ctx* c, const double* a, const double* b, int64_t n, double* out, bool is_atan2) {
  if (!c || n < 0 || (n > 0 && (!a || !out || (is_atan2 && !b)))) return CSM_ERR_INVALID_ARG;
  if (n == 0) return CSM_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;
  DevBuf da, db, dout;
  const size_t bytes = (size_t)n * sizeof(double);
  hipError_t e;
  if ((e = da.ensure_exact(bytes)) != hipSuccess || (e = dout.ensure_exact(bytes)) != hipSuccess ||
      (is_atan2 && (e = db.ensure_exact(bytes)) != hipSuccess))
    return c->hip_fail(e, "hipMalloc(test hook)");
  if ((e = hipMemcpyAsync(da.p, a, bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess ||
      (is_atan2 && (e = hipMemcpyAsync(db.p, b, bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess))
    return c->hip_fail(e, "hipMemcpyAsync(test hook)");
  e = is_atan2 ? csm::launch_atan2((const double*)da.p, (const double*)db.p, n, (double*)dout.p, c->stream)
               : csm::launch_sqrt((const double*)da.p, n, (double*)dout.p, c->stream);
  if (e != hipSuccess) return c->hip_fail(e, "test hook kernel");
  if ((e = hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(test hook back)");
  return CSM_OK;
}

}  // namespace csmh

using namespace csmh;

extern "C" {

int csm_deskew_plan(int32_t n_beams, double start_sec, double end_sec, double odom_interpolation_time,
                    int32_t* seg_close, double* lookup_sec, int32_t capacity, int32_t* n_segments) {
  return csm::deskew::plan(n_beams, start_sec, end_sec, odom_interpolation_time, seg_close, lookup_sec, capacity,
                           n_segments);
}

int csm_deskew_ranges(const csm_laser* laser, int32_t n_scans, const float* ranges, const int64_t* seg_offsets,
                      const int32_t* seg_close, const double* poses_xyyaw, float* ranges_out) {
  if (!laser || n_scans < 0 || (n_scans > 0 && (!ranges || !ranges_out))) return CSM_ERR_INVALID_ARG;
  if (!csm::deskew::plan_valid(*laser, n_scans, seg_offsets, seg_close, poses_xyyaw)) return CSM_ERR_INVALID_ARG;
  std::vector<double> cs((size_t)laser->n_beams * 2);
  csm::deskew::beam_trig_table(*laser, cs.data());
  csm::deskew::deskew_scans(*laser, cs.data(), 0, n_scans, ranges, seg_offsets, seg_close, poses_xyyaw, ranges_out);
  return CSM_OK;
}

int csm_load_ranges_deskewed_async(csm_ctx* c, const csm_laser* laser, int32_t n_scans, const float* ranges,
                                   double factor, const int64_t* seg_offsets, const int32_t* seg_close,
                                   const double* poses_xyyaw) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return queue_deskewed(c, laser, n_scans, ranges, factor, seg_offsets, seg_close, poses_xyyaw);
}

int csm_load_ranges_deskewed(csm_ctx* c, const csm_laser* laser, int32_t n_scans, const float* ranges, double factor,
                             const int64_t* seg_offsets, const int32_t* seg_close, const double* poses_xyyaw) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int st;
  if ((st = unload_batch(c)) != CSM_OK) return st;
  // through a staging slot (none is queued now), taken at once
  if ((st = queue_deskewed(c, laser, n_scans, ranges, factor, seg_offsets, seg_close, poses_xyyaw)) != CSM_OK)
    return st;
  return take_staged(c);
}

int csm_atan2_device(csm_ctx* c, const double* y, const double* x, int64_t n, double* out) {
  return unary_device(c, y, x, n, out, true);
}

int csm_sqrt_device(csm_ctx* c, const double* x, int64_t n, double* out) {
  return unary_device(c, x, nullptr, n, out, false);
}

}  // extern "C"
