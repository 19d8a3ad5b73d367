// csm_ranges.cpp — raw laser ranges in (csm_laser_range_threshold,
// csm_ranges_to_points on the host; csm_load_ranges, csm_load_ranges_async on
// the device).
//
// The reference hands its matcher a sensor_msgs/LaserScan: the endpoints are
// built by SlamNode::BuildRangeDataContainer (roborts_slam_node.cpp:290-311)
// and scaled by RangeDataContainer::CreateFrom (sensor_data_manager.h:99-115).
// The device path uploads the float32 ranges (a quarter of the fp64 points'
// bytes) into a staging slot and builds the same points there
// (csm_ranges.hip); everything downstream of the slot is csm_load_scans_async's.
#include <cstring>
#include <vector>

#include "csm_host.hpp"
#include "csm_ranges_host.hpp"

namespace csmh {
namespace {

// The laser's (cos a_i, sin a_i) table on the device, keyed on what it is
// computed from. Uploaded on stage_stream, so a batch already queued with
// another laser has read the old table before the copy runs; ready only once
// the copy was enqueued and the stream drained (the source is a local vector,
// and after a failed copy the next call uploads again).
int ensure_laser_table(csm_ctx* c, const csm_laser& L) {
  uint32_t amin, ainc;
  std::memcpy(&amin, &L.angle_min, sizeof(amin));
  std::memcpy(&ainc, &L.angle_increment, sizeof(ainc));
  if (c->laser_tab_ready && c->laser_tab_beams == L.n_beams && c->laser_tab_amin == amin &&
      c->laser_tab_ainc == ainc)
    return CSM_OK;
  c->laser_tab_ready = false;
  std::vector<double> cs((size_t)L.n_beams * 2);
  csm::laser_trig_table(L, cs.data());
  const size_t bytes = cs.size() * sizeof(double);
  hipError_t e;
  // (the stream is drained before a larger table replaces the buffer a queued
  // batch's kernels may still read)
  if (bytes > c->laser_tab.cap && (e = hipStreamSynchronize(c->stage_stream)) != hipSuccess)
    return c->hip_fail(e, "hipStreamSynchronize(stage)");
  if ((e = c->laser_tab.ensure(bytes)) != hipSuccess) return c->hip_fail(e, "hipMalloc(laser table)");
  if ((e = hipMemcpyAsync(c->laser_tab.p, cs.data(), bytes, hipMemcpyHostToDevice, c->stage_stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stage_stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(laser table)");
  c->laser_tab_beams = L.n_beams;
  c->laser_tab_amin = amin;
  c->laser_tab_ainc = ainc;
  c->laser_tab_ready = true;
  return CSM_OK;
}

// Profiling (csm_set_profiling 1): HIP-event times of the three ingest
// kernels of one batch, waited for here (the call is synchronous then).
struct IngestTimer {
  Event ev[4];
  bool on = false;
  explicit IngestTimer(bool want) {
    on = want;
    for (int i = 0; on && i < 4; ++i)
      if (ev[i].create(hipEventDefault) != hipSuccess) on = false;
  }
  void mark(int i, hipStream_t s) {
    if (on && hipEventRecord(ev[i], s) != hipSuccess) on = false;
  }
  void report(csm_ctx* c, double range_bytes, double point_bytes) {
    if (!on || hipEventSynchronize(ev[3]) != hipSuccess) return;
    static const char* const names[3] = {"ranges_count", "ranges_offsets", "ranges_points"};
    const double bytes[3] = {range_bytes, 0.0, range_bytes + point_bytes};
    for (int i = 0; i < 3; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) c->account(names[i], ms, bytes[i], 0.0);
    }
  }
};

}  // namespace

// A ranges batch's slot buffers (the ranges as float32, the counts, offsets
// and the most points the batch can keep) and the laser's table.
int ranges_slot_prepare(csm_ctx* c, csm_ctx::Staged& S, const csm_laser& L, int32_t n_scans) {
  int st;
  hipError_t e;
  if ((st = ensure_laser_table(c, L)) != CSM_OK) return st;
  const int64_t n_ranges = (int64_t)n_scans * L.n_beams;  // the most points the batch can keep
  const size_t range_bytes = (size_t)n_ranges * sizeof(float);
  const size_t point_bytes = (size_t)std::max<int64_t>(n_ranges, 1) * 2 * sizeof(double);
  const size_t off_bytes = ((size_t)n_scans + 1) * sizeof(int64_t);
  if ((e = S.ranges.ensure(std::max<size_t>(range_bytes, 4))) != hipSuccess ||
      (e = S.counts.ensure(((size_t)n_scans + 1) * sizeof(int32_t))) != hipSuccess ||
      (e = S.off_dev.ensure(off_bytes)) != hipSuccess || (e = S.batch.pts.ensure(point_bytes)) != hipSuccess ||
      (e = S.maxabs_dev.ensure(sizeof(unsigned long long))) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(stage)");
  if ((e = S.off_h.ensure(off_bytes)) != hipSuccess) return c->hip_fail(e, "hipHostMalloc(stage offsets)");
  return CSM_OK;
}

// The ingest of S.ranges (already enqueued on stage_stream): the points, their
// offsets and max |x| + |y|, copied down before S.ready.
int ranges_ingest(csm_ctx* c, csm_ctx::Staged& S, const csm_laser& L, double threshold, int32_t n_scans,
                  double factor) {
  hipError_t e;
  const int64_t n_ranges = (int64_t)n_scans * L.n_beams;
  const size_t range_bytes = (size_t)n_ranges * sizeof(float);
  const size_t off_bytes = ((size_t)n_scans + 1) * sizeof(int64_t);
  hipStream_t s = c->stage_stream;
  const double lo = (double)L.range_min;
  IngestTimer tm(c->profiling && !c->profile_first_level);
  // the slot's previous batch was matched by a call that has returned, so no
  // kernel reads its buffers any more. The points buffer is zeroed whole: the
  // kept count stays on the device, so points_maxabs_kernel runs over the
  // upper bound, and a zero point leaves its maximum as it is.
  if (n_ranges > 0 && (e = hipMemsetAsync(S.batch.pts.p, 0, (size_t)n_ranges * 2 * sizeof(double), s)) != hipSuccess)
    return c->hip_fail(e, "csm_load_ranges_async(memset)");
  tm.mark(0, s);
  if ((e = csm::launch_ranges_count((const float*)S.ranges.p, n_scans, L.n_beams, lo, threshold,
                                    (int32_t*)S.counts.p, s)) != hipSuccess)
    return c->hip_fail(e, "ranges_count_kernel");
  tm.mark(1, s);
  if ((e = csm::launch_ranges_offsets((const int32_t*)S.counts.p, n_scans, (int64_t*)S.off_dev.p, s)) != hipSuccess)
    return c->hip_fail(e, "ranges_offsets_kernel");
  tm.mark(2, s);
  if ((e = csm::launch_ranges_points((const float*)S.ranges.p, n_scans, L.n_beams, lo, threshold, factor,
                                     (const double*)c->laser_tab.p, (const int64_t*)S.off_dev.p, (double*)S.batch.pts.p,
                                     s)) != hipSuccess)
    return c->hip_fail(e, "ranges_points_kernel");
  tm.mark(3, s);
  if ((e = hipMemcpyAsync(S.off_h.p, S.off_dev.p, off_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = stage_maxabs_ready(c, S, n_ranges)) != hipSuccess)
    return c->hip_fail(e, "csm_load_ranges_async");
  if (tm.on && hipEventSynchronize(S.ready) == hipSuccess)  // the kept count is down: what the points pass wrote
    tm.report(c, (double)range_bytes, (double)((const int64_t*)S.off_h.p)[n_scans] * 2 * sizeof(double));
  return CSM_OK;
}

// csm_load_ranges_async once locked: the batch into the next free slot, all of
// it enqueued on stage_stream before S.ready. Nothing but this call's work
// writes the slot's buffers (the submit path parks a pending batch's points in
// a taken slot until the call that queues into it next).
int queue_ranges(csm_ctx* c, const csm_laser* laser, int32_t n_scans, const float* ranges, double factor) {
  if (!laser) return c->fail(CSM_ERR_INVALID_ARG, "null laser");
  const csm_laser L = *laser;
  double threshold = 0.0;
  if (!csm::laser_threshold(L, &threshold))
    return c->fail(CSM_ERR_INVALID_ARG, "bad laser (n_beams <= 0, range_min >= range_max or a field not finite)");
  if (n_scans < 0 || (n_scans > 0 && !ranges)) return c->fail(CSM_ERR_INVALID_ARG, "bad ranges");
  int st;
  csm_ctx::Staged* slot = nullptr;
  if ((st = open_stage_slot(c, &slot)) != CSM_OK) return st;
  csm_ctx::Staged& S = *slot;
  hipError_t e;
  if ((st = ranges_slot_prepare(c, S, L, n_scans)) != CSM_OK) return st;
  const size_t range_bytes = (size_t)n_scans * L.n_beams * sizeof(float);
  if (range_bytes > 0 && (e = hipMemcpyAsync(S.ranges.p, ranges, range_bytes, hipMemcpyHostToDevice,
                                             c->stage_stream)) != hipSuccess)
    return c->hip_fail(e, "csm_load_ranges_async(upload)");
  if ((st = ranges_ingest(c, S, L, threshold, n_scans, factor)) != CSM_OK) return st;
  commit_staged(c, S, csm_ctx::StagedKind::kRanges, n_scans);
  return CSM_OK;
}

}  // namespace csmh

using namespace csmh;

extern "C" {

int csm_laser_range_threshold(const csm_laser* laser, double* threshold) {
  if (!laser || !threshold) return CSM_ERR_INVALID_ARG;
  double t;
  if (!csm::laser_threshold(*laser, &t)) return CSM_ERR_INVALID_ARG;
  *threshold = t;
  return CSM_OK;
}

int csm_ranges_to_points(const csm_laser* laser, int32_t n_scans, const float* ranges, double factor,
                         double* points_xy, int64_t capacity_points, int64_t* point_offsets) {
  if (!laser || !point_offsets || n_scans < 0 || (n_scans > 0 && !ranges)) return CSM_ERR_INVALID_ARG;
  if (points_xy && capacity_points < 0) return CSM_ERR_INVALID_ARG;
  double threshold;
  if (!csm::laser_threshold(*laser, &threshold)) return CSM_ERR_INVALID_ARG;
  std::vector<double> cs;
  if (points_xy) {
    cs.resize((size_t)laser->n_beams * 2);
    csm::laser_trig_table(*laser, cs.data());
  }
  return csm::ranges_to_points(*laser, threshold, cs.data(), n_scans, ranges, factor, points_xy, capacity_points,
                               point_offsets)
             ? CSM_OK
             : CSM_ERR_INVALID_ARG;
}

int csm_load_ranges_async(csm_ctx* c, const csm_laser* laser, int32_t n_scans, const float* ranges, double factor) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return queue_ranges(c, laser, n_scans, ranges, factor);
}

int csm_load_ranges(csm_ctx* c, const csm_laser* laser, int32_t n_scans, const float* ranges, double factor) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int st;
  if ((st = unload_batch(c)) != CSM_OK) return st;
  // through a staging slot (none is queued now), taken at once
  if ((st = queue_ranges(c, laser, n_scans, ranges, factor)) != CSM_OK) return st;
  return take_staged(c);
}

}  // extern "C"
