// csm_batch.cpp — the resident batch of scans (ScanBatch, csm_host.hpp):
// loaded synchronously (csm_load_scans*), queued on the stage stream
// (csm_load_scans_async; csm_ranges.cpp and csm_deskew.cpp queue theirs
// through the same slots), taken by the next match, and read back
// (csm_loaded_scans); pinned host memory for the callers' arrays.
#include "csm_host.hpp"

namespace csmh {
namespace {

// Batches queued with csm_load_scans_async are dropped (their uploads are
// waited for): a synchronous load names the batch the next match runs, so
// csm_scan_matchers / csm_scan_matchers_batch never match a queued batch
// into output arrays sized for their own scans.
int drop_staged(csm_ctx* c) {
  if (c->staged_count <= 0) return CSM_OK;
  hipError_t e;
  if (c->stage_stream && (e = hipStreamSynchronize(c->stage_stream)) != hipSuccess)
    return c->hip_fail(e, "hipStreamSynchronize(stage)");
  c->staged_count = 0;
  return CSM_OK;
}

}  // namespace

int unload_batch(csm_ctx* c) {
  if (const int dst = pipe_drain(c)) return dst;  // a submitted batch still reads the context
  c->unload();
  return drop_staged(c);
}

// csm_load_scans once locked.
int load_scans_locked(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets) {
  int st;
  if ((st = unload_batch(c)) != CSM_OK) return st;
  if ((st = check_offsets(c, n_scans, offsets)) != CSM_OK) return st;
  const int64_t n_total = n_scans > 0 ? offsets[n_scans] - offsets[0] : 0;
  if ((st = check_points(c, pts, n_total)) != CSM_OK) return st;
  c->scan_off.assign(offsets, offsets + n_scans + 1);
  for (auto& o : c->scan_off) o -= offsets[0];
  if ((st = upload_points(c, n_total > 0 ? pts + 2 * offsets[0] : pts, n_total)) != CSM_OK) return st;
  hipError_t e;
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return c->hip_fail(e, "hipStreamSynchronize(points)");
  c->n_scans = n_scans;
  return CSM_OK;
}

// The staging slot the next queued batch goes into (csm_load_scans_async,
// csm_load_ranges*): a third queued batch is refused; the stage stream, the
// slot's event and its pinned word are made by the first call that needs them.
int open_stage_slot(csm_ctx* c, csm_ctx::Staged** out) {
  if (c->staged_count == 2) return c->fail(CSM_ERR_INVALID_ARG, "two batches already queued (csm_load_scans_async)");
  hipError_t e;
  if ((e = c->stage_stream.create(hipStreamNonBlocking)) != hipSuccess) return c->hip_fail(e, "hipStreamCreate(stage)");
  csm_ctx::Staged& S = c->staged[(c->staged_head + c->staged_count) % 2];
  if ((e = S.ready.create(hipEventDisableTiming)) != hipSuccess) return c->hip_fail(e, "hipEventCreate(stage)");
  if ((e = S.maxabs_h.ensure_exact(sizeof(unsigned long long))) != hipSuccess)
    return c->hip_fail(e, "hipHostMalloc(stage)");
  *out = &S;
  return CSM_OK;
}

hipError_t stage_maxabs_ready(csm_ctx* c, csm_ctx::Staged& S, int64_t n_points) {
  hipError_t e;
  hipStream_t s = c->stage_stream;
  unsigned long long* m = (unsigned long long*)S.maxabs_dev.p;
  if ((e = hipMemsetAsync(m, 0, sizeof(*m), s)) != hipSuccess ||
      (e = csm::launch_points_maxabs((const double*)S.batch.pts.p, n_points, m, s)) != hipSuccess ||
      (e = hipMemcpyAsync(S.maxabs_h.p, m, sizeof(*m), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return e;
  return hipEventRecord(S.ready, s);
}

void commit_staged(csm_ctx* c, csm_ctx::Staged& S, csm_ctx::StagedKind kind, int32_t n_scans) {
  S.kind = kind;
  S.batch.n_scans = n_scans;
  c->staged_count++;
}

// The oldest queued batch becomes the loaded one; the outgoing one parks in
// its slot (a pending submitted batch's last launch borrows it back,
// csm_scan_matchers_submit).
int take_staged(csm_ctx* c) {
  if (c->staged_count <= 0) return CSM_OK;
  csm_ctx::Staged& S = c->staged[c->staged_head];
  hipError_t e;
  if ((e = hipEventSynchronize(S.ready)) != hipSuccess) return c->hip_fail(e, "hipEventSynchronize(stage)");
  if (S.kind == csm_ctx::StagedKind::kDeskewed)
    if (const int rst = repair_deskewed(c, S)) return rst;
  if (S.kind != csm_ctx::StagedKind::kPoints) {  // the device's prefix counts, copied down before `ready`
    const int64_t* oh = (const int64_t*)S.off_h.p;
    S.batch.scan_off.assign(oh, oh + S.batch.n_scans + 1);
  }
  S.batch.scan_grid.clear();
  std::memcpy(&S.batch.pts_maxabs, S.maxabs_h.p, sizeof(double));
  c->swap_batch(S.batch);
  c->staged_head = (c->staged_head + 1) % 2;
  c->staged_count--;
  return CSM_OK;
}

}  // namespace csmh

using namespace csmh;

extern "C" {

int csm_load_scans(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  return load_scans_locked(c, n_scans, pts, offsets);
}

int csm_load_scans_grids(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets,
                         const int32_t* grid_index) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  const int st = load_scans_locked(c, n_scans, pts, offsets);
  if (st != CSM_OK || !grid_index) return st;
  c->scan_grid.assign(grid_index, grid_index + n_scans);
  return CSM_OK;
}

int csm_load_scans_async(csm_ctx* c, int32_t n_scans, const double* pts, const int64_t* offsets) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  int st;
  if ((st = check_offsets(c, n_scans, offsets)) != CSM_OK) return st;
  const int64_t n_total = n_scans > 0 ? offsets[n_scans] - offsets[0] : 0;
  if ((st = check_points(c, pts, n_total)) != CSM_OK) return st;
  csm_ctx::Staged* slot = nullptr;
  if ((st = open_stage_slot(c, &slot)) != CSM_OK) return st;
  csm_ctx::Staged& S = *slot;
  hipError_t e;
  const size_t bytes = (size_t)std::max<int64_t>(n_total, 1) * 2 * sizeof(double);
  if ((e = S.batch.pts.ensure(bytes)) != hipSuccess ||
      (e = S.maxabs_dev.ensure(sizeof(unsigned long long))) != hipSuccess)
    return c->hip_fail(e, "hipMalloc(stage)");
  // the buffer's previous batch was matched by a call that has returned, so
  // no kernel reads it any more
  if ((n_total > 0 && (e = hipMemcpyAsync(S.batch.pts.p, pts + 2 * offsets[0], (size_t)n_total * 2 * sizeof(double),
                                          hipMemcpyHostToDevice, c->stage_stream)) != hipSuccess) ||
      (e = stage_maxabs_ready(c, S, n_total)) != hipSuccess)
    return c->hip_fail(e, "csm_load_scans_async");
  S.batch.scan_off.assign(offsets, offsets + n_scans + 1);
  for (auto& o : S.batch.scan_off) o -= offsets[0];
  commit_staged(c, S, csm_ctx::StagedKind::kPoints, n_scans);
  return CSM_OK;
}

int csm_loaded_scans(csm_ctx* c, int32_t* n_scans, int64_t* point_offsets, int64_t offsets_capacity,
                     double* points_xy, int64_t capacity_points) {
  if (!c || !n_scans) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;
  if (c->n_scans < 0) return c->fail(CSM_ERR_INVALID_ARG, "no scans loaded (csm_load_scans)");
  const int32_t n = c->n_scans;
  *n_scans = n;
  const int64_t total = n > 0 ? c->scan_off[(size_t)n] : 0;
  if (point_offsets) {
    if (offsets_capacity < (int64_t)n + 1) return c->fail(CSM_ERR_INVALID_ARG, "offsets capacity below n_scans + 1");
    if (n > 0)
      std::memcpy(point_offsets, c->scan_off.data(), ((size_t)n + 1) * sizeof(int64_t));
    else
      point_offsets[0] = 0;
  }
  if (points_xy) {
    if (capacity_points < total) return c->fail(CSM_ERR_INVALID_ARG, "points capacity below the loaded point count");
    hipError_t e;
    if (total > 0 && ((e = hipMemcpyAsync(points_xy, c->pts.p, (size_t)total * 2 * sizeof(double),
                                          hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
                      (e = hipStreamSynchronize(c->stream)) != hipSuccess))
      return c->hip_fail(e, "hipMemcpy(loaded points)");
  }
  return CSM_OK;
}

int csm_host_alloc(size_t bytes, void** out) {
  if (!out) return CSM_ERR_INVALID_ARG;
  *out = nullptr;
  return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable) == hipSuccess ? CSM_OK : CSM_ERR_ALLOC;
}

int csm_host_free(void* p) { return (!p || hipHostFree(p) == hipSuccess) ? CSM_OK : CSM_ERR_INVALID_ARG; }

}  // extern "C"
