// csm_chain_maps.cpp — the resident scan store and the stack builder
// (include/csm_chain_maps.h): kept scans on the device as raw metres, their
// poses on the host, and csm_set_grid_stack_chains, which draws every submap of
// a query into the matcher's grid stack with one fill and one splat (a mark and
// a raise kernel) on the context's stream. What is computed on the host is csm_chain_maps.hpp's
// plan; the kernels are csm_chain_maps.hip's.
#include "csm_chain_maps.h"

#include "csm_chain_maps.hpp"
#include "csm_chain_maps_launch.hpp"
#include "csm_host.hpp"

using namespace csmh;

struct csm_scan_store {
  int device = 0;
  Stream stream;  // the points' uploads (declared before the buffers and events: destroyed after them)
  // After the last build that reads the store, on that build's stream. Each
  // build's stream first waits for the build before it, so the latest record
  // stands for every build handed out.
  Event built;
  bool built_used = false;
  Event plan_up;  // the last copy out of h_plan
  bool plan_up_used = false;
  mutable std::mutex mu;
  std::string err;
  std::vector<csm::ChainScan> scans;
  int64_t n_points = 0;
  DevBuf pts;      // every scan's points back to back: x, y in metres
  HostBuf h_plan;  // a build's placements, then its kernel table
  DevBuf d_plan;
  DevBuf hits;     // a build's hit mask: a byte a cell of the stack (csm_chain_maps.hip)

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  int hip_fail(hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return CSM_ERR_HIP;
  }
};

std::unique_lock<std::mutex> csm::scan_store_lock(csm_scan_store* s, csm::ScanStoreView* v) {
  std::unique_lock<std::mutex> lk(s->mu);
  v->device = s->device;
  v->pts = (const double*)s->pts.p;
  v->scans = s->scans.data();
  v->n_scans = (int32_t)s->scans.size();
  return lk;
}

extern "C" {

int csm_scan_store_create(int device, csm_scan_store** out) {
  if (!out) return CSM_ERR_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CSM_ERR_HIP;
  DeviceGuard g(device);
  auto* s = new csm_scan_store();
  s->device = device;
  if (s->stream.create(hipStreamNonBlocking) != hipSuccess || s->built.create(hipEventDisableTiming) != hipSuccess ||
      s->plan_up.create(hipEventDisableTiming) != hipSuccess) {
    delete s;
    return CSM_ERR_HIP;
  }
  *out = s;
  return CSM_OK;
}

int csm_scan_store_destroy(csm_scan_store* s) {
  if (!s) return CSM_OK;
  DeviceGuard g(s->device);  // across the delete: the members free themselves on the store's device
  if (s->built_used) (void)hipEventSynchronize(s->built);
  if (s->plan_up_used) (void)hipEventSynchronize(s->plan_up);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  delete s;
  return CSM_OK;
}

const char* csm_scan_store_last_error(const csm_scan_store* s) { return s ? s->err.c_str() : "null store"; }

int csm_scan_store_add(csm_scan_store* s, const double* points_m, int32_t n_points, const double sensor_pose[3],
                       int32_t* id) {
  if (!s || !sensor_pose || !id || n_points < 0 || (n_points > 0 && !points_m)) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->scans.size() >= (size_t)INT32_MAX) return s->fail(CSM_ERR_ALLOC, "scan store: 2^31 scans");
  DeviceGuard g(s->device);
  hipError_t e;
  const size_t have = (size_t)s->n_points * 16, need = have + (size_t)n_points * 16;
  if (need > s->pts.cap) {
    // a larger buffer with the points so far: builds in flight read the old one
    if (s->built_used && (e = hipEventSynchronize(s->built)) != hipSuccess) return s->hip_fail(e, "hipEventSynchronize(built)");
    DevBuf grown;
    if ((e = grown.ensure_exact(csm::grow_bytes(need, s->pts.cap))) != hipSuccess) return s->hip_fail(e, "hipMalloc(scan store)");
    if (have && ((e = hipMemcpyAsync(grown.p, s->pts.p, have, hipMemcpyDeviceToDevice, s->stream)) != hipSuccess ||
                 (e = hipStreamSynchronize(s->stream)) != hipSuccess))
      return s->hip_fail(e, "hipMemcpyAsync(scan store)");
    std::swap(s->pts, grown);
  }
  // the caller's buffer is free on return, and every later build finds the points there
  if (n_points > 0 &&
      ((e = hipMemcpyAsync((char*)s->pts.p + have, points_m, (size_t)n_points * 16, hipMemcpyHostToDevice, s->stream)) !=
           hipSuccess ||
       (e = hipStreamSynchronize(s->stream)) != hipSuccess))
    return s->hip_fail(e, "hipMemcpyAsync(scan points)");
  csm::ChainScan sc;
  sc.pt_begin = s->n_points;
  sc.n_points = n_points;
  std::memcpy(sc.pose, sensor_pose, sizeof(sc.pose));
  s->scans.push_back(sc);
  s->n_points += n_points;
  *id = (int32_t)s->scans.size() - 1;
  return CSM_OK;
}

int csm_scan_store_set_pose(csm_scan_store* s, int32_t id, const double sensor_pose[3]) {
  if (!s || !sensor_pose) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(s->mu);
  if (id < 0 || (size_t)id >= s->scans.size()) return s->fail(CSM_ERR_INVALID_ARG, "scan store: no kept scan of that id");
  std::memcpy(s->scans[(size_t)id].pose, sensor_pose, 3 * sizeof(double));
  return CSM_OK;
}

int csm_scan_store_count(const csm_scan_store* s, int32_t* n_scans, int64_t* n_points) {
  if (!s) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(s->mu);
  if (n_scans) *n_scans = (int32_t)s->scans.size();
  if (n_points) *n_points = s->n_points;
  return CSM_OK;
}

int csm_set_grid_stack_chains(csm_ctx* c, csm_scan_store* store, const csm_chain_map_param* mp, int32_t n_grids,
                              const int32_t* chain_offsets, const int32_t* chain_ids, const double map_offset[2],
                              csm_map_info* info_out) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!store || !mp || !chain_offsets || !map_offset) return c->fail(CSM_ERR_INVALID_ARG, "chain maps: null argument");
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;  // a submitted batch still reads the context
  std::lock_guard<std::mutex> slk(store->mu);
  if (store->device != c->device) return c->fail(CSM_ERR_INVALID_ARG, "scan store lives on another device");
  // everything that can reject the call comes before the current grid is touched
  const double t_plan = now_ms();
  csm::ChainPlan plan;
  std::string why;
  int st = csm::plan_chains(mp, n_grids, chain_offsets, chain_ids, map_offset, store->scans.data(),
                            (int32_t)store->scans.size(), &plan, &why);
  if (st != CSM_OK) return c->fail(st, why);
  csm_map_info info{};
  info.resolution = mp->resolution;
  info.offset_x = map_offset[0];
  info.offset_y = map_offset[1];
  info.size_x = mp->size_x;
  info.size_y = mp->size_y;
  info.update_index = plan.update_index;
  if ((st = check_grid_size(c, &info)) != CSM_OK) return st;
  const double plan_ms = now_ms() - t_plan;

  release_map_reader(c);
  park_current(c);
  const int64_t ncell = (int64_t)info.size_x * info.size_y, total = ncell * n_grids;
  const size_t place_bytes = plan.place.size() * sizeof(csm::ChainPlacement), ktab_bytes = plan.ktab.size() * sizeof(float);
  hipError_t e;
  // the plan goes up through the store's staging: the copy before it has left
  // it, and the build before this one no longer reads its device copy
  if (store->plan_up_used && (e = hipEventSynchronize(store->plan_up)) != hipSuccess)
    return c->hip_fail(e, "hipEventSynchronize(plan)");
  if ((e = store->h_plan.ensure(place_bytes + ktab_bytes)) != hipSuccess) return c->hip_fail(e, "hipHostMalloc(chain plan)");
  if (place_bytes + ktab_bytes > store->d_plan.cap && store->built_used &&
      (e = hipEventSynchronize(store->built)) != hipSuccess)
    return c->hip_fail(e, "hipEventSynchronize(built)");
  if ((e = store->d_plan.ensure(place_bytes + ktab_bytes)) != hipSuccess) return c->hip_fail(e, "hipMalloc(chain plan)");
  if (csm::chain_hits_bytes(total) > store->hits.cap && store->built_used &&
      (e = hipEventSynchronize(store->built)) != hipSuccess)
    return c->hip_fail(e, "hipEventSynchronize(built)");
  if ((e = store->hits.ensure(csm::chain_hits_bytes(total))) != hipSuccess) return c->hip_fail(e, "hipMalloc(chain hit mask)");
  if (place_bytes) std::memcpy(store->h_plan.p, plan.place.data(), place_bytes);
  std::memcpy((char*)store->h_plan.p + place_bytes, plan.ktab.data(), ktab_bytes);
  if (store->built_used && (e = hipStreamWaitEvent(c->stream, store->built, 0)) != hipSuccess)
    return c->hip_fail(e, "hipStreamWaitEvent(built)");
  if ((e = hipMemcpyAsync(store->d_plan.p, store->h_plan.p, place_bytes + ktab_bytes, hipMemcpyHostToDevice, c->stream)) !=
          hipSuccess ||
      (e = hipEventRecord(store->plan_up, c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(chain plan)");
  store->plan_up_used = true;

  if ((e = c->grid_buf.ensure((size_t)total * sizeof(float))) != hipSuccess) {
    c->has_grid = false;  // the stack that was there went with its buffer
    return c->hip_fail(e, "hipMalloc(grid stack)");
  }
  float* grids = (float*)c->grid_buf.p;
  // from the first write on, a call that fails leaves no grid: a stack drawn in part is none
  const auto drop = [c](int status) {
    c->has_grid = false;
    return status;
  };
  float fill_ms = 0.f, splat_ms = 0.f;
  if ((st = c->span_begin("chain_maps:fill")) != CSM_OK) return drop(st);
  if ((e = csm::launch_chain_fill(grids, (uint8_t*)store->hits.p, total, mp->default_cell_prob, c->stream)) != hipSuccess)
    return drop(c->hip_fail(e, "chain fill"));
  if ((st = c->span_end(&fill_ms, "chain_maps:fill")) != CSM_OK) return drop(st);
  if ((st = c->span_begin("chain_maps:splat")) != CSM_OK) return drop(st);
  e = csm::launch_chain_splat((const csm::ChainPlacement*)store->d_plan.p, (int32_t)plan.place.size(), plan.max_points,
                              (const double*)store->pts.p, 1 / mp->resolution, grids, (uint8_t*)store->hits.p, total,
                              info.size_x, info.size_y, plan.half_kernel,
                              (const float*)((const char*)store->d_plan.p + place_bytes), c->stream);
  // the store's buffers are read until here, even by a launch that failed part-way
  const hipError_t er = hipEventRecord(store->built, c->stream);
  if (er == hipSuccess) store->built_used = true;
  if (e != hipSuccess || er != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return drop(c->hip_fail(e != hipSuccess ? e : er, "chain splat"));
  }
  if ((st = c->span_end(&splat_ms, "chain_maps:splat")) != CSM_OK) return drop(st);
  if (c->profiling) {
    const int ks = 2 * plan.half_kernel + 1;
    double raises = 0.0;  // the splat's work as the reference does it: placements x points x (2 hk + 1)^2 raises
    for (const auto& p : plan.place) raises += (double)p.n_points * ks * ks;
    c->account("chain_maps:plan", (float)plan_ms, (double)(place_bytes + ktab_bytes), (double)plan.place.size());
    c->account("chain_maps:fill", fill_ms, (double)total * sizeof(float), 0.0);  // (+ a byte a cell of mask)
    c->account("chain_maps:splat", splat_ms, raises * sizeof(float), raises);
  }
  adopt_grid(c, grids, n_grids, info);
  c->grid_gen = ++c->gen_clock;
  if (info_out) *info_out = info;
  return CSM_OK;
}

int csm_grid_download(csm_ctx* c, int32_t grid_index, float* out, int64_t n_out) {
  if (!c) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(c->device);
  if (const int dst = pipe_drain(c)) return dst;  // a submitted batch still reads the context
  if (!c->has_grid || !c->d_grid) return c->fail(CSM_ERR_NO_GRID, "no grid set");
  const int64_t ncell = (int64_t)c->info.size_x * c->info.size_y;
  if (!out || grid_index < 0 || grid_index >= c->n_grids || n_out != ncell)
    return c->fail(CSM_ERR_INVALID_ARG, "grid download: index outside the stack, or n_out is not size_y * size_x");
  hipError_t e;
  if ((e = hipMemcpyAsync(out, c->d_grid + (int64_t)grid_index * ncell, (size_t)ncell * sizeof(float),
                          hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return c->hip_fail(e, "hipMemcpyAsync(grid download)");
  return CSM_OK;
}

}  // extern "C"
