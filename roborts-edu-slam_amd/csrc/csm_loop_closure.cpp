// csm_loop_closure.cpp — the sharded loop-closure search behind a C-ABI
// (include/csm_loop_closure.h; reference TryCloseLoop,
// pose_graph/range_scan_pose_graph.cpp:299-355). One process drives every
// device: a matcher context per device holds its shard of the submaps, the
// shards are searched concurrently from host threads, and one RCCL
// communicator per device (ncclCommInitAll) agrees on the answer.
#include "csm_loop_closure.h"

#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <cfloat>
#include <cstddef>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <functional>
#include <memory>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "csm_exchange.hpp"
#include "csm_gridmap_internal.hpp"
#include "csm_driver_levels.hpp"
#include "csm_lc_interface.hpp"

namespace {

// RCCL, resolved from a privately loaded librccl (RTLD_LOCAL): the matcher
// library has no link-time dependency on it, and a host process that
// carries its own RCCL (PyTorch) keeps it.
struct Rccl {
  void* h = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool load(std::string& err) {
    if (h) return true;
    for (const char* n : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
      h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (h) break;
    }
    if (!h) {
      err = std::string("cannot load librccl.so.1: ") + dlerror();
      return false;
    }
    CommInitAll = (decltype(CommInitAll))dlsym(h, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
    AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
    GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
    GetErrorString = (decltype(GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!CommInitAll || !CommDestroy || !AllReduce || !GroupStart || !GroupEnd || !GetErrorString) {
      err = "librccl.so.1 lacks an NCCL entry point";
      dlclose(h);
      h = nullptr;
      return false;
    }
    return true;
  }
};

Rccl& rccl() {
  static Rccl r;
  return r;
}

// The caller's current device is restored on every return: a host process
// (PyTorch, a ROS node) calling in must not be left on another GPU.
struct DeviceRestore {
  int prev = -1;
  DeviceRestore() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceRestore() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
std::mutex& rccl_mu() {
  static std::mutex m;
  return m;
}

// submaps [lo, hi) of `rank` (contiguous, sizes differ by at most one;
// roborts_csm/loop_closure.py shard_range)
void shard_range(int32_t n, int rank, int world, int32_t* lo, int32_t* hi) {
  const int32_t q = n / world, r = n % world;
  *lo = rank * q + (rank < r ? rank : r);
  *hi = *lo + q + (rank < r ? 1 : 0);
}

// One persistent host thread per device but the first (the caller's thread
// searches device 0's shard): a query wakes them instead of creating and
// joining G - 1 threads (tens of us against a ~0.3 ms query at 8 devices).
class ShardWorkers {
 public:
  explicit ShardWorkers(int n) {
    for (int r = 1; r < n; ++r) th_.emplace_back([this, r] { loop(r); });
  }
  ~ShardWorkers() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // fn(r) for every r in [0, n): r = 0 on the calling thread
  void run(const std::function<void(int)>& fn) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      job_ = &fn;
      pending_ = (int)th_.size();
      ++epoch_;
    }
    cv_.notify_all();
    fn(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  void loop(int r) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(int)>* job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || epoch_ != seen; });
        if (stop_) return;
        seen = epoch_;
        job = job_;
      }
      (*job)(r);
      std::lock_guard<std::mutex> lk(mu_);
      if (--pending_ == 0) done_cv_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(int)>* job_ = nullptr;
  uint64_t epoch_ = 0;
  int pending_ = 0;
  bool stop_ = false;
};

}  // namespace

namespace csmh {
int create_context(int device, int local_rank, int local_world, csm_ctx** out);  // csm_api.cpp
}

struct csm_loop_closure {
  std::mutex mu;
  std::string err;
  std::vector<int> devices;
  std::vector<csm_ctx*> ctx;
  std::vector<csm_scan_store*> stores;  // the kept scans, replicated: one store per device (made by the first add_scan)
  std::vector<std::vector<double>> scan_pts;  // ... and their raw points (m) on the host: csm_loop_closure_scan_match's query
  std::vector<ncclComm_t> comms;
  std::vector<hipStream_t> streams;
  std::vector<csm::LcExchange*> xbuf;  // device, one per device
  csm::LcExchange* h_x = nullptr;      // pinned host staging, one per device
  int32_t n_submaps = 0;
  // A failure after the exchange's first collective was enqueued leaves the
  // communicators out of step: the handle refuses further matches.
  bool broken = false;
  double resolution = 0.0;
  std::vector<double> offsets;
  // the submaps' common size, and the one map offset their stacks' geometry carries (what the
  // level drivers convert poses with)
  int32_t size_x = 0, size_y = 0;
  double stack_offset[2] = {0.0, 0.0};
  std::vector<int32_t> lo, hi;
  std::unique_ptr<ShardWorkers> workers;

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  int hip_fail(hipError_t e, const char* what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return CSM_ERR_HIP;
  }
  int nccl_fail(ncclResult_t r, const char* what) {
    err = std::string(what) + ": " + rccl().GetErrorString(r);
    return CSM_ERR_HIP;
  }
};

extern "C" {

int csm_loop_closure_destroy(csm_loop_closure* lc) {
  if (!lc) return CSM_ERR_INVALID_ARG;
  DeviceRestore restore;
  for (size_t r = 0; r < lc->comms.size(); ++r)
    if (lc->comms[r]) (void)rccl().CommDestroy(lc->comms[r]);
  for (size_t r = 0; r < lc->devices.size(); ++r) {
    (void)hipSetDevice(lc->devices[r]);
    if (r < lc->xbuf.size() && lc->xbuf[r]) (void)hipFree(lc->xbuf[r]);
    if (r < lc->streams.size() && lc->streams[r]) (void)hipStreamDestroy(lc->streams[r]);
  }
  lc->workers.reset();
  if (lc->h_x) (void)hipHostFree(lc->h_x);
  for (csm_scan_store* st : lc->stores)  // before the contexts: a store waits for the builds that read it
    if (st) csm_scan_store_destroy(st);
  for (csm_ctx* c : lc->ctx)
    if (c) csm_destroy(c);
  delete lc;
  return CSM_OK;
}

int csm_loop_closure_create(int32_t n_devices, const int32_t* devices, csm_loop_closure** out) {
  if (!out || n_devices <= 0) return CSM_ERR_INVALID_ARG;
  *out = nullptr;
  DeviceRestore restore;
  csm_loop_closure* lc = new csm_loop_closure();
  for (int r = 0; r < n_devices; ++r) lc->devices.push_back(devices ? devices[r] : r);
  int st;
  {
    std::lock_guard<std::mutex> lk(rccl_mu());
    if (!rccl().load(lc->err)) {
      *out = lc;  // the caller reads csm_loop_closure_last_error, then destroys
      return CSM_ERR_UNSUPPORTED;
    }
  }
  for (int r = 0; r < n_devices; ++r) {
    csm_ctx* c = nullptr;
    // the G contexts share this process's CPUs: host plan of rank r of G
    if ((st = csmh::create_context(lc->devices[r], r, n_devices, &c)) != CSM_OK) {
      lc->err = "csm_create on device " + std::to_string(lc->devices[r]) + " failed";
      *out = lc;
      return st;
    }
    lc->ctx.push_back(c);
    hipError_t e;
    hipStream_t s = nullptr;
    void* x = nullptr;
    if ((e = hipSetDevice(lc->devices[r])) != hipSuccess || (e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc(&x, sizeof(csm::LcExchange))) != hipSuccess) {
      *out = lc;
      return lc->hip_fail(e, "exchange buffers");
    }
    lc->streams.push_back(s);
    lc->xbuf.push_back((csm::LcExchange*)x);
  }
  hipError_t e;
  if ((e = hipHostMalloc((void**)&lc->h_x, sizeof(csm::LcExchange) * n_devices, hipHostMallocDefault)) != hipSuccess) {
    *out = lc;
    return lc->hip_fail(e, "hipHostMalloc(exchange)");
  }
  lc->comms.assign((size_t)n_devices, nullptr);
  ncclResult_t nr = rccl().CommInitAll(lc->comms.data(), n_devices, lc->devices.data());
  if (nr != ncclSuccess) {
    lc->comms.assign((size_t)n_devices, nullptr);
    *out = lc;
    return lc->nccl_fail(nr, "ncclCommInitAll");
  }
  *out = lc;
  return CSM_OK;
}

const char* csm_loop_closure_last_error(const csm_loop_closure* lc) { return lc ? lc->err.c_str() : "null handle"; }

int csm_loop_closure_set_submaps(csm_loop_closure* lc, const float* cells, int32_t n_submaps, const csm_map_info* info,
                                 const double* offsets, int64_t version) {
  if (!lc || !cells || !info || !offsets || n_submaps <= 0) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  DeviceRestore restore;
  const int G = (int)lc->devices.size();
  const int64_t per = (int64_t)info->size_x * info->size_y;
  // the new shard ranges are committed only once every shard is resident: a
  // failed upload leaves no submaps (match then fails with CSM_ERR_NO_GRID)
  // instead of a mix of old and new stacks under the old ranges
  std::vector<int32_t> lo((size_t)G, 0), hi((size_t)G, 0);
  lc->n_submaps = 0;
  for (int r = 0; r < G; ++r) {
    shard_range(n_submaps, r, G, &lo[(size_t)r], &hi[(size_t)r]);
    const int32_t n = hi[(size_t)r] - lo[(size_t)r];
    if (n == 0) continue;
    int st = csm_set_grid_stack(lc->ctx[(size_t)r], cells + lo[(size_t)r] * per, n, info, version);
    if (st != CSM_OK) return lc->fail(st, std::string("device ") + std::to_string(lc->devices[(size_t)r]) + ": " +
                                              csm_last_error(lc->ctx[(size_t)r]));
  }
  lc->lo.swap(lo);
  lc->hi.swap(hi);
  lc->resolution = info->resolution;
  lc->offsets.assign(offsets, offsets + 2 * (size_t)n_submaps);
  lc->size_x = info->size_x;
  lc->size_y = info->size_y;
  lc->stack_offset[0] = info->offset_x;
  lc->stack_offset[1] = info->offset_y;
  lc->n_submaps = n_submaps;
  return CSM_OK;
}

// The per-device stores, made on first use.
static int lc_ensure_stores(csm_loop_closure* lc) {
  if (!lc->stores.empty()) return CSM_OK;
  std::vector<csm_scan_store*> made;
  for (size_t r = 0; r < lc->devices.size(); ++r) {
    csm_scan_store* st = nullptr;
    const int rc = csm_scan_store_create(lc->devices[r], &st);
    if (rc != CSM_OK) {
      for (csm_scan_store* m : made) csm_scan_store_destroy(m);
      return lc->fail(rc, "csm_scan_store_create on device " + std::to_string(lc->devices[r]) + " failed");
    }
    made.push_back(st);
  }
  lc->stores.swap(made);
  return CSM_OK;
}

int csm_loop_closure_add_scan(csm_loop_closure* lc, const double* points_m, int32_t n_points, const double sensor_pose[3],
                              int32_t* id) {
  if (!lc || !sensor_pose || !id || n_points < 0 || (n_points > 0 && !points_m)) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  DeviceRestore restore;
  int st;
  if ((st = lc_ensure_stores(lc)) != CSM_OK) return st;
  int32_t first = -1;
  for (size_t r = 0; r < lc->stores.size(); ++r) {
    int32_t got = -1;
    if ((st = csm_scan_store_add(lc->stores[r], points_m, n_points, sensor_pose, &got)) != CSM_OK)
      return lc->fail(st, "device " + std::to_string(lc->devices[r]) + ": " + csm_scan_store_last_error(lc->stores[r]));
    if (r == 0) first = got;
    if (got != first) {  // a store an earlier failure left behind the others
      lc->n_submaps = 0;
      return lc->fail(CSM_ERR_HIP, "the devices' scan stores are out of step");
    }
  }
  if (lc->scan_pts.size() <= (size_t)first) lc->scan_pts.resize((size_t)first + 1);
  lc->scan_pts[(size_t)first].assign(points_m, points_m + 2 * (size_t)n_points);
  *id = first;
  return CSM_OK;
}

int csm_loop_closure_set_scan_pose(csm_loop_closure* lc, int32_t id, const double sensor_pose[3]) {
  if (!lc || !sensor_pose) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  if (lc->stores.empty()) return lc->fail(CSM_ERR_INVALID_ARG, "no kept scan of that id");
  for (size_t r = 0; r < lc->stores.size(); ++r) {
    const int st = csm_scan_store_set_pose(lc->stores[r], id, sensor_pose);
    if (st != CSM_OK) return lc->fail(st, csm_scan_store_last_error(lc->stores[r]));
  }
  return CSM_OK;
}

int csm_loop_closure_set_submaps_chains(csm_loop_closure* lc, const csm_chain_map_param* mp, int32_t n_submaps,
                                        const int32_t* chain_offsets, const int32_t* chain_ids,
                                        const double current_pose[3]) {
  if (!lc || !mp || !chain_offsets || !current_pose) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  DeviceRestore restore;
  // as csm_loop_closure_set_submaps: a failed call leaves no submaps
  lc->n_submaps = 0;
  if (n_submaps <= 0) return lc->fail(CSM_ERR_INVALID_ARG, "chain maps: n_submaps < 1");
  if (chain_offsets[0] != 0) return lc->fail(CSM_ERR_INVALID_ARG, "chain maps: chain_offsets[0] must be 0");
  for (int32_t i = 0; i < n_submaps; ++i)
    if (chain_offsets[i + 1] < chain_offsets[i])
      return lc->fail(CSM_ERR_INVALID_ARG, "chain maps: chain_offsets decrease at submap " + std::to_string(i));
  if (chain_offsets[n_submaps] > 0 && !chain_ids) return lc->fail(CSM_ERR_INVALID_ARG, "chain maps: null chain_ids");
  int st;
  if ((st = lc_ensure_stores(lc)) != CSM_OK) return st;
  // ResetScanMatchMapWithRangeVec (slam_processor.cpp:452-454): the map centred on the current pose
  const double cell = 1 / (1.0 / mp->resolution);  // GetCellLength()
  const double map_offset[2] = {-(current_pose[0] - 0.5 * mp->size_x * cell), -(current_pose[1] - 0.5 * mp->size_y * cell)};
  const int G = (int)lc->devices.size();
  std::vector<int32_t> lo((size_t)G, 0), hi((size_t)G, 0);
  for (int r = 0; r < G; ++r) shard_range(n_submaps, r, G, &lo[(size_t)r], &hi[(size_t)r]);
  // device r draws its shard only, the devices concurrently
  std::vector<int> status((size_t)G, CSM_OK);
  std::vector<std::string> errs((size_t)G);
  auto run = [&](int r) {
    const int32_t n = hi[(size_t)r] - lo[(size_t)r];
    if (n == 0) return;
    const int32_t base = chain_offsets[lo[(size_t)r]];
    std::vector<int32_t> off((size_t)n + 1);
    for (int32_t i = 0; i <= n; ++i) off[(size_t)i] = chain_offsets[lo[(size_t)r] + i] - base;
    const int rc = csm_set_grid_stack_chains(lc->ctx[(size_t)r], lc->stores[(size_t)r], mp, n, off.data(),
                                             chain_ids ? chain_ids + base : nullptr, map_offset, nullptr);
    if (rc != CSM_OK) {
      status[(size_t)r] = rc;
      errs[(size_t)r] = csm_last_error(lc->ctx[(size_t)r]);
    }
  };
  if (!lc->workers) lc->workers.reset(new ShardWorkers(G));
  lc->workers->run(run);
  for (int r = 0; r < G; ++r)
    if (status[(size_t)r] != CSM_OK)
      return lc->fail(status[(size_t)r], "device " + std::to_string(lc->devices[(size_t)r]) + ": " + errs[(size_t)r]);
  lc->lo.swap(lo);
  lc->hi.swap(hi);
  lc->resolution = mp->resolution;
  lc->size_x = mp->size_x;
  lc->size_y = mp->size_y;
  lc->stack_offset[0] = map_offset[0];
  lc->stack_offset[1] = map_offset[1];
  lc->offsets.resize(2 * (size_t)n_submaps);
  for (int32_t i = 0; i < n_submaps; ++i) {
    lc->offsets[2 * (size_t)i] = map_offset[0];
    lc->offsets[2 * (size_t)i + 1] = map_offset[1];
  }
  lc->n_submaps = n_submaps;
  return CSM_OK;
}

// csm_loop_closure_match with lc->mu held.
static int lc_match_locked(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                           const double pose_world[3], int32_t search, csm_loop_closure_result* res) {
  DeviceRestore restore;
  if (lc->broken) return lc->fail(CSM_ERR_HIP, "an earlier exchange failed part-way: the communicators are out of step");
  if (lc->n_submaps == 0) return lc->fail(CSM_ERR_NO_GRID, "no submaps set");
  int32_t na = 0, ns = 0;
  if (csm_window_dims(param, &na, &ns) != CSM_OK) return lc->fail(CSM_ERR_INVALID_ARG, "invalid window parameters");
  const int64_t n_cand = (int64_t)na * ns * ns;
  const int G = (int)lc->devices.size();
  // GetMapCoordsPose of the query pose in every submap (grid_map_base.h:68-69,89-93:
  // Scaling(1 / resolution) * Translation(offset), in Eigen's order)
  const double s = 1.0 / lc->resolution;
  std::vector<double> centers(3 * (size_t)lc->n_submaps);
  for (int32_t i = 0; i < lc->n_submaps; ++i) {
    centers[3 * (size_t)i] = s * pose_world[0] + s * lc->offsets[2 * (size_t)i];
    centers[3 * (size_t)i + 1] = s * pose_world[1] + s * lc->offsets[2 * (size_t)i + 1];
    centers[3 * (size_t)i + 2] = pose_world[2];
  }
  using clock = std::chrono::steady_clock;
  const auto ms_since = [](clock::time_point t) {
    return std::chrono::duration<double, std::milli>(clock::now() - t).count();
  };
  const clock::time_point t_search = clock::now();
  // per device: its shard's best, searched concurrently
  std::vector<int> status((size_t)G, CSM_OK);
  std::vector<std::string> errs((size_t)G);
  auto run = [&](int r) {
    csm::LcExchange& x = lc->h_x[r];
    x = csm::LcExchange{};
    x.local_score = -DBL_MAX;
    x.local_idx = -1;
    const int32_t lo = lc->lo[(size_t)r], n = lc->hi[(size_t)r] - lo;
    if (n > 0) {
      std::vector<int32_t> gi((size_t)n);
      for (int32_t i = 0; i < n; ++i) gi[(size_t)i] = i;
      const double* c = centers.data() + 3 * (size_t)lo;
      csm_best b{};
      int32_t w = -1;
      int st;
      if (search == CSM_LC_PYRAMID) {
        st = csm_search_windows(lc->ctx[(size_t)r], pts, n_points, param, n, gi.data(), c, nullptr, &b, &w, nullptr);
      } else {
        std::vector<csm_best> all((size_t)n);
        st = csm_best_windows(lc->ctx[(size_t)r], pts, n_points, param, n, gi.data(), c, all.data());
        for (int32_t i = 0; st == CSM_OK && i < n; ++i) {
          const csm_best& q = all[(size_t)i];
          if (w < 0 || q.score > b.score || (q.score == b.score && (int64_t)i * n_cand + q.flat_index <
                                                                      (int64_t)w * n_cand + b.flat_index)) {
            b = q;
            w = i;
          }
        }
      }
      if (st != CSM_OK) {
        status[(size_t)r] = st;
        errs[(size_t)r] = csm_last_error(lc->ctx[(size_t)r]);
        return;
      }
      x.local_score = b.score;
      x.local_idx = (int64_t)(lo + w) * n_cand + b.flat_index;
      x.local_row[0] = (double)(lo + w);
      x.local_row[1] = b.x;
      x.local_row[2] = b.y;
      x.local_row[3] = b.angle;
    }
    x.score = x.local_score;
  };
  if (!lc->workers) lc->workers.reset(new ShardWorkers(G));
  lc->workers->run(run);
  for (int r = 0; r < G; ++r)
    if (status[(size_t)r] != CSM_OK)
      return lc->fail(status[(size_t)r], "device " + std::to_string(lc->devices[(size_t)r]) + ": " + errs[(size_t)r]);

  const double search_ms = ms_since(t_search);
  const clock::time_point t_exchange = clock::now();
  // the exchange: MAX score -> pick -> MIN index -> row -> SUM row, all enqueued
  hipError_t e;
  ncclResult_t nr;
  Rccl& R = rccl();
  for (int r = 0; r < G; ++r) {
    if ((e = hipSetDevice(lc->devices[(size_t)r])) != hipSuccess) return lc->hip_fail(e, "hipSetDevice");
    if ((e = hipMemcpyAsync(lc->xbuf[(size_t)r], &lc->h_x[r], offsetof(csm::LcExchange, score_max),
                            hipMemcpyHostToDevice, lc->streams[(size_t)r])) != hipSuccess)
      return lc->hip_fail(e, "hipMemcpyAsync(exchange)");
  }
  auto all_reduce = [&](size_t off_in, size_t off_out, size_t count, ncclDataType_t t, ncclRedOp_t op) -> int {
    if ((nr = R.GroupStart()) != ncclSuccess) return lc->nccl_fail(nr, "ncclGroupStart");
    for (int r = 0; r < G; ++r) {
      char* b = (char*)lc->xbuf[(size_t)r];
      if ((nr = R.AllReduce(b + off_in, b + off_out, count, t, op, lc->comms[(size_t)r], lc->streams[(size_t)r])) !=
          ncclSuccess) {
        (void)R.GroupEnd();
        return lc->nccl_fail(nr, "ncclAllReduce");
      }
    }
    if ((nr = R.GroupEnd()) != ncclSuccess) return lc->nccl_fail(nr, "ncclGroupEnd");
    return CSM_OK;
  };
  // From the first collective on, a failure on one device leaves collectives
  // in flight on the others: every stream is drained (best effort; the staging
  // h_x stays untouched until then) and the handle refuses later matches.
  auto abandon = [&](int st) {
    lc->broken = true;
    for (int r = 0; r < G; ++r)
      if (hipSetDevice(lc->devices[(size_t)r]) == hipSuccess) (void)hipStreamSynchronize(lc->streams[(size_t)r]);
    return st;
  };
  int st;
  if ((st = all_reduce(offsetof(csm::LcExchange, score), offsetof(csm::LcExchange, score_max), 1, ncclFloat64,
                       ncclMax)) != CSM_OK)
    return abandon(st);
  for (int r = 0; r < G; ++r) {
    if ((e = hipSetDevice(lc->devices[(size_t)r])) != hipSuccess ||
        (e = csm::launch_lc_pick(lc->xbuf[(size_t)r], lc->streams[(size_t)r])) != hipSuccess)
      return abandon(lc->hip_fail(e, "lc_pick_kernel"));
  }
  if ((st = all_reduce(offsetof(csm::LcExchange, idx), offsetof(csm::LcExchange, idx_min), 1, ncclInt64, ncclMin)) !=
      CSM_OK)
    return abandon(st);
  for (int r = 0; r < G; ++r) {
    if ((e = hipSetDevice(lc->devices[(size_t)r])) != hipSuccess ||
        (e = csm::launch_lc_row(lc->xbuf[(size_t)r], lc->streams[(size_t)r])) != hipSuccess)
      return abandon(lc->hip_fail(e, "lc_row_kernel"));
  }
  if ((st = all_reduce(offsetof(csm::LcExchange, row), offsetof(csm::LcExchange, row_sum), 4, ncclFloat64,
                       ncclSum)) != CSM_OK)
    return abandon(st);
  csm::LcExchange* out = &lc->h_x[0];
  if ((e = hipSetDevice(lc->devices[0])) != hipSuccess ||
      (e = hipMemcpyAsync(out, lc->xbuf[0], sizeof(csm::LcExchange), hipMemcpyDeviceToHost, lc->streams[0])) !=
          hipSuccess)
    return abandon(lc->hip_fail(e, "hipMemcpyAsync(exchange result)"));
  for (int r = 0; r < G; ++r) {
    if ((e = hipSetDevice(lc->devices[(size_t)r])) != hipSuccess ||
        (e = hipStreamSynchronize(lc->streams[(size_t)r])) != hipSuccess)
      return abandon(lc->hip_fail(e, "exchange"));
  }
  res->search_ms = search_ms;
  res->exchange_ms = ms_since(t_exchange);
  res->n_devices = G;
  res->score = out->score_max;
  const bool none = out->idx_min == INT64_MAX;
  res->global_index = none ? -1 : out->idx_min;
  res->submap = none ? -1 : (int32_t)out->row_sum[0];
  res->x = out->row_sum[1];
  res->y = out->row_sum[2];
  res->angle = out->row_sum[3];
  // GetWorldCoordsPose of the winner in its submap (grid_map_base.h:83-87; csm_api.cpp Geometry)
  if (!none) {
    const double tx = s * lc->offsets[2 * (size_t)res->submap], ty = s * lc->offsets[2 * (size_t)res->submap + 1];
    const double inv_a = s * (1.0 / (s * s - 0.0 * 0.0));
    const double ntx = -(inv_a * tx), nty = -(inv_a * ty);
    res->pose_world[0] = inv_a * res->x + ntx;
    res->pose_world[1] = inv_a * res->y + nty;
    res->pose_world[2] = res->angle;
  }
  return CSM_OK;
}

int csm_loop_closure_match(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                           const double pose_world[3], int32_t search, csm_loop_closure_result* res) {
  if (!lc || !pts || !param || !pose_world || !res) return CSM_ERR_INVALID_ARG;
  if (search != CSM_LC_PYRAMID && search != CSM_LC_EXHAUSTIVE) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  return lc_match_locked(lc, pts, n_points, param, pose_world, search, res);
}

// The device that holds submap `submap`.
static int lc_owner(const csm_loop_closure* lc, int32_t submap) {
  const int G = (int)lc->devices.size();
  int r = 0;
  while (r < G - 1 && !(submap >= lc->lo[(size_t)r] && submap < lc->hi[(size_t)r])) ++r;
  return r;
}

// The full ScanMatch result of res->submap's window, on the device that holds
// it (csm_search_match on that one window of its resident stack; its pooled
// levels are the ones the search just used): cov and match as
// csm_search_match writes them, match->window the submap, res->pose_world the
// averaged pose's world coordinates. *err: the failure's message (the caller
// may run several of these at once, one per device).
static int lc_finish_submap(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                            const double pose_world[3], double cov[9], csm_loop_closure_result* res,
                            csm_match_result* match, std::string* err) {
  const int r = lc_owner(lc, res->submap);
  const int32_t local = res->submap - lc->lo[(size_t)r];
  const double s = 1.0 / lc->resolution;
  const double tx = s * lc->offsets[2 * (size_t)res->submap], ty = s * lc->offsets[2 * (size_t)res->submap + 1];
  const double center[3] = {s * pose_world[0] + tx, s * pose_world[1] + ty, pose_world[2]};  // GetMapCoordsPose, as the match
  DeviceRestore restore;
  csm_match_options mo{};
  mo.search.max_depth = -1;  // as null options: the search's own choice
  mo.collect_capacity = CSM_COLLECT_AUTO;
  const int st = csm_search_match(lc->ctx[(size_t)r], pts, n_points, param, 1, &local, center, &mo, cov, match);
  if (st != CSM_OK) {
    *err = "device " + std::to_string(lc->devices[(size_t)r]) + ": " + csm_last_error(lc->ctx[(size_t)r]);
    return st;
  }
  match->window = res->submap;  // the winner among all submaps
  // GetWorldCoordsPose of the averaged pose in its submap (grid_map_base.h:83-87)
  const double inv_a = s * (1.0 / (s * s - 0.0 * 0.0));
  const double ntx = -(inv_a * tx), nty = -(inv_a * ty);
  res->pose_world[0] = inv_a * match->pose_map[0] + ntx;
  res->pose_world[1] = inv_a * match->pose_map[1] + nty;
  res->pose_world[2] = match->pose_map[2];
  return CSM_OK;
}

int csm_loop_closure_match_full(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                                const double pose_world[3], int32_t search, double cov[9],
                                csm_loop_closure_result* res, csm_match_result* match) {
  if (!lc || !pts || !param || !pose_world || !cov || !res || !match) return CSM_ERR_INVALID_ARG;
  if (search != CSM_LC_PYRAMID && search != CSM_LC_EXHAUSTIVE) return CSM_ERR_INVALID_ARG;
  if (param->type == CSM_FAST) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  int st = lc_match_locked(lc, pts, n_points, param, pose_world, search, res);
  if (st != CSM_OK) return st;
  if (res->submap < 0) return lc->fail(CSM_ERR_INVALID_ARG, "no submap was scored");
  std::string err;
  if ((st = lc_finish_submap(lc, pts, n_points, param, pose_world, cov, res, match, &err)) != CSM_OK)
    return lc->fail(st, err);
  return CSM_OK;
}

// csm_loop_closure_match_gated with lc->mu held. Every device runs
// csm_search_gated on its shard concurrently; the answer is per submap and the
// shards are disjoint contiguous ranges in submap order, so the host
// concatenates them: no collective.
static int lc_match_gated_locked(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                                 const double pose_world[3], double min_response, csm_loop_closure_result* results,
                                 int32_t capacity, int32_t* n_pass) {
  DeviceRestore restore;
  if (lc->n_submaps == 0) return lc->fail(CSM_ERR_NO_GRID, "no submaps set");
  int32_t na = 0, ns = 0;
  if (csm_window_dims(param, &na, &ns) != CSM_OK) return lc->fail(CSM_ERR_INVALID_ARG, "invalid window parameters");
  const int64_t n_cand = (int64_t)na * ns * ns;
  const int G = (int)lc->devices.size();
  // GetMapCoordsPose of the query pose in every submap, as lc_match_locked
  const double s = 1.0 / lc->resolution;
  std::vector<double> centers(3 * (size_t)lc->n_submaps);
  for (int32_t i = 0; i < lc->n_submaps; ++i) {
    centers[3 * (size_t)i] = s * pose_world[0] + s * lc->offsets[2 * (size_t)i];
    centers[3 * (size_t)i + 1] = s * pose_world[1] + s * lc->offsets[2 * (size_t)i + 1];
    centers[3 * (size_t)i + 2] = pose_world[2];
  }
  using clock = std::chrono::steady_clock;
  const clock::time_point t_search = clock::now();
  std::vector<int> status((size_t)G, CSM_OK);
  std::vector<std::string> errs((size_t)G);
  std::vector<std::vector<int32_t>> wins((size_t)G);
  std::vector<std::vector<csm_best>> bests((size_t)G);
  std::vector<int32_t> counts((size_t)G, 0);
  auto run = [&](int r) {
    const int32_t lo = lc->lo[(size_t)r], n = lc->hi[(size_t)r] - lo;
    if (n <= 0) return;
    std::vector<int32_t> gi((size_t)n);
    for (int32_t i = 0; i < n; ++i) gi[(size_t)i] = i;
    wins[(size_t)r].resize((size_t)n);
    bests[(size_t)r].resize((size_t)n);
    const int st = csm_search_gated(lc->ctx[(size_t)r], pts, n_points, param, n, gi.data(),
                                    centers.data() + 3 * (size_t)lo, min_response, nullptr, wins[(size_t)r].data(),
                                    bests[(size_t)r].data(), n, &counts[(size_t)r], nullptr);
    if (st != CSM_OK) {
      status[(size_t)r] = st;
      errs[(size_t)r] = csm_last_error(lc->ctx[(size_t)r]);
    }
  };
  if (!lc->workers) lc->workers.reset(new ShardWorkers(G));
  lc->workers->run(run);
  for (int r = 0; r < G; ++r)
    if (status[(size_t)r] != CSM_OK)
      return lc->fail(status[(size_t)r], "device " + std::to_string(lc->devices[(size_t)r]) + ": " + errs[(size_t)r]);
  const double search_ms = std::chrono::duration<double, std::milli>(clock::now() - t_search).count();
  int32_t n = 0;
  for (int r = 0; r < G; ++r) {
    for (int32_t k = 0; k < counts[(size_t)r]; ++k, ++n) {
      if (n >= capacity) continue;
      const csm_best& b = bests[(size_t)r][(size_t)k];
      csm_loop_closure_result& res = results[n];
      res = csm_loop_closure_result{};
      res.submap = lc->lo[(size_t)r] + wins[(size_t)r][(size_t)k];
      res.score = b.score;
      res.global_index = (int64_t)res.submap * n_cand + b.flat_index;
      res.n_devices = G;
      res.x = b.x;
      res.y = b.y;
      res.angle = b.angle;
      res.search_ms = search_ms;
      res.exchange_ms = 0.0;
      // GetWorldCoordsPose of the candidate in its submap (grid_map_base.h:83-87), as lc_match_locked
      const double tx = s * lc->offsets[2 * (size_t)res.submap], ty = s * lc->offsets[2 * (size_t)res.submap + 1];
      const double inv_a = s * (1.0 / (s * s - 0.0 * 0.0));
      const double ntx = -(inv_a * tx), nty = -(inv_a * ty);
      res.pose_world[0] = inv_a * res.x + ntx;
      res.pose_world[1] = inv_a * res.y + nty;
      res.pose_world[2] = res.angle;
    }
  }
  *n_pass = n;
  return CSM_OK;
}

int csm_loop_closure_match_gated(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                                 const double pose_world[3], double min_response, csm_loop_closure_result* results,
                                 int32_t capacity, int32_t* n_pass) {
  if (!lc || !pts || !param || !pose_world || !n_pass || capacity < 0 || (capacity > 0 && !results) ||
      !(min_response == min_response))
    return CSM_ERR_INVALID_ARG;
  if (param->type == CSM_FAST) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  return lc_match_gated_locked(lc, pts, n_points, param, pose_world, min_response, results, capacity, n_pass);
}

// csm_loop_closure_match_gated_full with lc->mu held.
static int lc_match_gated_full_locked(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                                      const double pose_world[3], double min_response,
                                      csm_loop_closure_result* results, int32_t capacity, int32_t* n_pass, double* covs,
                                      csm_match_result* matches) {
  int st = lc_match_gated_locked(lc, pts, n_points, param, pose_world, min_response, results, capacity, n_pass);
  if (st != CSM_OK) return st;
  // each passing submap's device finishes that window: the devices in
  // parallel, a device's own submaps in order
  const int G = (int)lc->devices.size();
  const int32_t m = *n_pass < capacity ? *n_pass : capacity;
  std::vector<int> status((size_t)G, CSM_OK);
  std::vector<std::string> errs((size_t)G);
  auto run = [&](int r) {
    for (int32_t k = 0; k < m && status[(size_t)r] == CSM_OK; ++k) {
      if (lc_owner(lc, results[k].submap) != r) continue;
      status[(size_t)r] = lc_finish_submap(lc, pts, n_points, param, pose_world, covs + 9 * (size_t)k, &results[k],
                                           &matches[k], &errs[(size_t)r]);
    }
  };
  DeviceRestore restore;
  if (!lc->workers) lc->workers.reset(new ShardWorkers(G));
  lc->workers->run(run);
  for (int r = 0; r < G; ++r)
    if (status[(size_t)r] != CSM_OK) return lc->fail(status[(size_t)r], errs[(size_t)r]);
  return CSM_OK;
}

int csm_loop_closure_match_gated_full(csm_loop_closure* lc, const double* pts, int32_t n_points, const csm_param* param,
                                      const double pose_world[3], double min_response,
                                      csm_loop_closure_result* results, int32_t capacity, int32_t* n_pass, double* covs,
                                      csm_match_result* matches) {
  if (!lc || !pts || !param || !pose_world || !n_pass || capacity < 0 ||
      (capacity > 0 && (!results || !covs || !matches)) || !(min_response == min_response))
    return CSM_ERR_INVALID_ARG;
  if (param->type == CSM_FAST) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  return lc_match_gated_full_locked(lc, pts, n_points, param, pose_world, min_response, results, capacity, n_pass, covs,
                                    matches);
}

int csm_loop_closure_map_check(csm_loop_closure* lc, csm_gridmap* pub_map, int32_t scan_id,
                               const csm_map_check_param* param, const csm_loop_closure_result* results, int32_t n,
                               double* penalties) {
  if (!lc || !pub_map || !param || n < 0 || (n > 0 && (!results || !penalties))) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  csm::GridMapView view;
  int st = csm::gridmap_view(pub_map, &view);
  if (st != CSM_OK) return lc->fail(st, "map check: the pub map gave no view");
  size_t r = 0;
  while (r < lc->devices.size() && lc->devices[r] != view.device) ++r;
  if (r == lc->devices.size())
    return lc->fail(CSM_ERR_INVALID_ARG, "map check: the pub map lives on device " + std::to_string(view.device) +
                                             ", which is none of the loop closure's");
  if (n == 0) return CSM_OK;
  if (lc->stores.empty()) return lc->fail(CSM_ERR_INVALID_ARG, "map check: no kept scan of that id");
  std::vector<int32_t> ids((size_t)n, scan_id);
  std::vector<double> poses((size_t)n * 3);
  for (int32_t k = 0; k < n; ++k) std::memcpy(&poses[(size_t)3 * k], results[k].pose_world, 3 * sizeof(double));
  DeviceRestore restore;
  st = csm_gridmap_feedback_penalty_store(pub_map, lc->stores[r], n, ids.data(), poses.data(), param, penalties,
                                          nullptr);
  if (st != CSM_OK) return lc->fail(st, std::string("map check: ") + csm_gridmap_last_error(pub_map));
  return CSM_OK;
}

// SlamProcessor::ScanMatchInterface for every gated submap (csm_loop_closure.h). The rules around
// the correlative levels -- the box, the start pose, the mean, the penalty and the clamp -- are
// csm_lc_interface.hpp's.
int csm_loop_closure_scan_match(csm_loop_closure* lc, csm_gridmap* pub_map, int32_t scan_id,
                                const csm_loop_closure_interface_param* param, const double pose_world[3],
                                const double cov_init[9], csm_loop_closure_interface_result* results,
                                int32_t capacity, int32_t* n_pass) {
  if (!lc || !param || !pose_world || !n_pass || capacity < 0 || (capacity > 0 && !results) ||
      !(param->min_response == param->min_response))
    return CSM_ERR_INVALID_ARG;
  for (int l = 0; l < 3; ++l)
    if (param->levels[l].type == CSM_FAST) return CSM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(lc->mu);
  if (scan_id < 0 || (size_t)scan_id >= lc->scan_pts.size())
    return lc->fail(CSM_ERR_INVALID_ARG, "scan match: no kept scan of that id");
  size_t map_dev = 0;
  if (param->use_map_check) {
    if (!pub_map) return lc->fail(CSM_ERR_INVALID_ARG, "scan match: use_map_check without a pub map");
    csm::GridMapView view;
    const int vst = csm::gridmap_view(pub_map, &view);
    if (vst != CSM_OK) return lc->fail(vst, "scan match: the pub map gave no view");
    while (map_dev < lc->devices.size() && lc->devices[map_dev] != view.device) ++map_dev;
    if (map_dev == lc->devices.size())
      return lc->fail(CSM_ERR_INVALID_ARG, "scan match: the pub map lives on device " + std::to_string(view.device) +
                                               ", which is none of the loop closure's");
  }
  if (lc->n_submaps == 0) return lc->fail(CSM_ERR_NO_GRID, "no submaps set");
  const int32_t levels_run = param->use_fine_scan_match ? 3 : 1;
  // MapSizeCheck (scan_matchers.h:195-199) for every submap, before anything is launched: a submap
  // cannot grow here
  for (int32_t i = 0; i < lc->n_submaps; ++i) {
    const csm::InterfaceBox box = csm::interface_box(lc->resolution, &lc->offsets[2 * (size_t)i], pose_world,
                                                     param->range_max, param->levels[0].search_space_size);
    if (!csm::interface_box_fits(box, lc->size_x, lc->size_y))
      return lc->fail(CSM_ERR_UNSUPPORTED,
                      "scan match: MapSizeCheck would grow submap " + std::to_string(i) + " (" +
                          std::to_string(lc->size_x) + " x " + std::to_string(lc->size_y) + " cells); a submap of " +
                          std::to_string(csm::interface_size_that_fits(box, lc->size_x, lc->size_y)) +
                          " cells a side, centred the same, would have fit");
    // the fine levels convert poses with the stack's one geometry
    if (levels_run == 3 && (lc->offsets[2 * (size_t)i] != lc->stack_offset[0] ||
                            lc->offsets[2 * (size_t)i + 1] != lc->stack_offset[1]))
      return lc->fail(CSM_ERR_UNSUPPORTED, "scan match: submap " + std::to_string(i) +
                                               "'s offset is not the one its stack was set with (csm_map_info)");
  }
  // the query: CreateFrom(raw, 1 / resolution) (sensor_data_manager.h:99-115), rounded once
  const std::vector<double>& raw = lc->scan_pts[(size_t)scan_id];
  const int32_t n_points = (int32_t)(raw.size() / 2);
  const double factor = 1 / lc->resolution;
  std::vector<double> pts(raw.size());
  for (size_t i = 0; i < raw.size(); ++i) pts[i] = raw[i] * factor;

  // level 0: the gate and each passer's finish, as csm_loop_closure_match_gated_full
  // (no more entries than submaps can come back, whatever the caller's capacity)
  if (capacity > lc->n_submaps) capacity = lc->n_submaps;
  std::vector<csm_loop_closure_result> wide((size_t)capacity);
  std::vector<csm_match_result> wide_match((size_t)capacity);
  std::vector<double> covs((size_t)capacity * 9);
  static const double kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int32_t k = 0; k < capacity; ++k) std::memcpy(&covs[(size_t)9 * k], cov_init ? cov_init : kIdentity, sizeof(kIdentity));
  int st = lc_match_gated_full_locked(lc, pts.data(), n_points, &param->levels[0], pose_world, param->min_response,
                                      wide.data(), capacity, n_pass, covs.data(), wide_match.data());
  if (st != CSM_OK) return st;
  const int32_t m = *n_pass < capacity ? *n_pass : capacity;
  std::vector<double> poses((size_t)m * 3), resp((size_t)m * 3, 0.0);
  for (int32_t k = 0; k < m; ++k) {
    csm::interface_start_pose(wide_match[(size_t)k].accepted, wide[(size_t)k].pose_world, pose_world, &poses[(size_t)3 * k]);
    resp[(size_t)3 * k] = wide_match[(size_t)k].response;
  }
  // levels 1 and 2: each device's passers in one seeded call on its context, the devices concurrently
  const int G = (int)lc->devices.size();
  if (levels_run == 3 && m > 0) {
    std::vector<int> status((size_t)G, CSM_OK);
    std::vector<std::string> errs((size_t)G);
    auto run = [&](int r) {
      std::vector<int32_t> who, local;
      for (int32_t k = 0; k < m; ++k)
        if (lc_owner(lc, wide[(size_t)k].submap) == r) {
          who.push_back(k);
          local.push_back(wide[(size_t)k].submap - lc->lo[(size_t)r]);
        }
      const size_t n = who.size();
      if (n == 0) return;
      std::vector<double> gpts(n * pts.size()), gposes(n * 3), gcovs(n * 9), seed(n), scores(n, 0.0), lresp(2 * n, 0.0);
      std::vector<int64_t> goff(n + 1, 0);
      for (size_t j = 0; j < n; ++j) {
        const size_t k = (size_t)who[j];
        std::memcpy(gpts.data() + j * pts.size(), pts.data(), pts.size() * sizeof(double));
        goff[j + 1] = goff[j] + n_points;
        std::memcpy(&gposes[3 * j], &poses[3 * k], 3 * sizeof(double));
        std::memcpy(&gcovs[9 * j], &covs[9 * k], 9 * sizeof(double));
        seed[j] = resp[3 * k];
      }
      const int rc = csmh::scan_matchers_batch_grids_levels(lc->ctx[(size_t)r], (int32_t)n, gpts.data(), goff.data(),
                                                            local.data(), param->levels, 1, 1, seed.data(),
                                                            gposes.data(), gcovs.data(), scores.data(), lresp.data());
      if (rc != CSM_OK) {
        status[(size_t)r] = rc;
        errs[(size_t)r] = "device " + std::to_string(lc->devices[(size_t)r]) + ": " + csm_last_error(lc->ctx[(size_t)r]);
        return;
      }
      for (size_t j = 0; j < n; ++j) {
        const size_t k = (size_t)who[j];
        std::memcpy(&poses[3 * k], &gposes[3 * j], 3 * sizeof(double));
        std::memcpy(&covs[9 * k], &gcovs[9 * j], 9 * sizeof(double));
        resp[3 * k + 1] = lresp[j];
        resp[3 * k + 2] = lresp[n + j];
      }
    };
    DeviceRestore restore;
    if (!lc->workers) lc->workers.reset(new ShardWorkers(G));
    lc->workers->run(run);
    for (int r = 0; r < G; ++r)
      if (status[(size_t)r] != CSM_OK) return lc->fail(status[(size_t)r], errs[(size_t)r]);
  }
  // MapCheckPenalize at every entry's final pose, one launch (as csm_loop_closure_map_check)
  std::vector<double> penalty((size_t)m, 1.0);
  if (param->use_map_check && m > 0) {
    std::vector<int32_t> ids((size_t)m, scan_id);
    DeviceRestore restore;
    st = csm_gridmap_feedback_penalty_store(pub_map, lc->stores[map_dev], m, ids.data(), poses.data(), &param->check,
                                            penalty.data(), nullptr);
    if (st != CSM_OK) return lc->fail(st, std::string("scan match: map check: ") + csm_gridmap_last_error(pub_map));
  }
  for (int32_t k = 0; k < m; ++k) {
    csm_loop_closure_interface_result& R = results[k];
    R = csm_loop_closure_interface_result{};
    R.submap = wide[(size_t)k].submap;
    R.levels_run = levels_run;
    std::memcpy(R.pose, &poses[(size_t)3 * k], sizeof(R.pose));
    std::memcpy(R.cov, &covs[(size_t)9 * k], sizeof(R.cov));
    std::memcpy(R.response, &resp[(size_t)3 * k], sizeof(R.response));
    R.map_penalty = penalty[(size_t)k];
    R.score = csm::interface_score(csm::interface_mean(R.response, levels_run), R.map_penalty);
    R.wide = wide[(size_t)k];
    R.wide_match = wide_match[(size_t)k];
  }
  return CSM_OK;
}

int csm_loop_closure_matcher(csm_loop_closure* lc, int32_t shard, csm_ctx** ctx) {
  if (!lc || !ctx || shard < 0 || (size_t)shard >= lc->ctx.size()) return CSM_ERR_INVALID_ARG;
  *ctx = lc->ctx[(size_t)shard];
  return CSM_OK;
}

double csm_loop_closure_wide_gate(double threshold, int32_t levels_run) {
  return csm::interface_wide_gate(threshold, levels_run);
}

}  // extern "C"
