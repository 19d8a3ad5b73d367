"""Loop-closure search sharded over GPUs.

The reference closes loops by matching a scan against the map around older
pose-chain candidates, one ScanMatchInterface call after another
(range_scan_pose_graph.cpp:299-355 TryCloseLoop, :120-167 LinkNearChains ->
slam_processor.cpp:301 -> ScanMatchers::ScanMatch). At loop-closure scale the
work is one query scan x many submaps x a large (x, y, theta) window, and the
answer is the single best candidate over all of them. Here:

* submaps are sharded by index across ranks, [r*S/G, (r+1)*S/G) resident on
  rank r (csm_set_grid_stack; no grid is replicated);
* each rank scores its submaps in one launch (csm_best_windows: argmax per
  window on the device) and reduces them to (best score, lowest global
  candidate index) -- global index = submap * n_cand + enumeration index;
* the one exchange step: all_reduce(MAX) of the score, then all_reduce(MIN)
  of the index among the ranks that hold that score, then the winner's
  (x, y, theta) from its owner (all_reduce(SUM) of a one-hot row). Over
  RCCL ("nccl") these are three 8-byte-scale collectives; the result does
  not depend on the rank count or order.

The scorer is anything with ``best_windows(points, param, grid_index,
centers) -> (scores, flat, x, y, angle)`` (search="exhaustive") or
``search_windows(points, param, grid_index, centers) -> (best, window,
stats)`` (search="pyramid", the admissible multi-resolution branch and
bound of csrc/csm_pyramid.hip: same answer, a fraction of the scorings):
the HIP context (roborts_csm.Context) in production.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import window_dims


def shard_range(n_submaps: int, rank: int, world: int) -> tuple[int, int]:
    """Submaps [lo, hi) of `rank` (contiguous, sizes differ by at most one)."""
    q, r = divmod(n_submaps, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def world_to_map(pose_world, resolution: float, offset) -> np.ndarray:
    """GridMapBase::GetMapCoordsPose (grid_map_base.h:68-69,89-93): Eigen's
    Scaling(1/res) * Translation(offset), evaluated in its order."""
    s = 1.0 / resolution
    return np.array([s * pose_world[0] + s * offset[0], s * pose_world[1] + s * offset[1], pose_world[2]])


def worlds_to_map(pose_world, resolution: float, offsets) -> np.ndarray:
    """world_to_map for every submap offset at once (the same expressions,
    elementwise: s * x + s * offset_x, with s = 1 / resolution)."""
    s = 1.0 / resolution
    off = np.asarray(offsets, dtype=np.float64).reshape(-1, 2)
    out = np.empty((off.shape[0], 3))
    out[:, 0] = s * pose_world[0] + s * off[:, 0]
    out[:, 1] = s * pose_world[1] + s * off[:, 1]
    out[:, 2] = pose_world[2]
    return out


@dataclass
class LoopClosureResult:
    score: float
    global_index: int   # submap * n_cand + enumeration index; -1: nothing scored
    submap: int
    x: float            # map cells of `submap`
    y: float
    angle: float


class ShardedLoopClosure:
    """One rank's share of the submaps and the exchange that merges ranks."""

    def __init__(self, scorer, n_submaps: int, resolution: float, offsets: np.ndarray,
                 rank: int = 0, world: int = 1, group=None, device=None, search: str = "pyramid"):
        assert search in ("pyramid", "exhaustive")
        self.scorer = scorer
        self.search = search
        self.last_stats = None
        self.n_submaps = int(n_submaps)
        self.resolution = float(resolution)
        self.lo, self.hi = shard_range(self.n_submaps, rank, world)
        self.offsets = np.asarray(offsets, dtype=np.float64).reshape(-1, 2)  # this shard's submaps
        assert self.offsets.shape[0] == self.hi - self.lo
        self.rank, self.world, self.group, self.device = rank, world, group, device

    def local_best(self, points_cells, param, pose_world) -> LoopClosureResult:
        n_loc = self.hi - self.lo
        if n_loc == 0:
            return LoopClosureResult(-np.inf, -1, -1, 0.0, 0.0, 0.0)
        na, ns = window_dims(param)
        n_cand = na * ns * ns
        centers = worlds_to_map(pose_world, self.resolution, self.offsets)
        if self.search == "pyramid":
            b, w, self.last_stats = self.scorer.search_windows(points_cells, param, np.arange(n_loc), centers)
            return LoopClosureResult(float(b.score), int((self.lo + w) * n_cand + b.flat_index), self.lo + w,
                                     float(b.x), float(b.y), float(b.angle))
        sc, flat, x, y, a = self.scorer.best_windows(points_cells, param, np.arange(n_loc), centers)
        gidx = (np.arange(self.lo, self.hi, dtype=np.int64) * n_cand + flat.astype(np.int64))
        best = np.max(sc)
        k = int(np.argmin(np.where(sc == best, gidx, np.iinfo(np.int64).max)))
        return LoopClosureResult(float(sc[k]), int(gidx[k]), self.lo + k, float(x[k]), float(y[k]), float(a[k]))

    def match(self, points_cells, param, pose_world) -> LoopClosureResult:
        loc = self.local_best(points_cells, param, pose_world)
        if self.world == 1:
            return loc
        import torch
        import torch.distributed as dist
        dev = self.device if self.device is not None else "cpu"
        s = torch.tensor([loc.score], dtype=torch.float64, device=dev)
        dist.all_reduce(s, op=dist.ReduceOp.MAX, group=self.group)
        mine = loc.global_index if (loc.global_index >= 0 and loc.score == float(s.item())) else np.iinfo(np.int64).max
        i = torch.tensor([mine], dtype=torch.int64, device=dev)
        dist.all_reduce(i, op=dist.ReduceOp.MIN, group=self.group)
        win = int(i.item())
        row = torch.zeros(4, dtype=torch.float64, device=dev)
        if win == loc.global_index:
            row[:] = torch.tensor([loc.submap, loc.x, loc.y, loc.angle], dtype=torch.float64)
        dist.all_reduce(row, op=dist.ReduceOp.SUM, group=self.group)
        r = row.cpu().numpy()
        return LoopClosureResult(float(s.item()), win, int(r[0]), float(r[1]), float(r[2]), float(r[3]))


class DeviceLoopClosure:
    """The same search and exchange behind the C-ABI (include/csm_loop_closure.h):
    one process, the submaps sharded over `devices`, an in-process RCCL
    communicator per device (ncclCommInitAll) carrying the MAX / MIN / SUM
    all-reduces. What the reference's C++ back end (TryCloseLoop,
    range_scan_pose_graph.cpp:299-355) would call; no torch involved."""

    def __init__(self, devices=(0,)):
        import ctypes as C
        from . import _lib
        self._C, self._lib = C, _lib
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        st = _lib.csm_loop_closure_create(devs.size, devs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h))
        if st != 0:
            msg = _lib.csm_loop_closure_last_error(h).decode() if h.value else "create failed"
            if h.value:
                _lib.csm_loop_closure_destroy(h)
            from . import CsmError
            raise CsmError(st, msg)
        self._h = h
        self.n_devices = devs.size

    def _check(self, st):
        if st != 0:
            from . import CsmError
            raise CsmError(st, self._lib.csm_loop_closure_last_error(self._h).decode())

    def set_submaps(self, grids: np.ndarray, resolution: float, offsets, version: int = -1):
        from ._abi import CsmMapInfo
        C = self._C
        g = np.ascontiguousarray(grids, dtype=np.float32)
        self._grids = g  # resident by host pointer: keep alive
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1, 2)
        assert off.shape[0] == g.shape[0]
        # the stack's own geometry carries the submaps' offset when they share one (what the level
        # drivers behind scan_match convert poses with; the searches take centres in map cells)
        same = bool(off.shape[0]) and bool(np.all(off == off[0]))
        info = CsmMapInfo(float(resolution), float(off[0, 0]) if same else 0.0, float(off[0, 1]) if same else 0.0,
                          g.shape[2], g.shape[1], 0, 0)
        self._check(self._lib.csm_loop_closure_set_submaps(self._h, g.ctypes.data_as(C.c_void_p), g.shape[0],
                                                           C.byref(info), off.ctypes.data_as(C.POINTER(C.c_double)),
                                                           int(version)))

    def add_scan(self, points_m, sensor_pose) -> int:
        """csm_loop_closure_add_scan: keep a scan (sensor-frame end points in
        metres, its sensor pose) on every device -> its id (0, 1, ...)."""
        C = self._C
        pts = np.ascontiguousarray(points_m, dtype=np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(sensor_pose, dtype=np.float64)
        assert pose.size == 3
        dp = C.POINTER(C.c_double)
        i = C.c_int32(-1)
        self._check(self._lib.csm_loop_closure_add_scan(self._h, pts.ctypes.data_as(dp), pts.shape[0],
                                                        pose.ctypes.data_as(dp), C.byref(i)))
        return int(i.value)

    def set_scan_pose(self, scan_id: int, sensor_pose):
        """csm_loop_closure_set_scan_pose: UpdateRangeData after a graph solve."""
        C = self._C
        pose = np.ascontiguousarray(sensor_pose, dtype=np.float64)
        assert pose.size == 3
        self._check(self._lib.csm_loop_closure_set_scan_pose(self._h, int(scan_id),
                                                             pose.ctypes.data_as(C.POINTER(C.c_double))))

    def set_submaps_chains(self, param, chains, current_pose):
        """csm_loop_closure_set_submaps_chains: submap i drawn on its device
        from the kept scans chains[i] (ids) at their stored poses, centred on
        current_pose. param: chain_maps.ChainMapParam."""
        from .chain_maps import _chain_arrays
        C = self._C
        off, ids = _chain_arrays(chains)
        pose = np.ascontiguousarray(current_pose, dtype=np.float64)
        assert pose.size == 3
        mp = param.to_c()
        i32p = C.POINTER(C.c_int32)
        self._check(self._lib.csm_loop_closure_set_submaps_chains(self._h, C.byref(mp), off.size - 1,
                                                                  off.ctypes.data_as(i32p), ids.ctypes.data_as(i32p),
                                                                  pose.ctypes.data_as(C.POINTER(C.c_double))))

    def match(self, points_cells, param, pose_world, search: str = "pyramid") -> LoopClosureResult:
        from . import _as_param
        from ._abi import CsmLoopClosureResult
        C = self._C
        pts = np.ascontiguousarray(points_cells, dtype=np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(pose_world, dtype=np.float64)
        p = _as_param(param)
        r = CsmLoopClosureResult()
        self._check(self._lib.csm_loop_closure_match(self._h, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0],
                                                     C.byref(p), pose.ctypes.data_as(C.POINTER(C.c_double)),
                                                     0 if search == "pyramid" else 1, C.byref(r)))
        self.last_pose_world = np.array(r.pose_world[:])
        self.last_n_devices = int(r.n_devices)
        self.last_search_ms, self.last_exchange_ms = float(r.search_ms), float(r.exchange_ms)
        return LoopClosureResult(r.score, r.global_index, r.submap, r.x, r.y, r.angle)

    def match_full(self, points_cells, param, pose_world, cov, search: str = "pyramid"):
        """csm_loop_closure_match_full: match(), then the winning submap's full
        ScanMatch result (csm_search_match on the device that holds it) ->
        (LoopClosureResult, match dict as Context.search_match returns it).
        cov (float64, 9) is in/out; last_pose_world is the averaged pose's
        world coordinates."""
        from . import _as_param, match_result_dict
        from ._abi import CsmLoopClosureResult, CsmMatchResult
        C = self._C
        pts = np.ascontiguousarray(points_cells, dtype=np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(pose_world, dtype=np.float64)
        assert cov.dtype == np.float64 and cov.flags.c_contiguous and cov.size == 9
        p = _as_param(param)
        r, m = CsmLoopClosureResult(), CsmMatchResult()
        dp = C.POINTER(C.c_double)
        self._check(self._lib.csm_loop_closure_match_full(self._h, pts.ctypes.data_as(dp), pts.shape[0], C.byref(p),
                                                          pose.ctypes.data_as(dp), 0 if search == "pyramid" else 1,
                                                          cov.ctypes.data_as(dp), C.byref(r), C.byref(m)))
        self.last_pose_world = np.array(r.pose_world[:])
        self.last_n_devices = int(r.n_devices)
        self.last_search_ms, self.last_exchange_ms = float(r.search_ms), float(r.exchange_ms)
        return LoopClosureResult(r.score, r.global_index, r.submap, r.x, r.y, r.angle), match_result_dict(m)

    def _gated(self, points_cells, param, pose_world, min_response, capacity, covs):
        from . import _as_param, match_result_dict
        from ._abi import CsmLoopClosureResult, CsmMatchResult
        C = self._C
        pts = np.ascontiguousarray(points_cells, dtype=np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(pose_world, dtype=np.float64)
        p = _as_param(param)
        cap = int(capacity)
        res = (CsmLoopClosureResult * max(cap, 1))()
        n = C.c_int32(-1)
        dp = C.POINTER(C.c_double)
        head = (self._h, pts.ctypes.data_as(dp), pts.shape[0], C.byref(p), pose.ctypes.data_as(dp),
                float(min_response), res if cap > 0 else None, cap, C.byref(n))
        matches = None
        if covs is None:
            self._check(self._lib.csm_loop_closure_match_gated(*head))
        else:
            assert covs.dtype == np.float64 and covs.flags.c_contiguous and covs.size >= 9 * cap
            matches = (CsmMatchResult * max(cap, 1))()
            self._check(self._lib.csm_loop_closure_match_gated_full(*head, covs.ctypes.data_as(dp) if cap > 0 else None,
                                                                    matches if cap > 0 else None))
        m = min(int(n.value), cap)
        self.last_pose_worlds = np.array([res[k].pose_world[:] for k in range(m)]).reshape(m, 3)
        if m:
            self.last_n_devices = int(res[0].n_devices)
            self.last_search_ms, self.last_exchange_ms = float(res[0].search_ms), float(res[0].exchange_ms)
        out = [LoopClosureResult(res[k].score, res[k].global_index, res[k].submap, res[k].x, res[k].y, res[k].angle)
               for k in range(m)]
        return out, int(n.value), ([match_result_dict(matches[k]) for k in range(m)] if matches is not None else None)

    def match_gated(self, points_cells, param, pose_world, min_response: float, capacity: int):
        """csm_loop_closure_match_gated: every submap whose best score is >=
        min_response -> (list of LoopClosureResult in ascending submap order,
        at most `capacity` of them; n_pass, the count of every such submap).
        last_pose_worlds: the entries' world poses, one row each."""
        out, n, _ = self._gated(points_cells, param, pose_world, min_response, capacity, None)
        return out, n

    def match_gated_full(self, points_cells, param, pose_world, min_response: float, capacity: int, covs):
        """csm_loop_closure_match_gated_full: match_gated, then each entry's
        full ScanMatch result -> (results, n_pass, list of match dicts as
        Context.search_match returns them). covs (float64, capacity x 9) is
        in/out per entry; last_pose_worlds: the averaged poses' world
        coordinates."""
        return self._gated(points_cells, param, pose_world, min_response, capacity, covs)

    def map_check(self, pub_map, scan_id: int, poses_world, check_point_num: int, bound_tolerance: float,
                  penalty_gain: float, use_blur: bool = False, use_logistic: bool = True) -> np.ndarray:
        """csm_loop_closure_map_check: MapCheckPenalize of the kept scan
        `scan_id` at each of poses_world (e.g. last_pose_worlds of a gated
        match) on pub_map (gridmap.OccuGridMap on one of this handle's
        devices), one launch -> penalties float64 [n]. The caller multiplies
        its response and clamps to 1 (slam_processor.cpp:318-319)."""
        from ._abi import CsmLoopClosureResult, CsmMapCheckParam
        C = self._C
        w = np.ascontiguousarray(poses_world, dtype=np.float64).reshape(-1, 3)
        n = w.shape[0]
        res = (CsmLoopClosureResult * max(n, 1))()
        for k in range(n):
            res[k].pose_world[:] = w[k].tolist()
        prm = CsmMapCheckParam(int(check_point_num), int(bool(use_blur)), int(bool(use_logistic)), 0,
                               float(bound_tolerance), float(penalty_gain))
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.csm_loop_closure_map_check(self._h, pub_map.handle, int(scan_id), C.byref(prm), res, n,
                                                         out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def scan_match(self, pub_map, scan_id: int, levels, pose_world, min_response: float, capacity: int,
                   range_max: float, use_fine_scan_match: bool = True, check=None, cov_init=None):
        """csm_loop_closure_scan_match: ScanMatchInterface's result (slam_processor.cpp:250-326) for
        every submap whose level-0 best is >= min_response -> (list of dicts in ascending submap
        order, at most `capacity`; n_pass). levels: the three CorrelationScanMatchParam of the call;
        check: None (no map check, pub_map may be None) or (check_point_num, bound_tolerance,
        penalty_gain[, use_blur[, use_logistic]]), the logistic on by default as ScanMatchInterface
        passes it. Each dict: submap, levels_run, pose (3,), cov (3, 3), score, response (3,),
        map_penalty, wide (LoopClosureResult), wide_pose_world, wide_match (as Context.search_match)."""
        from . import _as_param, match_result_dict
        from ._abi import CsmLoopClosureInterfaceParam, CsmLoopClosureInterfaceResult, CsmMapCheckParam
        C = self._C
        prm = CsmLoopClosureInterfaceParam()
        for k in range(3):
            prm.levels[k] = _as_param(levels[k])
        prm.use_fine_scan_match = int(bool(use_fine_scan_match))
        prm.use_map_check = int(check is not None)
        prm.range_max = float(range_max)
        prm.min_response = float(min_response)
        if check is not None:
            c = tuple(check) + (False, True)[len(check) - 3:] if len(check) < 5 else tuple(check)
            prm.check = CsmMapCheckParam(int(c[0]), int(bool(c[3])), int(bool(c[4])), 0, float(c[1]), float(c[2]))
        pose = np.ascontiguousarray(pose_world, dtype=np.float64)
        assert pose.size == 3
        dp = C.POINTER(C.c_double)
        cov_p = None
        if cov_init is not None:
            cov0 = np.ascontiguousarray(cov_init, dtype=np.float64).reshape(9)
            cov_p = cov0.ctypes.data_as(dp)
        cap = int(capacity)
        res = (CsmLoopClosureInterfaceResult * max(cap, 1))()
        n = C.c_int32(-1)
        self._check(self._lib.csm_loop_closure_scan_match(
            self._h, pub_map.handle if pub_map is not None else None, int(scan_id), C.byref(prm),
            pose.ctypes.data_as(dp), cov_p, res if cap > 0 else None, cap, C.byref(n)))
        out = []
        for k in range(max(0, min(int(n.value), cap))):
            r, w = res[k], res[k].wide
            out.append({"submap": int(r.submap), "levels_run": int(r.levels_run), "pose": np.array(r.pose[:]),
                        "cov": np.array(r.cov[:]).reshape(3, 3), "score": float(r.score),
                        "response": np.array(r.response[:]), "map_penalty": float(r.map_penalty),
                        "wide": LoopClosureResult(w.score, w.global_index, w.submap, w.x, w.y, w.angle),
                        "wide_pose_world": np.array(w.pose_world[:]), "wide_match": match_result_dict(r.wide_match)})
        return out, int(n.value)

    def matcher(self, shard: int):
        """The matcher context of device `shard` of the handle, borrowed (csm_set_profiling /
        kernel_stats around a call)."""
        from . import Context
        h = self._C.c_void_p()
        self._check(self._lib.csm_loop_closure_matcher(self._h, int(shard), self._C.byref(h)))
        return Context.borrow(h, self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.csm_loop_closure_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
