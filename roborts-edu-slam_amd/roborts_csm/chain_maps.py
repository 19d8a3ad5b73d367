"""The matcher's grid stack drawn on the device from chains of kept scans
(include/csm_chain_maps.h).

The reference rebuilds a loop-closure or near-chain map for every call from
the chain's kept scans at the poses the pose graph holds at that moment
(SlamProcessor::ScanMatchInterface, slam_processor.cpp:250-326,
ResetScanMatchMapWithRangeVec :448-462). Here the kept scans live on the
device (ScanStore), their poses on the host, and set_grid_stack_chains draws
every submap of a query into a Context's grid stack with one fill and one
splat launch. Only the order-independent mode is built (ScanMatchMaps with
just_update_occu_ and the Gaussian blur); the other modes raise
CsmError(CSM_ERR_UNSUPPORTED) and remain with roborts_csm.gridmap.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import CsmError, _abi, _lib, kMapUnknownCellProb

_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)


@dataclass
class ChainMapParam:
    """csm_chain_map_param: the geometry and blur of every submap of a stack."""
    resolution: float
    deviation: float
    gaussian_blur_offset: float
    size_x: int
    size_y: int
    use_blur: bool = True
    default_cell_prob: float = float(kMapUnknownCellProb)

    def to_c(self) -> _abi.CsmChainMapParam:
        return _abi.CsmChainMapParam(float(self.resolution), float(self.deviation), float(self.gaussian_blur_offset),
                                     int(self.size_x), int(self.size_y), int(bool(self.use_blur)), 0,
                                     float(self.default_cell_prob), 0.0)


def _chain_arrays(chains):
    """chains: one sequence of scan ids per grid -> (offsets int32[n + 1], ids int32[>= 1])."""
    off = np.zeros(len(chains) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(c) for c in chains])
    ids = np.ascontiguousarray([i for c in chains for i in c], dtype=np.int32).reshape(-1)
    if ids.size == 0:
        ids = np.zeros(1, dtype=np.int32)  # never read: a pointer to pass
    return off, ids


class ScanStore:
    """csm_scan_store: the kept scans of SensorDataManager, resident on one device."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        st = _lib.csm_scan_store_create(int(device), C.byref(h))
        if st != _abi.CSM_OK:
            raise CsmError(st, f"csm_scan_store_create(device={device}) failed (no usable HIP device?)")
        self._h = h
        self.device = device

    def _check(self, st: int):
        if st != _abi.CSM_OK:
            raise CsmError(st, _lib.csm_scan_store_last_error(self._h).decode())

    def add(self, points_m, sensor_pose) -> int:
        """AddSensorData: sensor-frame end points in metres and the sensor pose -> the scan's id."""
        pts = np.ascontiguousarray(points_m, dtype=np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(sensor_pose, dtype=np.float64)
        assert pose.size == 3
        i = C.c_int32(-1)
        self._check(_lib.csm_scan_store_add(self._h, pts.ctypes.data_as(_dp), pts.shape[0], pose.ctypes.data_as(_dp),
                                            C.byref(i)))
        return int(i.value)

    def set_pose(self, scan_id: int, sensor_pose):
        """UpdateRangeData: the pose the next build draws the scan at."""
        pose = np.ascontiguousarray(sensor_pose, dtype=np.float64)
        assert pose.size == 3
        self._check(_lib.csm_scan_store_set_pose(self._h, int(scan_id), pose.ctypes.data_as(_dp)))

    def count(self) -> tuple[int, int]:
        """(kept scans, their points)."""
        n, p = C.c_int32(), C.c_int64()
        self._check(_lib.csm_scan_store_count(self._h, C.byref(n), C.byref(p)))
        return int(n.value), int(p.value)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.csm_scan_store_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def set_grid_stack_chains(ctx, store: ScanStore, param: ChainMapParam, chains, map_offset) -> _abi.CsmMapInfo:
    """csm_set_grid_stack_chains: grid g of ctx's stack = the ScanMatchMap of
    `param`'s geometry at `map_offset` drawn from the kept scans chains[g]
    (ids of `store`) at their stored poses -> the stack's csm_map_info."""
    off, ids = _chain_arrays(chains)
    mo = np.ascontiguousarray(map_offset, dtype=np.float64)
    assert mo.size == 2
    mp = param.to_c()
    info = _abi.CsmMapInfo()
    ctx._check(_lib.csm_set_grid_stack_chains(ctx._h, store._h, C.byref(mp), off.size - 1, off.ctypes.data_as(_i32p),
                                              ids.ctypes.data_as(_i32p), mo.ctypes.data_as(_dp), C.byref(info)))
    return info


def grid_download(ctx, grid_index: int, shape) -> np.ndarray:
    """csm_grid_download (a test hook): grid `grid_index` of ctx's resident
    stack as a float32 [size_y, size_x] array; shape = (size_y, size_x)."""
    out = np.empty((int(shape[0]), int(shape[1])), dtype=np.float32)
    ctx._check(_lib.csm_grid_download(ctx._h, int(grid_index), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
    return out
