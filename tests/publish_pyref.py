"""Numpy restatement of what SlamNode::PublishMapThread computes of a map
(roborts_slam_node.cpp:355-488), shared by tests/test_publish_info.py (CPU)
and tests/test_gpu_map_publish.py (GPU): the two GetGridStates rules, the
node's cell loop over a box, the publish box and the origin. It is applied to
the oracle's cells, which the device's equal bit for bit
(map_engines.same_state). Paths cited are relative to the reference root."""
from __future__ import annotations

import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)   # util/boundbox.h:38: a bound box never set has
FLT_MIN = float(np.finfo(np.float32).tiny)  # min (FLT_MAX, FLT_MAX) and max (FLT_MIN, FLT_MIN) (:41-42)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def cell_states(kind, prob, pass_count, occu_threshold=0.5, min_pass=2.0):
    """GetGridStates of every cell as the node writes it (roborts_slam_node.cpp:
    405-419, 455-469): 100 occupied, 0 free, -1 unknown; float32 compares."""
    prob = np.asarray(prob, dtype=np.float32)
    if kind == 1:  # CountCellFunctions::GetGridStates, map/grid_map_cell.h:125-136
        known = np.asarray(pass_count, dtype=np.float32) >= np.float32(min_pass)
        return np.where(known, np.where(prob < np.float32(occu_threshold), 0, 100), -1).astype(np.int8)
    # ProbabilityCellFunctions::GetGridStates, map/grid_map_cell.h:367-375
    return np.where(prob < np.float32(0.5), 0, np.where(prob > np.float32(0.5), 100, -1)).astype(np.int8)


def box_states(states, x0, y0, w, h):
    """The node's loop over a box (roborts_slam_node.cpp:444-469): byte (j, i)
    is GetGridStates(x0 + i, y0 + j), the cell at the linear index
    y * size_x + x (GetCell, map/grid_map_base.h:315-317), so column size_x is
    the next row's first cell. A negative x or y or an index outside the array
    (undefined in the reference) gives -1."""
    size_y, size_x = states.shape
    flat = states.ravel()
    x = x0 + np.arange(w, dtype=np.int64)[None, :]
    y = y0 + np.arange(h, dtype=np.int64)[:, None]
    lin = y * size_x + x
    ok = (x >= 0) & (y >= 0) & (lin < flat.size)
    out = np.full((h, w), -1, dtype=np.int8)
    out[ok] = flat[lin[ok]]
    return out


def axis_size(mn, mx):
    """BoundBox::GetSizeX / GetSizeY (util/boundbox.h:99-111). A count or an end
    beyond int32, or a NaN bound, is undefined there; defined as 0 cells."""
    if math.isnan(mn) or math.isnan(mx) or math.isinf(mn) or math.isinf(mx):
        return 0
    lo, hi = math.floor(mn), math.ceil(mx)  # Python ints: exact
    d = hi - lo
    if d < 0:
        return 0
    if d + 1 > I32_MAX or lo < I32_MIN or hi > I32_MAX:
        return 0
    return d + 1


def publish_box(bound):
    """(start_x, start_y, width, height) of the bound-box form: GetStartGrid =
    floor(min) (map/grid_map_base.h:319-323), GetBoundSizeX/Y; an empty grid
    starts at (0, 0) (the reference's int start = floor(FLT_MAX) is undefined)."""
    mnx, mny, mxx, mxy = (float(v) for v in bound)
    w, h = axis_size(mnx, mxx), axis_size(mny, mxy)
    if w == 0 or h == 0:
        return 0, 0, w, h
    return math.floor(mnx), math.floor(mny), w, h


def origin(resolution, offset, start):
    """map_.info.origin.position (roborts_slam_node.cpp:427-430): the oracle's
    GetWorldCoords(start) minus half a cell, in Python doubles. `resolution`
    is the one the map was constructed with (scale_factor_ = 1 / resolution)."""
    import pyoracle as O
    m = O.Map(np.zeros((2, 2), dtype=np.float32), resolution, offset)
    wx, wy, _ = O.map_to_world(m, [float(start[0]), float(start[1]), 0.0])
    scale_factor = 1.0 / resolution
    half = 0.5 * (1 / scale_factor)
    return wx - half, wy - half, 1 / scale_factor


def expected_grid(kind, prob, pass_count, info, resolution, cell=(0.5, 2.0), full_map=False):
    """(fields, grid) of the OccupancyGrid for an oracle map: `info` its
    pyoracle.GridMap.info() dict, `cell` = (occu_threshold, min_pass)."""
    if full_map:  # kDisplayFullMap, roborts_slam_node.cpp:391-404
        sx, sy, w, h = 0, 0, info["size_x"], info["size_y"]
    else:
        sx, sy, w, h = publish_box(info["bound"])
    ox, oy, res = origin(resolution, info["offset"], (sx, sy))
    st = cell_states(kind, prob, pass_count, *cell)
    fields = dict(origin_x=ox, origin_y=oy, resolution=res, width=w, height=h, start_x=sx, start_y=sy,
                  map_update_index=info["map_update_index"])
    return fields, box_states(st, sx, sy, w, h)


def info_fields(info):
    """A csm_occupancy_grid_info as the dict expected_grid returns."""
    return {k: getattr(info, k) for k in ("origin_x", "origin_y", "resolution", "width", "height", "start_x",
                                          "start_y", "map_update_index")}
