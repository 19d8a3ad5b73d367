"""The map publisher (include/csm_gridmap.h csm_gridmap_states and
csm_gridmap_occupancy_grid*, include/csm_frontend.h csm_frontend_publish_map;
SlamNode::PublishMapThread, roborts_slam_node.cpp:355-488): the device's grids
against the numpy restatement of tests/publish_pyref.py applied to the
oracle's cells, which the device's equal bit for bit. Tolerance 0 throughout:
states are bytes, info fields the same double expressions.

Two mutations of states_kernel, each built into a library of its own and run
against this file on an MI355X (3 of the 37 GPU tests fail under each):
  - the CountCell rule's `value < occu_threshold` as `<=`:
    test_count_cell_parameter_edges (cells whose value equals the threshold
    become free) and both front-end tests (cells at exactly 0.2) fail;
  - the linear index y * size_x + x replaced by x clamped to its row:
    test_states_of_a_box[*-wraps] on both maps (the box runs 58 columns past
    size_x, into the next rows' drawn cells) and
    test_count_cell_parameter_edges (with min_pass 0 the clamped cell is known,
    the cell past the array is -1) fail. The boxes "last_col" and "last_byte"
    alone cannot see it: column size_x is the next row's cell 0, and columns
    0, 1 and size_x - 1 are never drawn, so both reads give an untouched cell.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import map_scenarios as S
import publish_pyref as P
from map_engines import DeviceEngine, OracleEngine

gpu = pytest.mark.gpu

# scenario -> the CountCell (occu_threshold, min_pass) in force at its end
CELL = {"count_lines": (0.2, 3.0), "prob_lines_grow": (0.5, 2.0), "prob_occupied": (0.5, 2.0)}


@pytest.fixture(scope="module")
def maps():
    """name -> (scenario, oracle info, oracle prob, oracle pass, device map):
    every scenario built once, on the oracle and on the device."""
    scans = S.make_scans(4)
    out = {}
    for name in CELL:
        sc = S.scenarios()[name]
        a, _ = S.run(OracleEngine, sc, *scans)
        b, _ = S.run(DeviceEngine, sc, *scans)
        prob, pas = a.arrays()[:2]
        out[name] = (sc, a.m.info(), prob, pas, b.m)
    return out


def _expected(maps, name, full_map=False, cell=None):
    sc, info, prob, pas, _ = maps[name]
    return P.expected_grid(sc["kind"], prob, pas, info, sc["res"], cell or CELL[name], full_map)


@gpu
@pytest.mark.parametrize("full_map", [False, True])
@pytest.mark.parametrize("name", ["count_lines", "prob_lines_grow"])
def test_occupancy_grid_matches_restatement(maps, name, full_map):
    want_info, want = _expected(maps, name, full_map)
    info, grid = maps[name][4].OccupancyGrid(full_map=full_map)
    assert P.info_fields(info) == want_info
    assert grid.dtype == np.int8 and grid.shape == (want_info["height"], want_info["width"])
    assert np.array_equal(grid, want)
    assert P.info_fields(maps[name][4].OccupancyGridInfo(full_map)) == want_info
    if name == "count_lines" and not full_map:
        # an unaligned first column, a width and a byte count that are 2 mod 4
        assert (info.start_x, info.start_y, info.width, info.height) == (3, 34, 126, 171)
        assert {v: int((grid == v).sum()) for v in (-1, 0, 100)} == {-1: 17952, 0: 3494, 100: 100}


@gpu
def test_bound_never_set_is_an_empty_grid(maps):
    """prob_occupied never resizes, so its bound box stays (FLT_MAX, FLT_MIN):
    0 x 0 at start (0, 0), and the caller's buffer is not touched."""
    from roborts_csm import _abi
    from roborts_csm.gridmap import _lib
    m = maps["prob_occupied"][4]
    st = m.state()
    assert (st.bound_min_x, st.bound_max_x) == (P.FLT_MAX, P.FLT_MIN)
    want_info, want = _expected(maps, "prob_occupied")
    assert (want_info["width"], want_info["height"], want_info["start_x"], want_info["start_y"]) == (0, 0, 0, 0)
    info = _abi.CsmOccupancyGridInfo()
    buf = np.full(64, 7, dtype=np.int8)
    assert _lib.csm_gridmap_occupancy_grid(m.handle, 0, C.byref(info), buf.ctypes.data, buf.size) == _abi.CSM_OK
    assert P.info_fields(info) == want_info
    assert (buf == 7).all()
    info2, grid = m.OccupancyGrid()
    assert grid.shape == (0, 0) and P.info_fields(info2) == want_info
    # the full-map form of the same map is not empty
    want_info, want = _expected(maps, "prob_occupied", full_map=True)
    info3, grid = m.OccupancyGrid(full_map=True)
    assert P.info_fields(info3) == want_info and np.array_equal(grid, want)


@gpu
def test_argument_checks(maps):
    from roborts_csm import _abi
    from roborts_csm.gridmap import GridMapError, OccuGridMap, _lib
    m = maps["count_lines"][4]
    want_info, _ = _expected(maps, "count_lines")
    n = want_info["width"] * want_info["height"]
    info = _abi.CsmOccupancyGridInfo()
    buf = np.full(n, 7, dtype=np.int8)
    assert _lib.csm_gridmap_occupancy_grid(m.handle, 0, C.byref(info), buf.ctypes.data, n - 1) == \
        _abi.CSM_ERR_INVALID_ARG
    assert P.info_fields(info) == want_info and (buf == 7).all()
    for w, h in ((-1, 4), (4, -1), (65536, 32768)):  # negative sizes, 2^31 cells
        assert _lib.csm_gridmap_states(m.handle, 0, 0, w, h, buf.ctypes.data) == _abi.CSM_ERR_INVALID_ARG
    with pytest.raises(GridMapError) as e:
        m.GetGridStates(0, 0, -1, 4)
    assert e.value.status == _abi.CSM_ERR_INVALID_ARG
    assert (buf == 7).all()
    assert m.GetGridStates(5, 5, 0, 9, out=buf) is buf and m.GetGridStates(5, 5, 9, 0, out=buf) is buf
    assert (buf == 7).all()  # w * h == 0 does nothing
    fresh = OccuGridMap(0.05, (8, 8), (0.0, 0.0), 0.0, 0.5)
    p = C.c_void_p()
    assert _lib.csm_gridmap_occupancy_grid_end(fresh.handle, C.byref(p)) == _abi.CSM_ERR_INVALID_ARG
    # a second _begin before _end waits for the first; one _end then hands out the second grid
    full = _abi.CsmOccupancyGridInfo()
    assert _lib.csm_gridmap_occupancy_grid_begin(m.handle, 0, C.byref(info)) == _abi.CSM_OK
    assert _lib.csm_gridmap_occupancy_grid_begin(m.handle, 1, C.byref(full)) == _abi.CSM_OK
    assert _lib.csm_gridmap_occupancy_grid_end(m.handle, C.byref(p)) == _abi.CSM_OK
    want_full_info, want_full = _expected(maps, "count_lines", full_map=True)
    got = np.frombuffer((C.c_int8 * want_full.size).from_address(p.value), dtype=np.int8)
    assert P.info_fields(full) == want_full_info and np.array_equal(got.reshape(want_full.shape), want_full)
    assert _lib.csm_gridmap_occupancy_grid_end(m.handle, C.byref(p)) == _abi.CSM_ERR_INVALID_ARG


BOXES = [f"w{w}h{h}" for w in (1, 2, 3, 5) for h in (1, 7)] + ["w129", "last_col", "wraps", "last_byte",
                                                                "negative", "below"]


def _boxes(states):
    """name -> (x0, y0, w, h), placed from the oracle's states so that the
    boxes show drawn cells: the small ones lie around the first occupied cell,
    the ones past the row end in the rows of the leftmost drawn cell."""
    size_y, size_x = states.shape
    ay, ax = (int(v) for v in np.argwhere(states == 100)[0])
    drawn = np.argwhere(states != states[size_y - 1, size_x - 1])  # the last cell is never drawn
    drawn = drawn[drawn[:, 1] >= 2]  # nor are columns 0 and 1 (cell 0 holds default_cell_prob)
    ly, lx = (int(v) for v in drawn[np.argmin(drawn[:, 1])])
    assert lx < 55
    b = {}
    for w in (1, 2, 3, 5):      # a lane's four bytes span several box rows
        for h in (1, 7):
            b[f"w{w}h{h}"] = (ax - (w - 1) // 2, ay - (h - 1) // 2, w, h)
    b["w129"] = (max(ax - 100, 1), ay - 1, 129, 3)   # one past a whole number of dwords per row
    b["last_col"] = (size_x - 4, ly - 3, 5, 6)       # the last column is x = size_x: the next row's first cell
    b["wraps"] = (size_x - 2, ly - 3, 60, 5)         # far past size_x: the next rows' drawn cells
    b["last_byte"] = (size_x - 2, size_y - 3, 3, 3)  # ends at (size_x, size_y - 1): only that byte is past the array
    b["negative"] = (-2, -1, 7, 4)
    b["below"] = (ax - 2, size_y - 2, 6, 5)          # rows past the array
    assert sorted(b) == sorted(BOXES)
    return b


@gpu
@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("name", ["count_lines", "prob_lines_grow"])
def test_states_of_a_box(maps, name, box):
    sc, info, prob, pas, m = maps[name]
    states = P.cell_states(sc["kind"], prob, pas, *CELL[name])
    x0, y0, w, h = _boxes(states)[box]
    want = P.box_states(states, x0, y0, w, h)
    n = w * h
    buf = np.full(64 if n <= 64 else n + 64, 7, dtype=np.int8)  # the bytes past h * w stay as they were
    m.GetGridStates(x0, y0, w, h, out=buf)
    assert np.array_equal(buf[:n].reshape(h, w), want), (x0, y0, w, h)
    assert (buf[n:] == 7).all()
    if box == "last_byte":
        assert want[-1, -1] == -1
    if box == "negative":
        assert (want[0] == -1).all() and (want[:, :2] == -1).all()
    if box == "wraps":
        assert len(np.unique(want[:, 2:])) >= 2  # the wrapped part shows drawn cells
    if box == "w129" or (w > 1 and h > 1 and box[0] == "w"):
        assert len(np.unique(want)) >= 2


@gpu
def test_count_cell_parameter_edges(maps):
    """min_pass equal to a cell's pass count and occu_threshold equal to a
    cell's value, both picked from the oracle's cells so that both sides of
    `pass >= min_pass` and of `value < occu_threshold` occur in the box; with
    min_pass 0 every cell is known, and the byte past the array is still -1."""
    sc, info, prob, pas, m = maps["count_lines"]
    sx, sy, w, h = P.publish_box(info["bound"])
    x = sx + np.arange(w)[None, :]
    y = sy + np.arange(h)[:, None]
    lin = (y * info["size_x"] + x).ravel()
    bp, bv = pas.ravel()[lin], prob.ravel()[lin]
    passes = np.unique(bp[bp > 0])
    mp = float(passes[len(passes) // 2])
    known = bp >= np.float32(mp)
    vals = np.unique(bv[known])
    thr = float(vals[len(vals) // 2])
    assert (bp == np.float32(mp)).any() and (bp < np.float32(mp)).any() and (bp > np.float32(mp)).any()
    assert (bv[known] == np.float32(thr)).any() and (bv[known] < np.float32(thr)).any() \
        and (bv[known] > np.float32(thr)).any()
    try:
        for cell in ((thr, mp), (thr, 0.0), (0.5, 0.0)):
            m.set_cell_params(0.3, 0.7, *cell)
            got = m.GetGridStates(sx, sy, w, h)
            want = P.box_states(P.cell_states(1, prob, pas, *cell), sx, sy, w, h)
            assert np.array_equal(got, want), cell
            assert len(np.unique(want)) == (3 if cell[1] > 0 else 2)
            # the box that ends one cell past the array
            sxz, syz = info["size_x"], info["size_y"]
            got = m.GetGridStates(sxz - 2, syz - 3, 3, 3)
            want = P.box_states(P.cell_states(1, prob, pas, *cell), sxz - 2, syz - 3, 3, 3)
            assert np.array_equal(got, want) and want[-1, -1] == -1
            if cell[1] == 0.0:
                assert (want.ravel()[:-1] != -1).all()
    finally:
        m.set_cell_params(0.3, 0.7, *CELL["count_lines"])


# ---- the front end: test_frontend.py's 24-scan stream, `sim` parameters -----------------

N_SCANS, CORRECT_AFTER = 24, 12


@pytest.fixture(scope="module")
def recorded():
    """The oracle front end, run once: the expected grid after every scan and
    after the correction that follows scan CORRECT_AFTER, keyed by the
    PubMap's map_update_index. -> (stream, param, {index: (fields, grid)},
    keys in order, (ids, poses) of the correction)."""
    import pyoracle as O
    from roborts_csm.frontend import CsmFrontendResult
    from test_frontend import _corrections, _param, _stream
    st = _stream(N_SCANS, seed=4)
    prm = _param("sim")
    ofe = O.FrontEnd(prm.to_c())
    grids, keys, kept, correction = {}, [], [], None

    def record(first):
        m = ofe.map(0)
        prob, pas = m.cells()[:2]
        # UpdateMap's cell parameters (slam_processor.cpp:537-548): the first frame's, then the running ones
        cell = (0.5, 1.0) if first else (prm.map_occu_threshold, prm.map_min_passthrough)
        fields, grid = P.expected_grid(1, prob, pas, m.info(), prm.map_resolution, cell)
        keys.append(fields["map_update_index"])
        grids[fields["map_update_index"]] = (fields, grid)

    for k in range(N_SCANS):
        r = ofe.process(st.points_m[k], st.odom_poses[k], CsmFrontendResult())
        if r.map_updated:
            kept.append(np.array(r.pose[:]))
            record(len(kept) == 1)
        if k == CORRECT_AFTER:
            correction = _corrections(np.array(kept))
            ofe.correct_pose_and_map(*correction)
            record(False)
    return st, prm, grids, keys, correction


def test_recorded_key_is_unique_per_kept_scan(recorded):
    """CPU: map_update_index names one grid: it differs after every kept scan
    and after the correction, and the grids do change."""
    _, _, grids, keys, correction = recorded
    assert len(keys) == N_SCANS + 1 and len(set(keys)) == len(keys), keys
    assert keys == sorted(keys) and correction[0].size >= 3
    for fields, grid in grids.values():
        assert len(np.unique(grid)) == 3 and grid.shape == (fields["height"], fields["width"])


def _same(info, grid, grids):
    want_info, want = grids[info.map_update_index]
    assert P.info_fields(info) == want_info
    assert np.array_equal(grid, want), info.map_update_index


@gpu
def test_frontend_publish_interleaved(recorded):
    from roborts_csm.frontend import SlamFrontEnd
    st, prm, grids, keys, correction = recorded
    dfe = SlamFrontEnd(prm)
    try:
        info, grid = dfe.publish_map()  # before the first scan: no PubMap
        assert grid is None and info.map_update_index == -1 and (info.width, info.height) == (0, 0)
        seen, last = [], -1
        for k in range(N_SCANS):
            dfe.process(st.points_m[k], st.odom_poses[k])
            steps = [None] if k != CORRECT_AFTER else [None, correction]
            for step in steps:
                if step is not None:
                    dfe.correct_pose_and_map(*step)
                info, grid = dfe.publish_map(last)
                assert grid is not None, k
                _same(info, grid, grids)
                last = info.map_update_index
                seen.append(last)
                info, grid = dfe.publish_map(last)  # nothing new: roborts_slam_node.cpp:383
                assert grid is None and info.map_update_index == last
        assert seen == keys
    finally:
        dfe.close()


@gpu
def test_frontend_publisher_thread(recorded):
    """PublishMapThread beside the front end: a second thread publishes in a
    loop while this one processes the stream and, after scan CORRECT_AFTER,
    rebuilds the maps. Every grid it gets is the recorded one of its
    map_update_index: never a half-drawn scan, never a half-rebuilt map."""
    from roborts_csm.frontend import SlamFrontEnd
    st, prm, grids, keys, correction = recorded
    dfe = SlamFrontEnd(prm)
    stop = threading.Event()
    got, errors = [], []

    def publisher():
        last = -1
        try:
            while not stop.is_set():
                info, grid = dfe.publish_map(last)
                if grid is not None:
                    got.append((info, grid))
                    last = info.map_update_index
        except BaseException as e:  # reported by the main thread
            errors.append(e)

    t = threading.Thread(target=publisher, daemon=True)
    try:
        t.start()
        for k in range(N_SCANS):
            dfe.process(st.points_m[k], st.odom_poses[k])
            if k == CORRECT_AFTER:
                dfe.correct_pose_and_map(*correction)
        stop.set()
        t.join(timeout=60)
        assert not t.is_alive(), "the publisher thread did not end"
        assert not errors, errors
        info, grid = dfe.publish_map(got[-1][0].map_update_index if got else -1)
        if grid is not None:  # what the thread had not seen yet
            got.append((info, grid))
        assert got and got[-1][0].map_update_index == keys[-1]
        idx = [i.map_update_index for i, _ in got]
        print(f"publisher thread: {len(idx)} grids of {len(keys)} map states: {idx}")
        assert idx == sorted(set(idx)) and set(idx) <= set(keys), idx
        for info, grid in got:
            _same(info, grid, grids)
    finally:
        stop.set()
        t.join(timeout=60)
        if not t.is_alive():
            dfe.close()
