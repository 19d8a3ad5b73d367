"""The Gauss-Newton matcher with the whole solve in one launch
(csm_optimize_scan_match_batch_grids, optimize_solve_kernel): cost, pose and
iteration count equal the oracle (oracle/opt_oracle.cpp) and the host-loop
form (csm_optimize_scan_match_batch) bit for bit.

The committed F6 fixture at both parameter sets; scans whose lengths sit on the
edges of the kernel's 512-point LDS chunk; the 64 ray-cast scans of
test_optimize.py's batch test with their off-map and far-angle scans and four
parameter sets (no iteration, and 25 iterations with zero thresholds,
included); the reference's early returns; a stack of three grids with scans
pointed at them out of order; a scan whose angle is outside the device
sincos' domain (re-run by the host loop, counted); a context without the
device sincos (the whole call is the host loop's, counted); one launch per
call; a NaN step from an infinite cell.
"""
import os

import numpy as np
import pytest

import pyoracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import roborts_csm
    c = roborts_csm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def f1(golden_dir):
    return np.load(os.path.join(golden_dir, "f1_config1.npz"))


@pytest.fixture(scope="module")
def f6(golden_dir):
    return np.load(os.path.join(golden_dir, "f6_optimize.npz"))


def _prm(a):
    from roborts_csm.params import OptimizeScanMatchParam
    return OptimizeScanMatchParam(int(a[0]), float(a[1]), float(a[2]), float(a[3]), float(a[4]))


def _set(ctx, grid, res, off, update_index=0):
    import roborts_csm
    ctx.set_grid(roborts_csm.ScanMatchMap(grid, float(res), tuple(off), update_index, 0), force=True)


def _stat(ctx, name):
    return next((s for s in ctx.kernel_stats() if s["name"] == name), None)


def _oracle(m, points, offsets, prm, init):
    out = [O.optimize_scan_match(m, points[offsets[k]:offsets[k + 1]], prm, init[k]) for k in range(len(init))]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(-1, 3),
            np.array([o[2] for o in out], dtype=np.int32))


def _device(ctx, points, offsets, prm, init, grid_index=None):
    poses = np.ascontiguousarray(init, dtype=np.float64).copy()
    costs, iters = ctx.optimize_scan_match_batch_grids(points, offsets, grid_index, prm, poses)
    return costs, poses, iters


def _host_loop(ctx, points, offsets, prm, init):
    poses = np.ascontiguousarray(init, dtype=np.float64).copy()
    costs, iters = ctx.optimize_scan_match_batch(points, offsets, prm, poses)
    return costs, poses, iters


def _equal(a, b, what=None):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        same = x.view(np.uint64) == y.view(np.uint64) if x.dtype == np.float64 else x == y
        assert same.all(), (what, np.flatnonzero(~same.reshape(len(x), -1).all(axis=1))[:8])


def test_f6_fixture(ctx, f1, f6):
    _set(ctx, f1["grid"], f1["resolution"], f1["offset"])
    for tag in ("sim", "cfg"):
        got = _device(ctx, f6["points"], f6["offsets"], _prm(f6[f"param_{tag}"]), f6["init_poses"])
        _equal(got, (f6[f"cost_{tag}"], f6[f"pose_{tag}"], f6[f"iters_{tag}"].astype(np.int32)), tag)


def _smooth_grid(n, seed):
    """Occupancy-like values with gradients everywhere (a sum of a few waves)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    g = np.zeros((n, n))
    for _ in range(4):
        kx, ky, ph = rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 6.28)
        g += np.sin(kx * x + ky * y + ph)
    return (0.5 + g / 10.0).astype(np.float32)


def test_chunk_edges(ctx):
    """Scans of 1, 2, 511, 512, 513 and 1025 points: the edges of the 512-point chunk."""
    from roborts_csm.params import PARAM_CONFIG_OPTIMIZE, SIM_YAML_OPTIMIZE
    res, off = 0.05, (0.4, -0.3)
    grid = _smooth_grid(64, 41)
    rng = np.random.default_rng(42)
    sizes = [1, 2, 511, 512, 513, 1025]
    points = rng.uniform(-27.0, 27.0, size=(sum(sizes), 2))  # cells, sensor frame; some leave the 64 x 64 map
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    init = np.array([[32 * res - off[0] + dx, 32 * res - off[1] + dy, th]
                     for dx, dy, th in rng.normal(size=(len(sizes), 3)) * [0.1, 0.1, 0.3]])
    _set(ctx, grid, res, off)
    m = O.Map(grid, res, off)
    for prm in (SIM_YAML_OPTIMIZE, PARAM_CONFIG_OPTIMIZE):
        got = _device(ctx, points, offsets, prm, init)
        _equal(got, _oracle(m, points, offsets, prm, init), ("oracle", prm))
        _equal(got, _host_loop(ctx, points, offsets, prm, init), ("host loop", prm))
        assert (got[2] >= 1).all()


@pytest.fixture(scope="module")
def raycast():
    """test_optimize.py::test_device_batch_matches_oracle's batch."""
    from roborts_csm import worlds
    w = worlds.make_world(2000, 2000, 0.05, seed=11)
    b = worlds.make_scan_batch(w, 64, seed=12)
    init = b.init_poses.copy()
    init[5, :2] = [-w.offset[0] + 0.3, -w.offset[1] + 0.3]  # most endpoints off the map
    init[9, 2] += 1.5                                        # far off in angle
    return w, b, init


def test_raycast_batch(ctx, raycast):
    from roborts_csm.params import PARAM_CONFIG_OPTIMIZE, SIM_YAML_OPTIMIZE, OptimizeScanMatchParam
    w, b, init = raycast
    _set(ctx, w.grid, w.resolution, w.offset)
    m = O.Map(w.grid, w.resolution, w.offset)
    for prm in (SIM_YAML_OPTIMIZE, PARAM_CONFIG_OPTIMIZE, OptimizeScanMatchParam(25, 0.0, 0.0, 0.05, 0.05),
                OptimizeScanMatchParam(0, 0.1, 0.5, 0.5, 0.5)):
        got = _device(ctx, b.points_cells, b.offsets, prm, init)
        _equal(got, _oracle(m, b.points_cells, b.offsets, prm, init), ("oracle", prm))
        _equal(got, _host_loop(ctx, b.points_cells, b.offsets, prm, init), ("host loop", prm))


def test_one_launch_per_call(ctx, raycast):
    from roborts_csm.params import SIM_YAML_OPTIMIZE
    w, b, init = raycast
    assert SIM_YAML_OPTIMIZE.iterate_max_times == 10
    _set(ctx, w.grid, w.resolution, w.offset)
    ctx.set_profiling(True)
    try:
        _, _, iters = _device(ctx, b.points_cells, b.offsets, SIM_YAML_OPTIMIZE, init)
        solve = _stat(ctx, "optimize_solve_kernel")
        assert iters.max() > 1
        assert solve is not None and solve["launches"] == 1
        assert _stat(ctx, "optimize_cost_kernel") is None
        assert _stat(ctx, "optimize:host_scans")["launches"] == 0 and _stat(ctx, "optimize:host_batches") is None
    finally:
        ctx.set_profiling(False)


def test_early_returns(ctx, f1):
    from roborts_csm.params import SIM_YAML_OPTIMIZE
    pts = f1["points"]
    one = np.array([0, len(pts)], dtype=np.int64)
    pose = np.array([[0.1, 0.2, 0.3]])
    _set(ctx, f1["grid"], f1["resolution"], f1["offset"], update_index=-1)  # !IsMapInit (:73-76)
    costs, poses, iters = _device(ctx, pts, one, SIM_YAML_OPTIMIZE, pose)
    assert costs[0] == 1000.0 and np.array_equal(poses, pose) and iters[0] == 0
    _set(ctx, f1["grid"], f1["resolution"], f1["offset"])
    costs, poses, iters = _device(ctx, np.zeros((0, 2)), np.array([0, 0], dtype=np.int64), SIM_YAML_OPTIMIZE, pose)
    assert costs[0] == 1000.0 and np.array_equal(poses, pose) and iters[0] == 0
    # empty scans between real ones
    off = np.array([0, 0, len(pts), len(pts), 2 * len(pts)], dtype=np.int64)
    init = np.tile(np.asarray(f1["init_pose"], dtype=np.float64), (4, 1))
    costs, poses, iters = _device(ctx, np.vstack([pts, pts]), off, SIM_YAML_OPTIMIZE, init)
    m = O.Map(f1["grid"], float(f1["resolution"]), tuple(f1["offset"]))
    c, p, it = O.optimize_scan_match(m, pts, SIM_YAML_OPTIMIZE, f1["init_pose"])
    assert costs.tolist() == [1000.0, c, 1000.0, c] and iters.tolist() == [0, it, 0, it]
    assert np.array_equal(poses[1], p) and np.array_equal(poses[3], p)
    assert np.array_equal(poses[0], f1["init_pose"]) and np.array_equal(poses[2], f1["init_pose"])


def test_grid_stack(ctx):
    """Three grids, four scans pointed at them out of order: each equals the
    host-loop result with that grid set alone."""
    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.params import SIM_YAML_OPTIMIZE
    ws = [worlds.make_world(200, 200, 0.05, seed=s) for s in (51, 52, 53)]
    gidx = [2, 0, 1, 1]
    batches = [worlds.make_scan_batch(ws[g], 1, seed=60 + k) for k, g in enumerate(gidx)]
    points = np.vstack([b.points_cells for b in batches])
    offsets = np.concatenate([[0], np.cumsum([len(b.points_cells) for b in batches])]).astype(np.int64)
    # set_grid_stack places the stack at offset (0, 0): the worlds' poses move with their offset
    init = np.array([b.init_poses[0] + [ws[g].offset[0], ws[g].offset[1], 0.0] for b, g in zip(batches, gidx)])
    ctx.set_grid_stack(np.stack([w.grid for w in ws]), 0.05)
    costs, poses, iters = _device(ctx, points, offsets, SIM_YAML_OPTIMIZE, init, grid_index=gidx)
    for k, g in enumerate(gidx):
        _set(ctx, ws[g].grid, 0.05, (0.0, 0.0))
        pts = points[offsets[k]:offsets[k + 1]]
        one = np.array([0, len(pts)], dtype=np.int64)
        _equal((costs[k:k + 1], poses[k:k + 1], iters[k:k + 1]),
               _host_loop(ctx, pts, one, SIM_YAML_OPTIMIZE, init[k:k + 1]), k)
        c, p, it = O.optimize_scan_match(O.Map(ws[g].grid, 0.05, (0.0, 0.0)), pts, SIM_YAML_OPTIMIZE, init[k])
        assert costs[k] == c and np.array_equal(poses[k], p) and iters[k] == it and it > 1, k
    # a grid index outside the stack is rejected
    ctx.set_grid_stack(np.stack([w.grid for w in ws]), 0.05)
    for bad in ([2, 0, 3, 1], [2, -1, 1, 1]):
        with pytest.raises(roborts_csm.CsmError):
            _device(ctx, points, offsets, SIM_YAML_OPTIMIZE, init, grid_index=bad)


def test_domain_fallback(ctx, raycast):
    """One scan's angle outside the restated sincos' domain: the host loop runs
    that scan, the others are the kernel's."""
    from roborts_csm.params import SIM_YAML_OPTIMIZE
    w, b, init = raycast
    n = 6
    init = init[:n].copy()
    init[2, 2] = 2.0e8
    off = b.offsets[:n + 1]
    pts = b.points_cells[:off[-1]]
    _set(ctx, w.grid, w.resolution, w.offset)
    ctx.set_profiling(True)
    try:
        got = _device(ctx, pts, off, SIM_YAML_OPTIMIZE, init)
        assert _stat(ctx, "optimize:host_scans")["launches"] == 1
        assert _stat(ctx, "optimize_solve_kernel")["launches"] == 1
    finally:
        ctx.set_profiling(False)
    _equal(got, _oracle(O.Map(w.grid, w.resolution, w.offset), pts, off, SIM_YAML_OPTIMIZE, init))
    assert got[2][2] >= 1


def test_whole_batch_fallback(f1, f6, monkeypatch):
    """A context created without the device sincos: the host loop, same bits."""
    import roborts_csm
    monkeypatch.setenv("CSM_DEVICE_TRIG", "0")
    c = roborts_csm.Context(0)
    monkeypatch.delenv("CSM_DEVICE_TRIG")
    try:
        _set(c, f1["grid"], f1["resolution"], f1["offset"])
        c.set_profiling(True)
        got = _device(c, f6["points"], f6["offsets"], _prm(f6["param_sim"]), f6["init_poses"])
        assert _stat(c, "optimize:host_batches")["launches"] == 1
        assert _stat(c, "optimize_solve_kernel") is None and _stat(c, "optimize_cost_kernel")["launches"] >= 1
    finally:
        c.close()
    _equal(got, (f6["cost_sim"], f6["pose_sim"], f6["iters_sim"].astype(np.int32)))


def test_nan_step(ctx):
    """An infinite cell under an endpoint: b = -J e = -inf * 0, a NaN step.
    The reference returns kMaxCost and leaves the pose untouched (:103-106)."""
    from roborts_csm.params import SIM_YAML_OPTIMIZE
    res, off = 0.05, (0.0, 0.0)
    grid = _smooth_grid(64, 43)
    grid[30, 30] = np.inf
    rng = np.random.default_rng(44)
    pts0 = np.array([[0.4, 0.3], [5.2, 1.1], [-3.3, 2.2]])  # the first endpoint beside cell (30, 30)
    pts1 = rng.uniform(8.0, 20.0, size=(40, 2))              # a scan that stays clear of it
    points = np.vstack([pts0, pts1])
    offsets = np.array([0, 3, 43], dtype=np.int64)
    init = np.array([[30.1 * res, 30.2 * res, 0.0], [30.1 * res, 30.2 * res, 0.0]])
    m = O.Map(grid, res, off)
    want = _oracle(m, points, offsets, SIM_YAML_OPTIMIZE, init)
    assert want[0][0] == 1000.0 and np.array_equal(want[1][0], init[0]) and want[2][0] == 1  # the oracle's NaN return
    assert want[0][1] != 1000.0
    _set(ctx, grid, res, off)
    _equal(_device(ctx, points, offsets, SIM_YAML_OPTIMIZE, init), want)
