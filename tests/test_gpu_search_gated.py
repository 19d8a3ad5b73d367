"""GPU: the gated search (csm_search_gated, csm_loop_closure_match_gated[_full]):
every window whose best score is at or above a response, with its argmax.

Truth is Context.best_windows (the exhaustive per-window argmax, itself pinned
to the oracle) filtered in numpy by score >= gate. The bar is identity: the
same windows in ascending order, the same score bits, flat index, x, y and
angle. Gates are taken from the truth's own bests, so equality with the gate
(the comparison is inclusive) and ties across windows are hit exactly."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import search_pyref as R  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


@pytest.fixture(scope="module")
def f1(golden_dir):
    return np.load(os.path.join(golden_dir, "f1_config1.npz"))


@pytest.fixture(scope="module")
def stack5(f1):
    """tests/test_gpu_search.py's stack: submap 4 == submap 2 (cross-window ties)."""
    rng = np.random.default_rng(41)
    base = np.stack([f1["grid"], np.roll(f1["grid"], 37, axis=0), np.roll(f1["grid"], -53, axis=1),
                     rng.choice(np.array([0.3, 0.5, 1.0], dtype=np.float32), size=f1["grid"].shape)])
    return np.concatenate([base, base[2:3]])


def _p5(penalty):
    from roborts_csm.params import CorrelationScanMatchParam
    return CorrelationScanMatchParam(2.0, 0.05, math.pi / 2, 0.0349, 0.5, 100, 0, penalty, 0)


def _centers5(f1, n):
    from roborts_csm.loop_closure import world_to_map
    return np.stack([world_to_map(f1["init_pose"], float(f1["resolution"]), f1["offset"])] * n)


@pytest.fixture(scope="module")
def ctx5(f1, stack5):
    """One context on stack5 and the truth per penalty, computed once."""
    import roborts_csm
    c = roborts_csm.Context(0)
    c.set_grid_stack(stack5, float(f1["resolution"]), version=3)
    gi = np.arange(stack5.shape[0])
    centers = _centers5(f1, stack5.shape[0])
    truth = {pen: c.best_windows(f1["points"], _p5(pen), gi, centers) for pen in (False, True)}
    yield c, gi, centers, truth
    c.close()


def _expect(truth, T, capacity=None):
    sc, flat, x, y, a = truth
    keep = np.nonzero(sc >= T)[0]
    m = keep.size if capacity is None else min(keep.size, capacity)
    k = keep[:m]
    return (k.tolist(), _bits(sc[k]), flat[k].tolist(), _bits(x[k]), _bits(y[k]), _bits(a[k]), int(keep.size))


def _got(r):
    w, sc, flat, x, y, a, n, st = r
    return (w.tolist(), _bits(sc), flat.tolist(), _bits(x), _bits(y), _bits(a), n), st


def _check(c, pts, p, gi, centers, T, truth, capacity=None, path=0, **kw):
    """search_gated at T equals the filtered truth; returns the stats."""
    from roborts_csm import _abi
    assert (_abi.GATE_PRUNED, _abi.GATE_OVERFLOW, _abi.GATE_UNPOOLED) == (0, 1, 2)
    got, st = _got(c.search_gated(pts, p, gi, centers, T, capacity=capacity, **kw))
    assert got == _expect(truth, T, capacity), (T, kw)
    assert st["path"] == path, st
    if path == 0:
        assert 1 <= st["descents"] <= 3, st
    else:
        assert st["descents"] == 0, st
    return st


# ---- 1. stack5: the gates of the issue's table --------------------------------
@pytest.mark.parametrize("depth,top_kernel", [(-1, 0), (0, 0), (1, 0), (3, 0), (3, 1)])
@pytest.mark.parametrize("penalty", [False, True])
def test_gates_on_stack5(f1, ctx5, penalty, depth, top_kernel):
    """The minimum (all 5, equality), the median (3; without the penalty
    windows 2 and 4 sit exactly on it and tie across windows), the maximum (1),
    the next double above it (0), and 0.0: all 5 out of some 765,000 candidates
    at or above the gate, far more than the list holds (how many of them are
    listed depends on the order they arrive in: stats.listed and the number of
    descents are not asserted)."""
    c, gi, centers, truth = ctx5
    sc = truth[penalty][0]
    p = _p5(penalty)
    import roborts_csm
    na, ns = roborts_csm.window_dims(p)
    if not penalty:
        assert sc[2] == sc[4] == np.median(sc)
    for T, n_pass in ((sc.min(), 5), (float(np.median(sc)), 3), (sc.max(), 1), (np.nextafter(sc.max(), np.inf), 0),
                      (0.0, 5)):
        st = _check(c, f1["points"], p, gi, centers, float(T), truth[penalty], max_depth=depth, top_kernel=top_kernel)
        assert _expect(truth[penalty], T)[-1] == n_pass
        assert st["candidates"] == 5 * na * ns * ns
        if depth >= 0:
            assert st["depth"] == depth
        if depth != 0 and T == sc.max():
            assert st["nodes"][0] < st["candidates"]  # pruning did something


# ---- 2. plateau: every candidate ties -------------------------------------------
@pytest.mark.parametrize("penalty", [False, True])
def test_plateau_takes_the_third_descent(f1, penalty):
    import roborts_csm
    from roborts_csm.params import CorrelationScanMatchParam
    g = np.full((3,) + f1["grid"].shape, 0.5, dtype=np.float32)
    p = CorrelationScanMatchParam(1.0, 0.05, 0.2, 0.0349, 0.5, 100, 0, penalty, 0)
    centers = np.array([[200.0, 200.0, 0.1]] * 3)
    gi = np.arange(3)
    na, ns = roborts_csm.window_dims(p)
    with roborts_csm.Context(0) as c:
        c.set_outside_value(0.5)
        c.set_grid_stack(g, float(f1["resolution"]), version=1)
        truth = c.best_windows(f1["points"], p, gi, centers)
        T = float(truth[0].max())
        if not penalty:
            assert truth[0].min() == T and truth[1].tolist() == [0, 0, 0]
            # every candidate ties at the gate: the count is deterministic and above 10240
            st = _check(c, f1["points"], p, gi, centers, T, truth, max_depth=3)
            assert st["listed"] == 3 * na * ns * ns > 10240
            assert st["descents"] == 3, st
            st = _check(c, f1["points"], p, gi, centers, T, truth, max_depth=3, list_capacity=64, path=1)
        else:
            _check(c, f1["points"], p, gi, centers, T, truth, max_depth=3)
            _check(c, f1["points"], p, gi, centers, float(truth[0].min()), truth, max_depth=3)


# ---- 3. a fixed list too small for the ties ---------------------------------------
def test_fixed_list_of_4_falls_back(f1, ctx5):
    """At the minimum gate at least 5 candidates hit, and at least 5 tie at
    their windows' maxima: a list of 4 overflows twice."""
    c, gi, centers, truth = ctx5
    for penalty in (False, True):
        T = float(truth[penalty][0].min())
        _check(c, f1["points"], _p5(penalty), gi, centers, T, truth[penalty], list_capacity=4, path=1)


def test_small_fixed_list_holds_the_ties(f1, ctx5):
    """A fixed list of 8 at the gate 0.0: some 765,000 candidates hit, and those
    that were a running maximum when they arrived do not fit 8 entries (in
    every run seen; the count depends on the arrival order, so it is not
    asserted). The second descent keeps the keys and lists only the candidates
    tied at their window's maximum -- one per window here, no window's best is
    tied -- which fit: the pruned path, never a third descent. Descending again
    without the keys overflows the fixed list again and takes the fallback."""
    c, gi, centers, truth = ctx5
    for penalty in (False, True):
        for T in (0.0, float(truth[penalty][0].min())):
            st = _check(c, f1["points"], _p5(penalty), gi, centers, T, truth[penalty], list_capacity=8)
            assert st["descents"] in (1, 2), st
            if st["descents"] == 2:
                assert st["listed"] == 5, st  # the ties alone: deterministic


# ---- 4. slices ------------------------------------------------------------------------
@pytest.mark.parametrize("node_capacity", [16, 64])
def test_sliced_levels(f1, ctx5, node_capacity):
    c, gi, centers, truth = ctx5
    from roborts_csm.params import CorrelationScanMatchParam
    p = CorrelationScanMatchParam(1.6, 0.05, 0.35, 0.0349, 0.5, 100, 0, True, 0)
    t = c.best_windows(f1["points"], p, gi, centers)
    for T in (float(np.sort(t[0])[-2]), float(t[0].max())):
        _check(c, f1["points"], p, gi, centers, T, t, max_depth=4, node_capacity=node_capacity)


# ---- 5. negative fixed point, windows off the grid ----------------------------------
@pytest.mark.parametrize("penalty", [False, True])
def test_negative_fixed_point_and_off_grid(f1, penalty):
    import roborts_csm
    from roborts_csm.params import CorrelationScanMatchParam
    rng = np.random.default_rng(7)
    g = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(2,) + f1["grid"].shape)
    sy, sx = g.shape[1:]
    p = CorrelationScanMatchParam(3.0, 0.05, 0.5, 0.0349, 0.5, 100, 0, penalty, 0)
    centers = np.array([[-20.0, 10.0, 0.3], [sx + 15.0, sy - 5.0, -1.0]])
    with roborts_csm.Context(0) as c:
        c.set_outside_value(0.75)
        c.set_grid_stack(g, float(f1["resolution"]), version=1)
        truth = c.best_windows(f1["points"], p, np.arange(2), centers)
        lo, hi = sorted(truth[0].tolist())
        # a negative gate; one between the two windows' bests (where the two
        # tie, as they do without the penalty, that is their common best: both
        # pass on equality)
        mid = 0.5 * (lo + hi)
        for T in (-0.25, mid):
            for top_kernel in (0, 1):
                _check(c, f1["points"], p, np.arange(2), centers, T, truth, max_depth=5, top_kernel=top_kernel)
        assert _expect(truth, -0.25)[-1] == 2 and _expect(truth, mid)[-1] == (1 if lo < hi else 2)


# ---- 6. windows outside the pooled search ---------------------------------------------
def test_unpooled_window_step(f1, ctx5):
    c, gi, centers, _ = ctx5
    from roborts_csm.params import CorrelationScanMatchParam
    p = CorrelationScanMatchParam(2.0, 2.0 * float(f1["resolution"]), 0.3, 0.0349, 0.5, 100, 0, True, 0)
    t = c.best_windows(f1["points"], p, gi, centers)
    for T in (float(np.median(t[0])), float(t[0].min()), float(np.nextafter(t[0].max(), np.inf))):
        _check(c, f1["points"], p, gi, centers, T, t, path=2)


# ---- 7. many windows -------------------------------------------------------------------------
def test_many_windows_percentile_gates():
    """300 windows on search_pyref.scene() (3 grids of 93 x 77, grid_index
    cycling), seeded centres of which some hang off the grid, a window of a few
    cells. Seed 71 was checked with the CPU oracle to give three different
    bests at the 10th, 50th and 90th percentile (asserted below on the truth)."""
    import roborts_csm
    from roborts_csm.params import CorrelationScanMatchParam
    g = R.scene()
    rng = np.random.default_rng(71)
    pts = rng.uniform(-25.0, 25.0, (60, 2))
    n = 300
    centers = np.stack([rng.uniform(-6.0, 99.0, n), rng.uniform(-6.0, 83.0, n), rng.uniform(-math.pi, math.pi, n)],
                       axis=1)
    assert ((centers[:, 0] < 0) | (centers[:, 0] > 93) | (centers[:, 1] < 0) | (centers[:, 1] > 77)).sum() >= 10
    gi = np.arange(n) % 3
    with roborts_csm.Context(0) as c:
        c.set_grid_stack(g, 0.05, version=1)
        for penalty in (False, True):
            p = CorrelationScanMatchParam(0.2, 0.05, 0.1, 0.0349, 0.5, 100, 0, penalty, 0)
            truth = c.best_windows(pts, p, gi, centers)
            s = np.sort(truth[0])
            gates = [float(s[30]), float(s[150]), float(s[270])]
            assert gates[0] < gates[1] < gates[2]
            counts = []
            for T in gates:
                _check(c, pts, p, gi, centers, T, truth)
                counts.append(_expect(truth, T)[-1])
            assert counts[0] >= 270 and 150 <= counts[1] < counts[0] and 30 <= counts[2] < counts[1]
            # fewer entries than passing windows; counting only
            _check(c, pts, p, gi, centers, gates[1], truth, capacity=7)
            got, st = _got(c.search_gated(pts, p, gi, centers, gates[1], capacity=0))
            assert got == ([], [], [], [], [], [], counts[1]) and st["path"] == 0


# ---- 8. later calls on the same context ------------------------------------------------------
def _later_calls(c, f1, stack5):
    p = _p5(True)
    gi = np.arange(stack5.shape[0])
    centers = _centers5(f1, stack5.shape[0])
    b, w, st = c.search_windows(f1["points"], p, gi, centers, max_depth=3)
    out = [(_bits([b.score, b.x, b.y, b.angle]), b.flat_index, w, st["nodes"])]
    cov = (np.eye(3) * 0.25).reshape(9).copy()
    r = c.search_match(f1["points"], p, gi, centers, cov, max_depth=3, collect_capacity=-1)
    f = r["front"]
    out.append((_bits([r["response"], r["threshold"], f.score, f.x, f.y, f.angle]), _bits(r["pose_map"]), _bits(cov),
                f.flat_index, r["accepted"], r["window"], r["count"], r["path"], r["collected"]))
    flat, score, nf = c.search_collect(f1["points"], p, int(w), centers[w], 3, float(b.score) - 0.01)
    assert 0 < nf <= flat.size
    out.append((flat[:nf].tolist(), _bits(score[:nf]), nf))
    return out


def _gated_all(c, f1, stack5):
    gi = np.arange(stack5.shape[0])
    centers = _centers5(f1, stack5.shape[0])
    out = []
    for T in (0.0, 0.8):
        got, st = _got(c.search_gated(f1["points"], _p5(True), gi, centers, T, max_depth=3))
        out.append((got, st["path"]))  # descents and nodes depend on the list's size and the arrival order
    return out


def test_later_calls_see_a_fresh_contexts_bits(f1, stack5):
    """A gated call that regrew the list (the plateau's third descent), then
    csm_search_windows, csm_search_match (CSM_COLLECT_AUTO) and
    csm_search_collect on that context: a fresh context's bits. And the other
    way round: after those calls (the match's collect uses and may regrow the
    same list), the gated call gives a fresh context's results and stats."""
    import roborts_csm
    from roborts_csm.params import CorrelationScanMatchParam
    res = float(f1["resolution"])
    plateau = np.full((3,) + f1["grid"].shape, 0.5, dtype=np.float32)
    pp = CorrelationScanMatchParam(1.0, 0.05, 0.2, 0.0349, 0.5, 100, 0, False, 0)
    used, fresh, fresh2 = (roborts_csm.Context(0) for _ in range(3))
    try:
        for c in (used, fresh, fresh2):
            c.set_outside_value(0.5)
        used.set_grid_stack(plateau, res, version=1)
        centers = np.array([[200.0, 200.0, 0.1]] * 3)
        T = float(used.best_windows(f1["points"], pp, np.arange(3), centers)[0].max())
        st = used.search_gated(f1["points"], pp, np.arange(3), centers, T, max_depth=3)[-1]
        assert st["descents"] == 3 and st["listed"] > 10240, st
        for c in (used, fresh, fresh2):
            c.set_grid_stack(stack5, res, version=2)
        assert _later_calls(used, f1, stack5) == _later_calls(fresh, f1, stack5)
        # the other way round: `used` and `fresh` have searched, matched and collected
        want = _gated_all(fresh2, f1, stack5)
        assert _gated_all(used, f1, stack5) == want
        assert _gated_all(fresh, f1, stack5) == want
    finally:
        for c in (used, fresh, fresh2):
            c.close()


# ---- 9. loop closure ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def submaps(f1):
    """tests/test_gpu_loop_closure.py's submaps, built the same way."""
    rng = np.random.default_rng(43)
    base = np.stack([f1["grid"], np.roll(f1["grid"], 29, axis=0), np.roll(f1["grid"], -41, axis=1),
                     rng.choice(np.array([0.3, 0.5, 1.0], dtype=np.float32), size=f1["grid"].shape)])
    grids = np.concatenate([base, base[1:2], base[:1]])  # duplicates: cross-submap ties
    offsets = np.tile(np.asarray(f1["offset"], dtype=np.float64), (grids.shape[0], 1))
    offsets[3] += (0.35, -0.2)
    return grids, offsets


def _devices():
    import ctypes as C
    n = C.c_int(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipGetDeviceCount(C.byref(n))
    return list(range(max(1, min(n.value, 8))))


def _lc_rows(results, pose_worlds):
    return [(r.submap, r.global_index, _bits([r.score, r.x, r.y, r.angle]), _bits(pw))
            for r, pw in zip(results, pose_worlds)]


@pytest.mark.parametrize("devices", ["one", "all"])
def test_loop_closure_match_gated(f1, submaps, devices):
    """Both device sets are held to the same truth (the per-submap filter of
    the Python shard's bests): the result does not depend on the device count."""
    import roborts_csm
    from roborts_csm.loop_closure import DeviceLoopClosure, worlds_to_map
    grids, offsets = submaps
    res = float(f1["resolution"])
    p = _p5(False)
    pose = np.array(f1["init_pose"], dtype=np.float64)
    S = grids.shape[0]
    na, ns = roborts_csm.window_dims(p)
    centers = worlds_to_map(pose, res, offsets)
    with roborts_csm.Context(0) as c:  # the Python shard's bests
        c.set_grid_stack(grids, res, version=5)
        sc, flat, x, y, a = c.best_windows(f1["points"], p, np.arange(S), centers)
    s = 1.0 / res
    inv_a = s * (1.0 / (s * s - 0.0 * 0.0))
    device_sets = [[0] if devices == "one" else _devices()]
    gates = (float(np.median(sc)), float(sc.min()), float(np.nextafter(sc.max(), np.inf)))
    per_set = []
    for devs in device_sets:
        lc = DeviceLoopClosure(devs)
        try:
            lc.set_submaps(grids, res, offsets, version=5)
            rows = []
            for T in gates:
                keep = np.nonzero(sc >= T)[0]
                want = [(int(k), int(k) * na * ns * ns + int(flat[k]), _bits([sc[k], x[k], y[k], a[k]]),
                         _bits([inv_a * x[k] + -(inv_a * (s * offsets[k][0])),
                                inv_a * y[k] + -(inv_a * (s * offsets[k][1])), a[k]])) for k in keep]
                out, n = lc.match_gated(f1["points"], p, pose, T, S)
                assert n == keep.size and [r.submap for r in out] == sorted(r.submap for r in out)
                assert _lc_rows(out, lc.last_pose_worlds) == want
                if out:
                    assert lc.last_n_devices == len(devs) and lc.last_exchange_ms == 0.0
                rows.append(_lc_rows(out, lc.last_pose_worlds))
                short, n2 = lc.match_gated(f1["points"], p, pose, T, 2)
                assert n2 == keep.size and _lc_rows(short, lc.last_pose_worlds) == want[:2]
                assert lc.match_gated(f1["points"], p, pose, T, 0) == ([], int(keep.size))
            per_set.append(rows)
        finally:
            lc.close()
    assert all(rows == per_set[0] for rows in per_set)  # the same result at 1 and at all devices


def test_loop_closure_match_gated_full(f1, submaps):
    import roborts_csm
    from roborts_csm.loop_closure import DeviceLoopClosure, worlds_to_map
    grids, offsets = submaps
    res = float(f1["resolution"])
    p = _p5(False)
    pose = np.array(f1["init_pose"], dtype=np.float64)
    S = grids.shape[0]
    centers = worlds_to_map(pose, res, offsets)
    cov0 = (np.eye(3) * 0.25).reshape(9)
    with roborts_csm.Context(0) as c:
        c.set_grid_stack(grids, res, version=5)
        sc = c.best_windows(f1["points"], p, np.arange(S), centers)[0]
        T = float(np.median(sc))
        keep = np.nonzero(sc >= T)[0]
        singles = []
        for k in keep:
            cov = cov0.copy()
            singles.append((c.search_match(f1["points"], p, [int(k)], centers[k:k + 1], cov, collect_capacity=-1), cov))
    lc = DeviceLoopClosure(_devices())
    try:
        lc.set_submaps(grids, res, offsets, version=5)
        covs = np.tile(cov0, (S, 1)).copy()
        out, n, matches = lc.match_gated_full(f1["points"], p, pose, T, S, covs)
        assert n == keep.size and [r.submap for r in out] == keep.tolist()
        s = 1.0 / res
        inv_a = s * (1.0 / (s * s - 0.0 * 0.0))
        for j, (k, m, (m1, cov1)) in enumerate(zip(keep, matches, singles)):
            assert m["window"] == int(k)
            for key in ("response", "threshold", "accepted", "count", "path", "collected"):
                assert m[key] == m1[key], (k, key)
            assert _bits(m["pose_map"]) == _bits(m1["pose_map"])
            fa, fb = m["front"], m1["front"]
            assert (_bits([fa.score, fa.x, fa.y, fa.angle]), fa.flat_index) == \
                   (_bits([fb.score, fb.x, fb.y, fb.angle]), fb.flat_index)
            assert _bits(covs[j]) == _bits(cov1)
            tx, ty = s * offsets[k][0], s * offsets[k][1]
            assert _bits(lc.last_pose_worlds[j]) == _bits([inv_a * m["pose_map"][0] + -(inv_a * tx),
                                                            inv_a * m["pose_map"][1] + -(inv_a * ty), m["pose_map"][2]])
        assert _bits(covs[len(keep):]) == _bits(np.tile(cov0, (S - len(keep), 1)))  # entries past n_pass untouched
    finally:
        lc.close()


# ---- 10. rejected calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["nan_gate", "fast", "negative_capacity"])
def test_rejected_call_leaves_the_context_usable(f1, stack5, bad):
    import roborts_csm
    from roborts_csm import _abi
    res = float(f1["resolution"])
    gi = np.arange(stack5.shape[0])
    centers = _centers5(f1, stack5.shape[0])
    used, fresh = (roborts_csm.Context(0) for _ in range(2))
    try:
        for c in (used, fresh):
            c.set_grid_stack(stack5, res, version=3)
        p = _p5(True)
        with pytest.raises(roborts_csm.CsmError) as e:
            if bad == "nan_gate":
                used.search_gated(f1["points"], p, gi, centers, float("nan"))
            elif bad == "fast":
                used.search_gated(f1["points"], p.with_(correlation_scan_match_type=_abi.FAST), gi, centers, 0.5)
            else:
                used.search_gated(f1["points"], p, gi, centers, 0.5, capacity=-1)
        assert e.value.status == _abi.CSM_ERR_INVALID_ARG

        def call(c):
            got, st = _got(c.search_gated(f1["points"], p, gi, centers, 0.8, max_depth=3))
            return got, st["path"]
        assert call(used) == call(fresh)
    finally:
        used.close()
        fresh.close()
