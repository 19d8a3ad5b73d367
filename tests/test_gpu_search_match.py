"""GPU: csm_search_match / csm_search_collect / csm_loop_closure_match_full --
the reference's full ScanMatch result (response, FindBestCandidate's averaged
pose, covariances) of the admissible search's winner window, from a collect of
the candidates at or above the covariance bound (csrc/csm_pyramid.hip
pyr_collect_kernel, csrc/csm_search.cpp collect, csrc/csm_search_match.cpp).

The truth is the oracle (oracle/pyoracle.py): score_window for the collected
sets, scan_match for response / pose / covariance. Every comparison is exact:
sets equal, doubles bit-equal.

The scans are cut out of the grid itself (occupied cells around a true pose,
seen from it), so a window has one peak and the scores at or above the bound
are a few hundred distinct values: the pruned path's precondition, which the
parity tests assert from the oracle's scores before they assert path == 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402
import search_pyref as R  # noqa: E402

RES = 0.05
W, H = 93, 77
ARES = 0.0349
COARSE, FINE, SUPER = 0, 1, 2
COV0 = np.array([7.0, -1.0, 2.0, 3.0, 8.0, -4.0, 5.0, 6.0, 9.0])  # in/out: entries a type leaves must survive
DEFAULT_CAPACITY = 10240


def _param(ns, n_angles, penalty, typ, res=RES, thr=0.0, use=200):
    from roborts_csm.params import CorrelationScanMatchParam
    import roborts_csm
    p = CorrelationScanMatchParam((ns - 1) * res, res, (n_angles - 1) / 2 * ARES + 0.002, ARES, thr, use, 0,
                                  bool(penalty), typ)
    assert roborts_csm.window_dims(p) == (n_angles, ns)
    return p


def _scan(grid, true_pose, n, seed, radius=30.0, level=0.75, far=0.3):
    """n points (60-120) in the sensor frame of true_pose (map cells, rad):
    cells of `grid` at or above `level` within `radius` cells, jittered inside
    the cell; a share `far` of the points lies 150-200 cells away, off the
    grid for every candidate. The scene's background sits near 0.5, the
    covariance bound's cap: with these points a window's scores away from the
    peak stay well below the bound."""
    rng = np.random.default_rng(seed)
    cx, cy, th = true_pose
    ys, xs = np.nonzero(grid >= level)
    near = (xs - cx) ** 2 + (ys - cy) ** 2 <= radius ** 2
    xs, ys = xs[near], ys[near]
    n_far = int(n * far)
    n_hit = n - n_far
    assert xs.size >= n_hit, (xs.size, n_hit)
    pick = rng.choice(xs.size, size=n_hit, replace=False)
    wx = xs[pick] + rng.uniform(-0.3, 0.3, n_hit)
    wy = ys[pick] + rng.uniform(-0.3, 0.3, n_hit)
    ang, rad = rng.uniform(0.0, 2.0 * np.pi, n_far), rng.uniform(150.0, 200.0, n_far)
    wx = np.concatenate([wx, cx + rad * np.cos(ang)])
    wy = np.concatenate([wy, cy + rad * np.sin(ang)])
    order = rng.permutation(n)
    wx, wy = wx[order], wy[order]
    c, s = np.cos(-th), np.sin(-th)
    dx, dy = wx - cx, wy - cy
    return np.ascontiguousarray(np.stack([c * dx - s * dy, s * dx + c * dy], axis=1))


# (ns, angles, true pose, window centre offset from it, points, seed, far share, cell level): the seeds of
# the first two are picked so that, for all three types with the penalty on and off, the oracle's scores at
# or above the bound are pairwise distinct, more than 20 (and more than 64, the capacity fallback's) and, in
# the first, FindBest's prefix holds two candidates (pruned_precondition asserts what the tests rely on)
SHAPES = {
    "ns33a5": (33, 5, (47.8, 39.8, -0.03), (3.0, -3.0, 0.0), 96, 3255, 0.25, 0.6),
    "ns21a9": (21, 9, (30.9, 40.1, 0.01), (-1.0, 3.0, 0.0), 120, 9329, 0.25, 0.6),
    "ns33a7_off": (33, 7, (9.4, 7.7, 0.05), (-3.0, -2.0, 0.0), 60, 13, 0.3, 0.75),    # hangs off the grid on two sides
    "ns21a5": (21, 5, (50.2, 40.9, 0.0), (1.0, 1.0, 0.0), 120, 14, 0.3, 0.75),
}


@pytest.fixture(scope="module")
def stack():
    return R.scene(W, H)


_cases = {}


def _case(stack, shape, grid=0):
    """(pts, pose_world, centre in map cells) of a shape on a grid of the stack."""
    key = (shape, grid)
    if key not in _cases:
        ns, na, true_pose, off, n, seed, far, level = SHAPES[shape]
        pts = _scan(stack[grid], true_pose, n, seed, level=level, far=far)
        centre = np.array(true_pose) + np.array(off)
        pose_world = np.array([centre[0] * RES, centre[1] * RES, centre[2]])
        m = O.Map(stack[grid], RES, outside=0.0)
        _cases[key] = (pts, pose_world, O.world_to_map(m, pose_world))
    return _cases[key]


_oracle = {}


def _oracle_scores(stack, shape, grid, p, outside=0.0):
    key = ("sc", shape, grid, bool(p.use_center_penalty), p.correlation_scan_match_type, outside)
    if key not in _oracle:
        pts, _, centre = _case(stack, shape, grid)
        ns, na = SHAPES[shape][:2]
        _oracle[key] = O.score_window(O.Map(stack[grid], RES, outside=outside), pts, p, centre, na * ns * ns)
    return _oracle[key]


def _oracle_match(stack, shape, grid, p, outside=0.0):
    key = ("sm", shape, grid, bool(p.use_center_penalty), p.correlation_scan_match_type, outside)
    if key not in _oracle:
        pts, pose_world, _ = _case(stack, shape, grid)
        _oracle[key] = O.scan_match(O.Map(stack[grid], RES, outside=outside), pts, p, pose_world, COV0)
    return _oracle[key]


def cov_bound(best):
    return min(best - 0.1, 0.5)


def fb_count(sc):
    return int(((sc - sc.max()) >= -0.01).sum())


def pruned_precondition(sc, typ, capacity=DEFAULT_CAPACITY):
    """The scores >= T are pairwise distinct and at most `capacity`; for
    COARSE / FINE at least 20 are > T (the rank-20 boundary is exercised).
    Returns their count."""
    T = cov_bound(sc.max())
    sel = sc[sc >= T]
    assert np.unique(sel).size == sel.size, "equal scores at or above the bound"
    assert sel.size <= capacity
    if typ in (COARSE, FINE):
        assert int((sc > T).sum()) >= 20
    return int(sel.size)


@pytest.fixture(scope="module")
def ctxs(stack):
    import roborts_csm
    made = {}

    def get(outside=0.0):
        if outside not in made:
            c = roborts_csm.Context(0)
            c.set_outside_value(outside)
            c.set_grid_stack(stack, RES, version=1)
            made[outside] = c
        return made[outside]

    yield get
    for c in made.values():
        c.close()


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check_full(res, cov, oracle, m, ns, na, sc=None):
    """A csm_search_match result against oracle.scan_match's, bit for bit."""
    r, pose, ocov, front, _ = oracle
    assert _same_bits(res["response"], r), (res["response"], r)
    assert _same_bits(cov, ocov), (cov, ocov)
    assert res["front"].flat_index == front, (res["front"].flat_index, front)
    assert res["accepted"] == (r > 0.0)  # response_threshold = 0
    if res["accepted"]:
        assert _same_bits(O.map_to_world(m, res["pose_map"]), pose), (res["pose_map"], pose)
    if sc is not None:
        assert res["count"] == fb_count(sc)
        assert res["front"].score == sc[front]
        assert res["threshold"] == cov_bound(sc.max())


# ---- 1. the collect hook ---------------------------------------------------
# (shape, grid of the stack, penalty, outside value)
COLLECT = [("ns33a5", 0, False, 0.0), ("ns21a9", 0, True, 0.0), ("ns33a7_off", 0, True, 0.0),
           ("ns21a5", 1, False, 0.0), ("ns21a5", 2, True, 0.75)]


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("shape,grid,penalty,outside", COLLECT)
def test_collect_is_the_oracles_set(stack, ctxs, shape, grid, penalty, outside, depth):
    ns, na = SHAPES[shape][:2]
    p = _param(ns, na, penalty, COARSE)
    pts, _, centre = _case(stack, shape, grid)
    sc = _oracle_scores(stack, shape, grid, p, outside)
    best = sc.max()
    at = np.sort(sc)[-max(40, sc.size // 50)]  # an existing score: the >= boundary
    ctx = ctxs(outside)
    for T in (cov_bound(best), 0.37 * best + 0.011, at):
        want = np.nonzero(sc >= T)[0]
        flat, score, n = ctx.search_collect(pts, p, grid, centre, depth, T)
        assert n == want.size, (T, n, want.size)
        assert np.array_equal(flat[:n], want)
        assert _same_bits(score[:n], sc[want])
    assert (sc == at).any() and (sc >= at).sum() > (sc > at).sum()


def test_collect_capacity_counts_and_stops(stack, ctxs):
    ns, na = SHAPES["ns21a9"][:2]
    p = _param(ns, na, True, COARSE)
    pts, _, centre = _case(stack, "ns21a9", 0)
    sc = _oracle_scores(stack, "ns21a9", 0, p)
    T = cov_bound(sc.max())
    want = np.nonzero(sc >= T)[0]
    cap = 7
    assert want.size > cap
    import ctypes as C
    import roborts_csm
    from roborts_csm import _lib
    flat = np.full(cap + 16, -5, dtype=np.int64)
    score = np.full(cap + 16, -5.0)
    n = C.c_int64(-1)
    cp = roborts_csm._as_param(p)
    ctx = ctxs(0.0)
    ctx._check(_lib.csm_search_collect(ctx._h, roborts_csm._dptr(pts), pts.shape[0], C.byref(cp), 0,
                                       roborts_csm._dptr(np.ascontiguousarray(centre)), 2, float(T),
                                       roborts_csm._i64ptr(flat), roborts_csm._dptr(score), cap, C.byref(n)))
    assert n.value == want.size                                # the full count
    assert (flat[cap:] == -5).all() and (score[cap:] == -5.0).all()  # nothing past the capacity
    assert np.isin(flat[:cap], want).all() and np.unique(flat[:cap]).size == cap
    assert _same_bits(score[:cap], sc[flat[:cap]])


def test_collect_unsupported_outside_the_pooled_search(stack, ctxs):
    import roborts_csm
    from roborts_csm import _abi
    p = _param(21, 5, False, COARSE, res=RES / 2)  # half-cell steps
    pts, _, centre = _case(stack, "ns21a5", 0)
    with pytest.raises(roborts_csm.CsmError) as e:
        ctxs(0.0).search_collect(pts, p, 0, centre, 2, 0.4)
    assert e.value.status == _abi.CSM_ERR_UNSUPPORTED


# ---- 2. pruned parity ------------------------------------------------------
@pytest.mark.parametrize("max_depth", [1, 2, 3])
@pytest.mark.parametrize("penalty", [False, True])
@pytest.mark.parametrize("typ", [COARSE, FINE, SUPER])
@pytest.mark.parametrize("shape", ["ns33a5", "ns21a9"])
def test_pruned_result_is_the_oracles(stack, ctxs, shape, typ, penalty, max_depth):
    ns, na = SHAPES[shape][:2]
    p = _param(ns, na, penalty, typ)
    pts, _, centre = _case(stack, shape, 0)
    sc = _oracle_scores(stack, shape, 0, p)
    n_set = pruned_precondition(sc, typ)
    cov = COV0.copy()
    res = ctxs(0.0).search_match(pts, p, [0], [centre], cov, max_depth=max_depth)
    assert res["path"] == 0 and res["collected"] == n_set, (res["path"], res["collected"], n_set)
    assert res["window"] == 0 and not res["search"]["exhaustive"] and res["search"]["depth"] == max_depth
    assert n_set <= res["collect_nodes"][0] <= sc.size and res["collect_nodes"][max_depth] > 0
    _check_full(res, cov, _oracle_match(stack, shape, 0, p), O.Map(stack[0], RES, outside=0.0), ns, na, sc)


# ---- 3. fallbacks ----------------------------------------------------------
def _zero_ctx(cells):
    import roborts_csm
    c = roborts_csm.Context(0)
    c.set_outside_value(0.0)
    g = np.zeros((1, H, W), dtype=np.float32)
    for (y, x) in cells:
        g[0, y, x] = 1.0
    c.set_grid_stack(g, RES, version=1)
    return c, g


def test_fallback_tie_matters():
    """One point, two adjacent cells at 1.0: several candidates share the
    maximum, std::sort's order among them decides the pose -> exhaustive."""
    c, g = _zero_ctx([(30, 40), (30, 41)])
    try:
        p = _param(21, 5, False, COARSE)
        pts = np.array([[0.2, 0.1]])
        m = O.Map(g[0], RES, outside=0.0)
        pose_world = np.array([38.0 * RES, 32.0 * RES, 0.0])
        centre = O.world_to_map(m, pose_world)
        sc = O.score_window(m, pts, p, centre, 5 * 21 * 21)
        assert (sc == sc.max()).sum() > 1 and sc.max() == 1.0
        cov = COV0.copy()
        res = c.search_match(pts, p, [0], [centre], cov)
        assert res["path"] == 1 and res["collected"] == int((sc >= 0.5).sum())
        _check_full(res, cov, O.scan_match(m, pts, p, pose_world, COV0), m, 21, 5, sc)
    finally:
        c.close()


def test_fallback_capacity(stack, ctxs):
    shape = "ns33a5"
    ns, na = SHAPES[shape][:2]
    p = _param(ns, na, True, COARSE)
    pts, _, centre = _case(stack, shape, 0)
    sc = _oracle_scores(stack, shape, 0, p)
    n_set = pruned_precondition(sc, COARSE)
    assert n_set > 64
    cov = COV0.copy()
    res = ctxs(0.0).search_match(pts, p, [0], [centre], cov, collect_capacity=64)
    assert res["path"] == 2 and res["collected"] == n_set
    _check_full(res, cov, _oracle_match(stack, shape, 0, p), O.Map(stack[0], RES, outside=0.0), ns, na, sc)


def test_fallback_half_cell_step(stack, ctxs):
    p = _param(21, 5, True, COARSE, res=RES / 2)
    pts, pose_world, centre = _case(stack, "ns21a5", 0)
    m = O.Map(stack[0], RES, outside=0.0)
    sc = O.score_window(m, pts, p, centre, 5 * 21 * 21)
    cov = COV0.copy()
    res = ctxs(0.0).search_match(pts, p, [0], [centre], cov)
    assert res["path"] == 3 and res["search"]["exhaustive"] and res["collected"] == 0
    _check_full(res, cov, O.scan_match(m, pts, p, pose_world, COV0), m, 21, 5, sc)


def test_fallback_no_response():
    """An all-zero grid, outside 0: best = 0 < 1e-6, the covariances' early
    return, no collect."""
    c, g = _zero_ctx([])
    try:
        p = _param(21, 5, False, COARSE)
        pts = np.random.default_rng(2).uniform(-20.0, 20.0, (60, 2))
        m = O.Map(g[0], RES, outside=0.0)
        pose_world = np.array([45.0 * RES, 38.0 * RES, 0.1])
        centre = O.world_to_map(m, pose_world)
        cov = COV0.copy()
        res = c.search_match(pts, p, [0], [centre], cov)
        assert res["path"] == 5 and res["collected"] == 0 and not res["accepted"] and res["response"] == 0.0
        want = np.array([500.0, 0.0, 0.0, 0.0, 500.0, 0.0, 0.0, 0.0, 4 * ARES * ARES])
        assert _same_bits(cov, want)
        r, pose, ocov, _, _ = O.scan_match(m, pts, p, pose_world, COV0)
        assert r == 0.0 and _same_bits(cov, ocov) and _same_bits(pose, pose_world)  # not accepted: the pose stays
    finally:
        c.close()


def test_min_response_skips_phase_two(stack, ctxs):
    shape = "ns21a9"
    ns, na = SHAPES[shape][:2]
    p = _param(ns, na, True, COARSE)
    pts, _, centre = _case(stack, shape, 0)
    sc = _oracle_scores(stack, shape, 0, p)
    assert sc.max() < 0.99
    cov = COV0.copy()
    ctx = ctxs(0.0)
    res = ctx.search_match(pts, p, [0], [centre], cov, min_response=0.99)
    assert res["path"] == 4 and _same_bits(cov, COV0) and res["collected"] == 0
    b, w, _ = ctx.search_windows(pts, p, [0], [centre])
    assert res["response"] == min(1.0, sc.max()) and res["window"] == w == 0
    assert (res["front"].score, res["front"].flat_index) == (b.score, b.flat_index) == (sc.max(), int(np.argmax(sc)))


# ---- 4. many windows -------------------------------------------------------
def test_many_windows_lower_window_wins(stack, ctxs):
    """Grid 2 is a copy of grid 0 and their windows share a centre: equal
    bests, the lower window wins, as csm_search_windows reports it."""
    shape = "ns21a9"
    ns, na = SHAPES[shape][:2]
    p = _param(ns, na, False, COARSE)
    pts, _, centre = _case(stack, shape, 0)
    other = centre + np.array([3.0, -2.0, 0.0])
    ctx = ctxs(0.0)
    for gi, ctr, win in (([0, 1, 2], [centre, other, centre], 0), ([1, 2, 0], [other, centre, centre], 1)):
        b, w, _ = ctx.search_windows(pts, p, gi, ctr)
        cov = COV0.copy()
        res = ctx.search_match(pts, p, gi, ctr, cov)
        assert res["window"] == w == win
        sc = _oracle_scores(stack, shape, 0, p)
        n_set = pruned_precondition(sc, COARSE)
        assert res["path"] == 0 and res["collected"] == n_set
        _check_full(res, cov, _oracle_match(stack, shape, 0, p), O.Map(stack[0], RES, outside=0.0), ns, na, sc)


# ---- 5. loop closure -------------------------------------------------------
def test_loop_closure_match_full(stack):
    from roborts_csm.loop_closure import DeviceLoopClosure, world_to_map
    shape = "ns33a5"
    ns, na = SHAPES[shape][:2]
    p = _param(ns, na, True, COARSE)
    pts = _case(stack, shape, 0)[0]
    offsets = np.array([[0.35, -0.2], [0.0, 0.0], [-0.15, 0.4]])
    true = np.array(SHAPES[shape][2]) + np.array(SHAPES[shape][3])
    pose_world = np.array([true[0] * RES - offsets[0, 0], true[1] * RES - offsets[0, 1], true[2]])
    lc = DeviceLoopClosure([0])
    try:
        lc.set_submaps(stack, RES, offsets, version=3)
        r0 = lc.match(pts, p, pose_world)
        cov = COV0.copy()
        r, full = lc.match_full(pts, p, pose_world, cov)
        got_world = lc.last_pose_world.copy()
    finally:
        lc.close()
    assert (r.score, r.global_index, r.submap, r.x, r.y, r.angle) == \
           (r0.score, r0.global_index, r0.submap, r0.x, r0.y, r0.angle)
    assert full["window"] == r.submap
    g = r.submap
    m = O.Map(stack[g], RES, tuple(offsets[g]))  # the loop closure's contexts keep the default outside value
    resp, pose, ocov, front, _ = O.scan_match(m, pts, p, pose_world, COV0)
    centre = world_to_map(pose_world, RES, offsets[g])
    assert _same_bits(centre, O.world_to_map(m, pose_world))
    assert _same_bits(full["response"], resp) and _same_bits(cov, ocov) and full["front"].flat_index == front
    assert full["accepted"] and _same_bits(got_world, pose), (got_world, pose)
    assert r.global_index == g * na * ns * ns + front and full["path"] in (0, 1, 2)
