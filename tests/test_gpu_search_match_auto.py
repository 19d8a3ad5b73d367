"""GPU, end to end: csm_search_match's reduced finish and automatic capacity
(collect_capacity = CSM_COLLECT_AUTO), and csm_loop_closure_match_full, which
passes it.

The collected list stays on the device; a set larger than the context's reduce
minimum (CSM_LIST_REDUCE_MIN, default 8192) is finished from the subset a
device selection keeps (csrc/csm_select.hip, csrc/csm_search_match.hpp). The
truth is the oracle's scan_match, bit for bit, as in test_gpu_search_match.py,
whose scene, scans, shapes and helpers these tests share.

The large window: 9 x 41^2 = 15,129 candidates on a synthetic 93 x 77 grid with
a background near 0.55 and walls near 0.9 that the scan is cut from, so nearly
every candidate scores at or above T = 0.5 -- more than the default capacity of
10,240 -- while the top is unique. The grid's seed was picked with the oracle;
big_precondition asserts from the oracle's scores what the tests rely on."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402
import test_gpu_search_match as SM  # noqa: E402  (shared scene, shapes, oracle caches and checks)

RES, W, H = SM.RES, SM.W, SM.H
COARSE, FINE, SUPER = SM.COARSE, SM.FINE, SM.SUPER
COV0 = SM.COV0
AUTO = -1
DEFAULT_CAPACITY = 10240

BIG_NS, BIG_NA = 41, 9
BIG_SEED = 3
BIG_TRUE = (46.3, 38.2, 0.01)
BIG_OFF = (2.0, -1.0, 0.0)


def stat(ctx, name):
    for s in ctx.kernel_stats():
        if s["name"] == name:
            return int(s["launches"])
    return 0


def outputs(res, cov):
    """The 13 doubles a caller reads: response, pose, covariance."""
    return np.concatenate([[res["response"]], res["pose_map"], cov])


def big_grid(seed=BIG_SEED):
    """Multiples of 2^-16 (the fixed-point path): a background near 0.55, a
    two-cell-thick rectangular wall near 0.9 around the true pose, a seeded
    jitter on every cell."""
    rng = np.random.default_rng(seed)
    q = 2.0 ** -16
    g = (36045 + rng.integers(-1500, 1501, (H, W))) * q
    wall = np.zeros((H, W), dtype=bool)
    cx, cy = int(BIG_TRUE[0]), int(BIG_TRUE[1])
    wall[cy - 8:cy + 9, cx - 10:cx + 11] = True
    wall[cy - 6:cy + 7, cx - 8:cx + 9] = False
    g[wall] = (58982 + rng.integers(-1500, 1501, int(wall.sum()))) * q
    g32 = g.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), g)
    return g32


_big = {}


def big_case():
    """(grid, pts, pose_world, centre, param, oracle scores, oracle match) of the large window."""
    if not _big:
        g = big_grid()
        pts = SM._scan(g, BIG_TRUE, 100, BIG_SEED, radius=14.0, level=0.8, far=0.0)
        centre0 = np.array(BIG_TRUE) + np.array(BIG_OFF)
        pose_world = np.array([centre0[0] * RES, centre0[1] * RES, centre0[2]])
        m = O.Map(g, RES, outside=0.0)
        centre = O.world_to_map(m, pose_world)
        p = SM._param(BIG_NS, BIG_NA, False, COARSE)
        sc = O.score_window(m, pts, p, centre, BIG_NA * BIG_NS * BIG_NS)
        _big.update(g=g, pts=pts, pose_world=pose_world, centre=centre, p=p, sc=sc, m=m,
                    match=O.scan_match(m, pts, p, pose_world, COV0))
    return _big


def near_best_scores(sc, ns, bx, by, tol, T):
    """The scores >= T of the candidates within tol of (bx, by) in candidate units
    relative to the window's first candidate, descending."""
    flat = np.arange(sc.size)
    x, y = (flat // ns) % ns, flat % ns
    near = (np.abs(x - bx) <= tol) & (np.abs(y - by) <= tol) & (sc >= T)
    return np.sort(sc[near])[::-1]


def big_precondition():
    """From the oracle's scores: T = 0.5, more than 10,240 candidates at or
    above it, the band and the first 22 scores pairwise distinct, the
    near-best set's first 22 pairwise distinct. Returns |{s >= T}|."""
    B = big_case()
    sc = B["sc"]
    best = sc.max()
    assert best >= 0.6 and SM.cov_bound(best) == 0.5
    n_set = int((sc >= 0.5).sum())
    assert n_set > DEFAULT_CAPACITY, n_set
    order = np.sort(sc)[::-1]
    head = order[:max(22, SM.fb_count(sc))]
    assert np.unique(head).size == head.size, "equal scores in the band or the first 22"
    # the near-best set around FindBest's averaged pose (one cell: sres / mres = 1), in candidate units
    band = np.nonzero(sc - best >= -0.01)[0]
    w = sc[band]
    bx = float((((band // BIG_NS) % BIG_NS) * w).sum() / w.sum())
    by = float(((band % BIG_NS) * w).sum() / w.sum())
    nb = near_best_scores(sc, BIG_NS, bx, by, 1.0 + 1e-9, 0.5)[:22]
    assert nb.size >= 3 and np.unique(nb).size == nb.size, "equal scores among the near-best set's first 22"
    return n_set


def make_ctx(grids, reduce_min=None, profiling=True):
    """A context over a stack of grids; reduce_min: CSM_LIST_REDUCE_MIN as csm_create reads it."""
    import roborts_csm
    old = os.environ.get("CSM_LIST_REDUCE_MIN")
    try:
        if reduce_min is None:
            os.environ.pop("CSM_LIST_REDUCE_MIN", None)
        else:
            os.environ["CSM_LIST_REDUCE_MIN"] = str(reduce_min)
        c = roborts_csm.Context(0)
    finally:
        if old is None:
            os.environ.pop("CSM_LIST_REDUCE_MIN", None)
        else:
            os.environ["CSM_LIST_REDUCE_MIN"] = old
    c.set_outside_value(0.0)
    c.set_grid_stack(np.ascontiguousarray(grids, dtype=np.float32), RES, version=1)
    if profiling:
        c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def stack():
    return SM.R.scene(W, H)


@pytest.fixture(scope="module")
def ctx_reduce_all(stack):
    c = make_ctx(stack, reduce_min=0)
    yield c
    c.close()


# ---- 1. every set reduced (CSM_LIST_REDUCE_MIN=0) ---------------------------
@pytest.mark.parametrize("penalty", [False, True])
@pytest.mark.parametrize("typ", [COARSE, FINE, SUPER])
@pytest.mark.parametrize("shape", ["ns33a5", "ns21a9"])
def test_reduced_result_is_the_oracles(stack, ctx_reduce_all, shape, typ, penalty):
    ns, na = SM.SHAPES[shape][:2]
    p = SM._param(ns, na, penalty, typ)
    pts, _, centre = SM._case(stack, shape, 0)
    sc = SM._oracle_scores(stack, shape, 0, p)
    n_set = SM.pruned_precondition(sc, typ)
    ctx = ctx_reduce_all
    before = stat(ctx, "search_match:reduced")
    selects = stat(ctx, "list_select")
    cov = COV0.copy()
    res = ctx.search_match(pts, p, [0], [centre], cov, max_depth=2)
    assert res["path"] == 0 and res["collected"] == n_set, (res["path"], res["collected"], n_set)
    SM._check_full(res, cov, SM._oracle_match(stack, shape, 0, p), O.Map(stack[0], RES, outside=0.0), ns, na, sc)
    assert stat(ctx, "search_match:reduced") == before + 1
    assert stat(ctx, "list_select") > selects and stat(ctx, "search_match:reduce_overflow") == 0


# ---- 2. automatic capacity ---------------------------------------------------
def test_auto_capacity_grows_the_list_once():
    B = big_case()
    n_set = big_precondition()
    oracle = B["match"]
    ctx = make_ctx(B["g"][None])
    try:
        cov = COV0.copy()
        res = ctx.search_match(B["pts"], B["p"], [0], [B["centre"]], cov, collect_capacity=AUTO)
        assert res["path"] == 0 and res["collected"] == n_set, (res["path"], res["collected"], n_set)
        SM._check_full(res, cov, oracle, B["m"], BIG_NS, BIG_NA, B["sc"])
        assert stat(ctx, "search_match:regrown") == 1 and stat(ctx, "search_match:reduced") == 1
        want = outputs(res, cov)
        # the grown list is kept: a second identical call descends once
        cov2 = COV0.copy()
        res2 = ctx.search_match(B["pts"], B["p"], [0], [B["centre"]], cov2, collect_capacity=AUTO)
        assert res2["path"] == 0 and res2["collected"] == n_set
        assert stat(ctx, "search_match:regrown") == 1 and stat(ctx, "search_match:reduced") == 2
        assert SM._same_bits(outputs(res2, cov2), want)
    finally:
        ctx.close()


def test_default_capacity_overflows_explicit_capacity_reduces():
    B = big_case()
    n_set = big_precondition()
    ctx = make_ctx(B["g"][None])
    try:
        cov_auto = COV0.copy()
        auto = ctx.search_match(B["pts"], B["p"], [0], [B["centre"]], cov_auto, collect_capacity=AUTO)
        want = outputs(auto, cov_auto)
        # the default capacity: path 2, the exhaustive finish, the same 13 doubles
        cov = COV0.copy()
        res = ctx.search_match(B["pts"], B["p"], [0], [B["centre"]], cov, collect_capacity=0)
        assert res["path"] == 2 and res["collected"] == n_set
        assert SM._same_bits(outputs(res, cov), want)
        SM._check_full(res, cov, B["match"], B["m"], BIG_NS, BIG_NA, B["sc"])
    finally:
        ctx.close()
    # an explicit capacity that fits, the default reduce minimum: path 0 through the reduction
    ctx = make_ctx(B["g"][None])
    try:
        cov = COV0.copy()
        res = ctx.search_match(B["pts"], B["p"], [0], [B["centre"]], cov, collect_capacity=20000)
        assert res["path"] == 0 and res["collected"] == n_set
        assert stat(ctx, "search_match:reduced") == 1 and stat(ctx, "search_match:regrown") == 0
        assert SM._same_bits(outputs(res, cov), want)
    finally:
        ctx.close()


# ---- 3. planted fallbacks ----------------------------------------------------
def test_auto_capacity_tie_that_matters_is_path_1():
    """test_fallback_tie_matters' construction under automatic capacity: one
    point, two adjacent cells at 1.0 -> several candidates share the maximum."""
    g = np.zeros((1, H, W), dtype=np.float32)
    g[0, 30, 40] = g[0, 30, 41] = 1.0
    ctx = make_ctx(g, reduce_min=0)
    try:
        p = SM._param(21, 5, False, COARSE)
        pts = np.array([[0.2, 0.1]])
        m = O.Map(g[0], RES, outside=0.0)
        pose_world = np.array([38.0 * RES, 32.0 * RES, 0.0])
        centre = O.world_to_map(m, pose_world)
        sc = O.score_window(m, pts, p, centre, 5 * 21 * 21)
        assert (sc == sc.max()).sum() > 1 and sc.max() == 1.0
        cov = COV0.copy()
        res = ctx.search_match(pts, p, [0], [centre], cov, collect_capacity=AUTO)
        assert res["path"] == 1 and res["collected"] == int((sc >= 0.5).sum())
        SM._check_full(res, cov, O.scan_match(m, pts, p, pose_world, COV0), m, 21, 5, sc)
    finally:
        ctx.close()


def test_reduce_overflow_finishes_the_whole_list():
    """A plateau: every cell 0.75, one cell a little higher, one point. All
    15,129 candidates lie in FindBest's band, so selection A outgrows 10,240
    and the whole list is finished: the plateau's equal scores lie in the band,
    so that finish says a tie matters, and the result is the exhaustive one."""
    g = np.full((1, H, W), 0.75, dtype=np.float32)
    g[0, 38, 46] = 0.7578125
    ctx = make_ctx(g)
    try:
        p = SM._param(BIG_NS, BIG_NA, False, COARSE)
        pts = np.array([[0.2, 0.1]])
        m = O.Map(g[0], RES, outside=0.0)
        pose_world = np.array([46.0 * RES, 38.0 * RES, 0.0])
        centre = O.world_to_map(m, pose_world)
        n_cand = BIG_NA * BIG_NS * BIG_NS
        sc = O.score_window(m, pts, p, centre, n_cand)
        assert sc.max() == 0.7578125 and int((sc - sc.max() >= -0.01).sum()) == n_cand > DEFAULT_CAPACITY
        cov = COV0.copy()
        res = ctx.search_match(pts, p, [0], [centre], cov, collect_capacity=AUTO)
        assert res["collected"] == n_cand and res["path"] == 1, (res["collected"], res["path"])
        assert stat(ctx, "search_match:reduce_overflow") == 1 and stat(ctx, "search_match:reduced") == 0
        assert stat(ctx, "search_match:regrown") == 1
        SM._check_full(res, cov, O.scan_match(m, pts, p, pose_world, COV0), m, BIG_NS, BIG_NA, sc)
    finally:
        ctx.close()


# ---- 4. loop closure -----------------------------------------------------------
def test_loop_closure_match_full_small_stack(stack):
    """The existing three-submap stack: the result is the oracle's."""
    from roborts_csm.loop_closure import DeviceLoopClosure
    shape = "ns33a5"
    ns, na = SM.SHAPES[shape][:2]
    p = SM._param(ns, na, True, COARSE)
    pts = SM._case(stack, shape, 0)[0]
    offsets = np.array([[0.35, -0.2], [0.0, 0.0], [-0.15, 0.4]])
    true = np.array(SM.SHAPES[shape][2]) + np.array(SM.SHAPES[shape][3])
    pose_world = np.array([true[0] * RES - offsets[0, 0], true[1] * RES - offsets[0, 1], true[2]])
    lc = DeviceLoopClosure([0])
    try:
        lc.set_submaps(stack, RES, offsets, version=3)
        cov = COV0.copy()
        r, full = lc.match_full(pts, p, pose_world, cov)
        got_world = lc.last_pose_world.copy()
    finally:
        lc.close()
    g = r.submap
    m = O.Map(stack[g], RES, tuple(offsets[g]))
    resp, pose, ocov, front, _ = O.scan_match(m, pts, p, pose_world, COV0)
    assert SM._same_bits(full["response"], resp) and SM._same_bits(cov, ocov) and full["front"].flat_index == front
    assert full["accepted"] and SM._same_bits(got_world, pose), (got_world, pose)
    assert full["window"] == g and full["path"] in (0, 1, 2)


def test_loop_closure_match_full_large_window_is_pruned():
    """A stack whose winning window is the 15,129-candidate case: match_full
    passes CSM_COLLECT_AUTO, so the call is finished from the list (path 0),
    where the default capacity sent it through the exhaustive path 2."""
    from roborts_csm.loop_closure import DeviceLoopClosure
    B = big_case()
    n_set = big_precondition()
    low = np.full((H, W), 0.25, dtype=np.float32)
    grids = np.stack([low, B["g"], low])
    offsets = np.zeros((3, 2))
    lc = DeviceLoopClosure([0])
    try:
        lc.set_submaps(grids, RES, offsets, version=5)
        cov = COV0.copy()
        r, full = lc.match_full(B["pts"], B["p"], B["pose_world"], cov)
        got_world = lc.last_pose_world.copy()
    finally:
        lc.close()
    assert r.submap == 1 and full["window"] == 1
    m = O.Map(B["g"], RES, (0.0, 0.0))  # the loop closure's contexts keep the default outside value
    resp, pose, ocov, front, _ = O.scan_match(m, B["pts"], B["p"], B["pose_world"], COV0)
    assert full["path"] == 0 and full["collected"] == n_set, (full["path"], full["collected"], n_set)
    assert SM._same_bits(full["response"], resp) and SM._same_bits(cov, ocov) and full["front"].flat_index == front
    assert full["accepted"] and SM._same_bits(got_world, pose), (got_world, pose)
