"""GPU: what the search entry points (csrc/csm_search_entry.cpp) share beyond
their results -- the profiling accounts, and the guard that leaves a context
usable after a rejected call. The scenes, scans and shapes are those of
test_gpu_search_match.py and test_gpu_search_match_auto.py (big_case: 15,129
candidates), whose tests pin the results themselves against the oracle.

1. Profiling accounting. With profiling on, one context runs one
   csm_search_windows, one csm_search_match finished from the whole list, one
   finished from the device selection under CSM_COLLECT_AUTO (the list grows
   once: two collects) and one csm_list_select. Every row of csm_kernel_stats
   -- pyramid_search, the top kernel's row, pyr_bound_kernel<...>, pyr_collect,
   list_select, search_match:* -- must hold the launches, algorithmic bytes and
   scorings of tests/golden/search_entry_stats.json, which
   tests/golden/make_search_entry_stats.py recorded from the library of the
   commit before the entry points moved into their own unit, twice on an
   MI355X. Times are not compared. Fields that differed between the two
   recordings are left out of the file and listed in its "unstable": none did.

2. A failed call leaves the context usable. Each of the five entry points is
   called with an argument it rejects once it holds the context (a grid_index
   outside the stack; near[3] = 0 for csm_list_select: CSM_ERR_INVALID_ARG,
   nothing launched), then with valid arguments; the valid call's outputs equal
   those of the same call on a fresh context, bit for bit."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_search_match as SM  # noqa: E402  (shared scene, shapes and oracle caches)
import test_gpu_search_match_auto as AUTO  # noqa: E402  (big_case, make_ctx)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_entry_stats.json")
SHAPE = "ns33a5"
REDUCE_MIN = 2048  # above SHAPE's collected set, below big_case's
FIELDS = ("launches", "algorithmic_bytes", "scorings")


def list_select_input():
    rng = np.random.default_rng(41)
    n = 70001
    return rng.permutation(n) / float(n) - 0.25, rng.permutation(n).astype(np.int64)


def profiled_rows():
    """The four calls on one profiling context -> {row name: {launches, algorithmic_bytes, scorings}}."""
    stack = SM.R.scene(SM.W, SM.H)
    ns, na = SM.SHAPES[SHAPE][:2]
    p = SM._param(ns, na, True, SM.COARSE)
    pts, _, centre = SM._case(stack, SHAPE, 0)
    n_small = SM.pruned_precondition(SM._oracle_scores(stack, SHAPE, 0, p), SM.COARSE)
    B = AUTO.big_case()
    n_big = AUTO.big_precondition()
    assert n_small <= REDUCE_MIN < n_big, (n_small, n_big)
    ctx = AUTO.make_ctx(stack, reduce_min=REDUCE_MIN)
    try:
        ctx.search_windows(pts, p, [0, 1, 2], [centre, centre, centre], max_depth=2)
        res = ctx.search_match(pts, p, [0], [centre], SM.COV0.copy(), max_depth=2)
        assert res["path"] == 0 and res["collected"] == n_small
        ctx.set_grid_stack(B["g"][None], SM.RES, version=2)
        res = ctx.search_match(B["pts"], B["p"], [0], [B["centre"]], SM.COV0.copy(), collect_capacity=AUTO.AUTO)
        assert res["path"] == 0 and res["collected"] == n_big
        score, flat = list_select_input()
        assert ctx.list_select(score, flat, 22)[2] == 22
        return {s["name"]: {f: s[f] for f in FIELDS} for s in ctx.kernel_stats()}
    finally:
        ctx.close()


def test_profiling_accounts_are_the_recorded_ones():
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    want = golden["rows"]
    got = profiled_rows()
    for name in ("pyramid_search", "pyr_collect", "list_select", "search_match:reduced", "search_match:regrown"):
        assert name in want, name  # the file holds what the test is about
    assert any(n.startswith("pyr_bound_kernel<") for n in want)
    assert want["pyr_collect"]["launches"] == 3 and want["list_select"]["launches"] > 2
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, row in want.items():
        for field, value in row.items():
            assert got[name][field] == value, (name, field, got[name][field], value)


# ---- 2. a rejected call, then a valid one -----------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _search_args(stack):
    shape = "ns21a9"
    ns, na = SM.SHAPES[shape][:2]
    pts, _, centre = SM._case(stack, shape, 0)
    return pts, SM._param(ns, na, True, SM.COARSE), centre


def _windows(ctx, stack, gi):
    pts, p, centre = _search_args(stack)
    b, w, st = ctx.search_windows(pts, p, [gi], [centre], max_depth=2)
    return _bits([b.score, b.x, b.y, b.angle]), b.flat_index, w, st["depth"], st["exhaustive"], st["candidates"]


def _match(ctx, stack, gi):
    pts, p, centre = _search_args(stack)
    cov = SM.COV0.copy()
    r = ctx.search_match(pts, p, [gi], [centre], cov, max_depth=2)
    f = r["front"]
    return (_bits([r["response"], r["threshold"], f.score, f.x, f.y, f.angle]), _bits(r["pose_map"]), _bits(cov),
            f.flat_index, r["accepted"], r["window"], r["count"], r["path"], r["collected"])


def _collect(ctx, stack, gi):
    pts, p, centre = _search_args(stack)
    T = SM.cov_bound(SM._oracle_scores(stack, "ns21a9", 0, p).max())
    flat, score, n = ctx.search_collect(pts, p, gi, centre, 2, T)
    assert 0 < n < flat.size
    return flat[:n].tolist(), _bits(score[:n]), n


def _bounds(ctx, stack, gi):
    pts, p, centre = _search_args(stack)
    return _bits(ctx.search_bounds(pts, p, [gi], [centre], 2, 2))


def _select(ctx, stack, gi):
    score, flat = list_select_input()
    near = (0.0, 0.0, 1.0, 0.0 if gi else 300.0, 120.0, 90.0, 40.0)  # n_space 0: rejected
    out_flat, out_score, n = ctx.list_select(score, flat, 22, band_on=True, best=0.7, near=near)
    assert n >= 22
    return out_flat[:n].tolist(), _bits(out_score[:n]), n


@pytest.mark.parametrize("call", [_windows, _match, _collect, _bounds, _select], ids=lambda f: f.__name__[1:])
def test_rejected_call_leaves_the_context_usable(call):
    import roborts_csm
    from roborts_csm import _abi
    stack = SM.R.scene(SM.W, SM.H)
    used, fresh = (AUTO.make_ctx(stack, profiling=False) for _ in range(2))
    try:
        with pytest.raises(roborts_csm.CsmError) as e:
            call(used, stack, stack.shape[0])  # one past the stack's last grid
        assert e.value.status == _abi.CSM_ERR_INVALID_ARG
        assert call(used, stack, 0) == call(fresh, stack, 0)
    finally:
        used.close()
        fresh.close()
