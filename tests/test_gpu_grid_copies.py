"""When the copies derived from the fixed-point grid are rebuilt
(csrc/csm_grid_copies.hpp, csm_grid.cpp ensure_level_copies): the palette with
its strips and maps of uniform boxes, and the strip copies of gridi, are built
once per grid generation by the first level that reads them, and again after
every change of the resident grid: a row refresh, a cell refresh, another host
map, a map switched back in (no upload, but the copies are the context's and
follow grid_gen), a new outside value. Over the 400 x 400 f1 grid, one coarse
13 x 13 level (the pair box kernel) and one sub-cell fine level (the phase
kernel's strip form) per step: every score and the argmax bit for bit against
the CPU oracle, and the exact number of analyses and builds accounted in
kernel_stats() after each step. The counts follow from the code; they hold on
the commit before the copies became one record as well."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

from test_gpu_palette import _ctx, _stats  # noqa: E402

COUNTED = ("grid:analyze", "grid:palette", "grid:bg_map", "grid:istrips")


def _levels(n_points):
    from roborts_csm.params import SIM_YAML_LEVELS
    # 30 angles of 13 x 13 one-cell steps; 11 angles of 11 x 11 steps of 0.4 cells
    return [(SIM_YAML_LEVELS[0].with_(use_point_size=int(n_points)), 30 * 13 * 13, np.array([106.5, 206.5, 1.3])),
            (SIM_YAML_LEVELS[1].with_(use_point_size=int(n_points)), 11 * 11 * 11, np.array([100.53, 200.37, 0.1]))]


@pytest.fixture(scope="module")
def f1(golden_dir):
    return np.load(os.path.join(golden_dir, "f1_config1.npz"))


@pytest.fixture(scope="module")
def base(f1):
    """The f1 grid's oracle results, coarse then fine: shared, read only."""
    g = np.array(f1["grid"], dtype=np.float32)
    pts = np.ascontiguousarray(f1["points"])
    return g, pts, _oracle(g, float(f1["resolution"]), tuple(f1["offset"]), pts)


def _oracle(g, res, offset, pts, outside=0.3):
    m = O.Map(g, res, offset, outside=outside)
    return [(O.score_window(m, pts, lv, cen, n), O.best_window(m, pts, lv, cen)) for lv, n, cen in _levels(len(pts))]


def _score(c, pts, want, order=(0, 1)):
    levels = _levels(len(pts))
    for i in order:
        lv, _, cen = levels[i]
        scores, (s, flat) = want[i]
        assert np.array_equal(c.score_window(pts, lv, cen), scores), i
        got = c.best_window(pts, lv, cen)
        assert got.score == s and got.flat_index == flat, i


def _counts(c):
    st = _stats(c)
    counts = tuple(st[k]["launches"] if k in st else 0 for k in COUNTED)
    print(dict(zip(COUNTED, counts)))
    return counts


def test_copies_follow_the_grid(f1, base):
    import roborts_csm
    res, off = float(f1["resolution"]), tuple(f1["offset"])
    g0, pts, want0 = base
    g = g0.copy()
    a = roborts_csm.ScanMatchMap(g, res, off, 0, 1)
    c = _ctx()
    try:
        c.set_grid(a)
        _score(c, pts, want0)  # 1. the first coarse level builds the palette family, the first fine level the strips
        assert _counts(c) == (1, 1, 1, 1)
        st = _stats(c)
        assert "score_box_pair_kernel<13,all>" in st and "score_phase_kernel<11,all>" in st, st.keys()
        _score(c, pts, want0)  # 2. the same windows again: everything is current
        assert _counts(c) == (1, 1, 1, 1)
        g[150:170, :] = np.float32(0.8125)  # 3. rows refreshed with values the fixed-point copy holds exactly
        a.version = 2
        c.update_grid_rows(a, 150, 170)
        _score(c, pts, _oracle(g, res, off, pts))
        assert _counts(c) == (1, 2, 2, 2)
        idx = np.arange(200 * 400 + 100, 200 * 400 + 180, dtype=np.int32)  # 4. cells refreshed
        g.ravel()[idx] = np.float32(0.6875)
        a.version = 3
        c.update_grid_cells(a, idx)
        want_a = _oracle(g, res, off, pts)
        _score(c, pts, want_a)
        assert _counts(c) == (1, 3, 3, 3)
        gb = np.ascontiguousarray(np.roll(g0, 37, axis=0))  # 5. a second host map: A is parked
        c.set_grid(roborts_csm.ScanMatchMap(gb, res, off, 0, 1))
        _score(c, pts, _oracle(gb, res, off, pts))
        assert _counts(c) == (2, 4, 4, 4)
        uploads = _stats(c)["grid:upload"]["launches"]
        c.set_grid(a)  # 6. A again at its version: swapped back, no upload, no analysis; the copies are rebuilt
        _score(c, pts, want_a)
        assert _counts(c) == (2, 5, 5, 5)
        assert _stats(c)["grid:upload"]["launches"] == uploads == 2
        c.set_outside_value(0.5)  # 7. every fixed-point copy is shifted by the outside value
        _score(c, pts, _oracle(g, res, off, pts, outside=0.5))
        assert _counts(c) == (3, 6, 6, 6)
    finally:
        c.close()


@pytest.mark.parametrize("env,order,counts", [
    # the fine level first: its map of 5 x 5 boxes needs the palette, which the coarse level then finds current
    ({}, (1, 0), (1, 1, 1, 1)),
    # no maps of uniform boxes: the fine level alone builds no palette
    ({"CSM_BG_RUNS": "0"}, (1,), (1, 0, 0, 1)),
    # the v6 box kernel over gridi (no pair kernel): no palette for either level
    ({"CSM_KERNEL": "v8"}, (0, 1), (1, 0, 0, 1)),
])
def test_copies_built_on_demand(f1, base, env, order, counts):
    import roborts_csm
    g, pts, want = base
    c = _ctx(**env)
    try:
        c.set_grid(roborts_csm.ScanMatchMap(g, float(f1["resolution"]), tuple(f1["offset"]), 0, 1))
        _score(c, pts, want, order)
        assert _counts(c) == counts
        st = _stats(c)
        assert "score_phase_kernel<11,all>" in st, st.keys()
        assert ("grid:palette" in st) == (counts[1] > 0) and ("grid:bg_map" in st) == (counts[2] > 0)
    finally:
        c.close()
