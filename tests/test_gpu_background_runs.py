"""GPU parity of the pair box kernel's map of uniform boxes (csrc/csm_box.hip
score_box_pair_kernel<.., BG>, csrc/csm_palette.hip bg_map_kernel).

A beam whose whole 13 x 13 box holds the grid's background value adds that
value to every candidate: the kernel drops it from its run lists, counts it,
and adds count * value to the integer sums once. The bar is the one of every
other kernel: all scores bit for bit against the CPU oracle, the argmax index
equal; and the same context with CSM_BG_RUNS=0 (the map never built) gives the
same bits. The grids here have a background other than the outside value
(0.5 against 0.3) unless a test says otherwise: in the fixed-point grid the
outside value is 0, so only such a background makes the added constant
non-zero, and a kernel that forgot it would fail.

The fine level's phase kernel (csrc/csm_phase.hip, BG) does the same with a
second map of 5 x 5 boxes.

Covered: the box's extent (one odd cell just outside and just inside every
side of a box, 13 x 13 and 5 x 5, with the exact number of set corners),
boxes partly and wholly uniform in the run-list form (200 beams, and 700:
two run-list segments) and the run-free form (70 beams), the fine level over
the same grid, windows whose corners lie in the strips' low padding and at the high edge, a
background equal to the outside value, a grid with no dominant value (no set
bit: the map is unused), a stack of two grids with different backgrounds, and
one 3-level batch match.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

RES = 0.05
BG = np.float32(0.5)
NA, NS = 30, 13  # the coarse level's window: 30 angles of 13 x 13 one-cell steps


def _level(n_points):
    from roborts_csm.params import SIM_YAML_LEVELS
    return SIM_YAML_LEVELS[0].with_(use_point_size=int(n_points))


def _ctx(**env):
    """A context whose single-window calls take the throughput kernels
    (CSM_SMALL=0: not the few-window split kernel)."""
    import roborts_csm
    env = dict({"CSM_SMALL": "0"}, **env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = roborts_csm.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def ctxs():
    """The map in use (the default) and never built."""
    on, off = _ctx(), _ctx(CSM_BG_RUNS="0")
    yield on, off
    on.close()
    off.close()


def _stats(c):
    return {k["name"]: k for k in c.kernel_stats()}


_SEEN = {}


def _set_bits(c, name="grid:bg_map"):
    """Set bits of the maps built since the last call (grid:bg_map, and
    grid:bg_map5 for the 5 x 5 map, account them as scorings; a map is built
    by the first launch that reads a grid)."""
    total = _stats(c).get(name, {"scorings": 0})["scorings"]
    new = total - _SEEN.get((id(c), name), 0)
    _SEEN[(id(c), name)] = total
    return new


def _corners_set(sx, sy, n):
    """Set corners of an all-background sx x sy grid with one odd cell away
    from its edges: a box is uniform when it lies within columns -1 .. sx - 1
    and rows -1 .. sy - 1 of the padded image (column -1 and row -1 repeat the
    grid's first, everything further out holds the outside value) and misses
    the odd cell, which n * n boxes hold."""
    return (sx - n + 2) * (sy - n + 2) - n * n


def _set(ctxs, g):
    import roborts_csm
    for c in ctxs:
        c.set_grid(roborts_csm.ScanMatchMap(g, RES, (0.0, 0.0), 0, 1), force=True)
    return O.Map(g, RES, (0.0, 0.0))


def _check(ctxs, m, pts, centers):
    lv = _level(pts.shape[0])
    on, off = ctxs
    for cen in centers:
        want = O.score_window(m, pts, lv, cen, NA * NS * NS)
        s, flat = O.best_window(m, pts, lv, cen)
        for c in (on, off):
            assert np.array_equal(c.score_window(pts, lv, cen), want), cen
            got = c.best_window(pts, lv, cen)
            assert got.score == s and got.flat_index == flat, cen
    st = _stats(on)
    assert "score_box_pair_kernel<13,all>" in st and "score_box_pair_kernel<13,best>" in st, st.keys()
    assert "grid:bg_map" not in _stats(off)


def _banded(n=128):
    """All background but two blurred wall bands (five values with the background)."""
    g = np.full((n, n), BG, dtype=np.float32)
    for d, v in ((0, 1.0), (1, 0.875), (2, 0.75), (3, 0.625)):
        for s in (-1, 1):
            g[:, 62 + s * d] = np.maximum(g[:, 62 + s * d], np.float32(v))
            g[101 + s * d, :] = np.maximum(g[101 + s * d, :], np.float32(v))
    return g


def test_box_extent(ctxs):
    """A 96 x 80 grid, all background but one cell, and a three-beam scan
    whose first beam lies on the sensor (its box is the window itself at every
    angle, corner (34, 29)): the odd cell one cell before the box, on its
    first and last cells and one cell past it, in x and in y. A map that took
    the box one cell short or long on any side would drop a beam that reads
    the odd cell, or fail to drop one that the oracle check below shows
    uniform."""
    pts = np.array([[0.0, 0.0], [7.3, -2.2], [-11.6, 9.1]])
    cen = np.array([40.3, 35.3, 0.4])
    one = pts[:1]
    # (three beams take the run-free form; 150 more on the sensor, runs of up
    # to 64 beams with the window's corner, take the run-list form)
    many = np.concatenate([pts, np.zeros((150, 2))])
    lv1 = _level(1)
    flat_bg = None
    for dx in (-1, 0, 12, 13):
        for dy in (-1, 0, 12, 13):
            g = np.full((80, 96), BG, dtype=np.float32)
            g[29 + dy, 34 + dx] = np.float32(1.0)
            m = _set(ctxs, g)
            # the geometry this test assumes, from the oracle: the first beam
            # alone reads the odd cell exactly when it lies inside the box
            sc1 = O.score_window(m, one, lv1, cen, NA * NS * NS)
            if flat_bg is None:
                flat_bg = O.score_window(O.Map(np.full((80, 96), BG, dtype=np.float32), RES, (0.0, 0.0)), one, lv1,
                                         cen, NA * NS * NS)
            inside = dx in (0, 12) and dy in (0, 12)
            assert np.array_equal(sc1, flat_bg) != inside, (dx, dy)
            _check(ctxs, m, pts, [cen])
            # a box taken one cell short or long on a side changes this count
            assert _set_bits(ctxs[0]) == _corners_set(96, 80, 13)
            assert _set_bits(ctxs[0], "grid:bg_map5") == _corners_set(96, 80, 5)
            _check(ctxs, m, one, [cen])
            _check(ctxs, m, many, [cen])


def _fine(n_points):
    from roborts_csm.params import SIM_YAML_LEVELS
    return SIM_YAML_LEVELS[1].with_(use_point_size=int(n_points))  # 11 angles of 11 x 11 steps of 0.4 cells


def _check_fine(ctxs, m, pts, centers):
    lv = _fine(pts.shape[0])
    for cen in centers:
        want = O.score_window(m, pts, lv, cen, 11 * 11 * 11)
        s, flat = O.best_window(m, pts, lv, cen)
        for c in ctxs:
            assert np.array_equal(c.score_window(pts, lv, cen), want), cen
            got = c.best_window(pts, lv, cen)
            assert got.score == s and got.flat_index == flat, cen
    st = _stats(ctxs[0])
    assert "score_phase_kernel<11,all>" in st and "score_phase_kernel<11,best>" in st, st.keys()


def test_box_extent_fine(ctxs):
    """The same for the fine level's 5 x 5 box (corner (38, 33) for a beam on
    the sensor): the odd cell at offsets -1, 0, 4 and 5 in x and in y; three
    beams take the phase kernel's short form, 153 its full one."""
    pts = np.array([[0.0, 0.0], [7.3, -2.2], [-11.6, 9.1]])
    cen = np.array([40.33, 35.37, 0.1])
    one = pts[:1]
    many = np.concatenate([pts, np.zeros((150, 2))])
    lv1 = _fine(1)
    flat_bg = O.score_window(O.Map(np.full((80, 96), BG, dtype=np.float32), RES, (0.0, 0.0)), one, lv1, cen,
                             11 * 11 * 11)
    for dx in (-1, 0, 4, 5):
        for dy in (-1, 0, 4, 5):
            g = np.full((80, 96), BG, dtype=np.float32)
            g[33 + dy, 38 + dx] = np.float32(1.0)
            m = _set(ctxs, g)
            inside = dx in (0, 4) and dy in (0, 4)
            assert np.array_equal(O.score_window(m, one, lv1, cen, 11 * 11 * 11), flat_bg) != inside, (dx, dy)
            _check_fine(ctxs, m, pts, [cen])
            assert _set_bits(ctxs[0], "grid:bg_map5") == _corners_set(96, 80, 5)
            _set_bits(ctxs[0])
            _check_fine(ctxs, m, one, [cen])
            _check_fine(ctxs, m, many, [cen])


def test_mixed_boxes_fine(ctxs):
    """The fine level over the two wall bands and at the grid's edges: 5 x 5
    boxes partly and wholly uniform, 700 beams (two segments of the phase
    kernel) and 70 (its short form)."""
    rng = np.random.default_rng(55)
    m = _set(ctxs, _banded())
    cens = [np.array(c) for c in ([25.2, 25.4, 0.3], [62.3, 40.1, 0.0], [75.1, 101.3, -2.0], [2.2, 3.1, 0.2],
                                  [-3.4, 40.2, 1.0], [125.3, 124.1, 0.4], [131.2, 60.4, 2.2])]
    for n in (700, 70):
        pts = np.ascontiguousarray(rng.uniform(-10.0, 10.0, size=(n, 2)))
        _check_fine(ctxs, m, pts, cens)
    _set_bits(ctxs[0])
    assert _set_bits(ctxs[0], "grid:bg_map5") > 0


@pytest.mark.parametrize("n_beams", [70, 200, 700])
def test_mixed_boxes(ctxs, n_beams):
    """Two wall bands on a 128 x 128 grid, beams within 10 cells of the
    sensor: windows astride a band (boxes partly uniform, runs kept between
    dropped ones), beside one, and one far from both whose every box is
    uniform (every run dropped: no list at all). 70 beams take the run-free
    form, 700 cross the run list's segment of 576."""
    rng = np.random.default_rng(n_beams)
    pts = np.ascontiguousarray(rng.uniform(-10.0, 10.0, size=(n_beams, 2)))
    pts[: n_beams // 4] = np.round(pts[: n_beams // 4])  # shared corners: runs longer than one beam
    m = _set(ctxs, _banded())
    cens = [np.array(c) for c in ([25.2, 25.4, 0.3],  # every box uniform
                                  [62.3, 40.1, 0.0], [50.7, 30.2, 1.1], [75.1, 101.3, -2.0], [30.4, 88.8, 2.9],
                                  [62.0, 101.0, 0.5], [100.6, 60.6, -0.7], [45.5, 112.5, 1.9])]
    _check(ctxs, m, pts, cens)
    assert _set_bits(ctxs[0]) > 0


def test_window_placement(ctxs):
    """Windows at the grid's low edges (box corners inside the strips' low
    padding: cells before column -1 and row -1 hold the outside value, not
    the background) and at its high edges (boxes that run past the grid)."""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(rng.uniform(-9.0, 9.0, size=(300, 2)))
    pts[:60] = np.round(pts[:60] * 2.0) / 2.0
    m = _set(ctxs, _banded())
    cens = [np.array(c) for c in ([2.2, 3.1, 0.2], [-3.4, 40.2, 1.0], [40.3, -2.6, -1.2], [6.0, 6.0, 0.0],
                                  [125.3, 124.1, 0.4], [131.2, 60.4, 2.2], [60.3, 133.9, -0.5], [127.0, 127.0, 3.0])]
    _check(ctxs, m, pts, cens)


def test_background_is_outside_value(ctxs):
    """The real maps' case: the background is the outside value (0 in the
    fixed-point grid, the constant added is 0), and boxes in the low padding
    and past the high edges are uniform too."""
    rng = np.random.default_rng(4)
    pts = np.ascontiguousarray(rng.uniform(-10.0, 10.0, size=(400, 2)))
    g = _banded()
    g[g == BG] = np.float32(0.3)
    m = _set(ctxs, g)
    cens = [np.array(c) for c in ([25.2, 25.4, 0.3], [62.3, 40.1, 0.0], [-4.2, -3.3, 0.7], [130.1, 128.8, 1.4],
                                  [75.1, 101.3, -2.0])]
    _check(ctxs, m, pts, cens)
    assert _set_bits(ctxs[0]) > 0


def test_no_dominant_value(ctxs):
    """Eight values at random, none the outside value: no 13 x 13 box is
    uniform, and the boxes off the grid hold an index no cell has. The map
    has no set bit, the kernel runs without it, and the scores are equal."""
    rng = np.random.default_rng(8)
    vals = (0.3125 + 2.0 ** -4 * np.arange(8)).astype(np.float32)
    g = rng.choice(vals, size=(128, 128)).astype(np.float32)
    pts = np.ascontiguousarray(rng.uniform(-10.0, 10.0, size=(300, 2)))
    m = _set(ctxs, g)
    _set_bits(ctxs[0])
    _check(ctxs, m, pts, [np.array(c) for c in ([25.2, 25.4, 0.3], [2.0, 3.0, 1.0], [126.0, 125.0, -1.0])])
    assert _stats(ctxs[0])["grid:bg_map"]["launches"] >= 1 and _set_bits(ctxs[0]) == 0


def test_stack_two_backgrounds():
    """best_windows over a stack of two grids with different backgrounds
    (0.5 and 0.75, one palette for the stack): each window adds its own
    grid's value for the beams it drops."""
    rng = np.random.default_rng(12)
    a = _banded()
    b = np.where(a == BG, np.float32(0.75), np.float32(0.5)).astype(np.float32)
    b[:, 20:23] = np.float32(1.0)
    stack = np.stack([a, b])
    pts = np.ascontiguousarray(rng.uniform(-10.0, 10.0, size=(500, 2)))
    lv = _level(pts.shape[0])
    cen = np.array([[25.2, 25.4, 0.3], [25.2, 25.4, 0.3], [62.3, 40.1, 0.0], [62.3, 40.1, 0.0], [21.4, 90.2, 1.0],
                    [3.1, 2.2, -1.0], [100.6, 60.6, -0.7]])
    gi = np.array([0, 1, 0, 1, 1, 1, 0], dtype=np.int32)
    want = [O.best_window(O.Map(stack[gi[i]], RES, (0.0, 0.0)), pts, lv, cen[i]) for i in range(len(gi))]
    for env in ({}, {"CSM_BG_RUNS": "0"}):
        c = _ctx(**env)
        try:
            c.set_grid_stack(stack, RES, version=1)
            sc, flat, _, _, _ = c.best_windows(pts, lv, gi, cen)
            for i, (s, fl) in enumerate(want):
                assert sc[i] == s and flat[i] == fl, (env, i)
            st = _stats(c)
            assert "score_box_pair_kernel<13,best>" in st, st.keys()
            assert ("grid:bg_map" in st) == (not env)
            if not env:
                assert st["grid:bg_map"]["scorings"] > 0
        finally:
            c.close()


def test_full_match(ctxs):
    """One 3-level batch match of 64 ray-cast scans on a 256 x 256 world whose
    unknown cells hold 0.5 (the outside value stays 0.3) against the oracle."""
    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.params import headline_levels
    w = worlds.make_world(256, 256, RES, seed=31)
    b = worlds.make_scan_batch(w, 64, seed=32)
    g = np.array(w.grid, dtype=np.float32)
    g[g == np.float32(0.3)] = BG
    lv = headline_levels()
    eye = np.tile(np.eye(3).reshape(1, 9), (64, 1))
    s2, p2, c2 = O.scan_matchers_batch(O.Map(g, w.resolution, w.offset), b.points_cells, b.offsets, lv, b.init_poses,
                                       eye)
    for c in ctxs:
        c.set_grid(roborts_csm.ScanMatchMap(g, float(w.resolution), tuple(w.offset), 0, 1), force=True)
        poses, covs = np.ascontiguousarray(b.init_poses.copy()), eye.copy()
        s = c.scan_matchers_batch(b.points_cells, b.offsets, lv, poses, covs)
        assert np.array_equal(s, s2) and np.array_equal(poses, p2) and np.array_equal(covs, c2)
    assert _set_bits(ctxs[0]) > 0
    assert any(k.startswith("score_box_pair_kernel<13") for k in _stats(ctxs[0]))
