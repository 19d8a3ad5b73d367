"""GPU: scoring, the grid's copies and the search at grid sizes where the
layouts' arithmetic is tight (tests/grid_shapes.py): widths 1 and 3 modulo 4
(gridi_pitch leaves no spare zero column at 1 modulo 4), every strip and tile
residue the suite did not run, grids lower or narrower than a 13 x 13 box, one
strip wide, one row, one column and one cell. Every comparison is bit for bit
against the CPU oracle; tests/test_grid_geom.py proves on the CPU that no read
pattern leaves a buffer at these sizes.

Grids per shape: `ring4` (four values, the two highest alone on the outermost
two rows and columns, so a read that wraps to the next row or runs past the
last finds a non-zero cell where the pad's zero belongs) and `sparse` (one fill
value over about 85 % of the cells inside the ring, the rest in a band and
three odd cells: the maps of uniform boxes reach kBgMinShare and are read);
`values40` at (29, 33): more values than the pair kernel's palettes hold.
The fill is chosen on the CPU from the shape (grid_shapes.sparse): at (40, 49)
a value above the outside value reaches the share (90 % fill, the rest in one
band), so the constant a dropped beam adds is not zero there; at the smaller
shapes no such fill can (too few boxes fit inside the ring) and the fill is
the outside value, which the cells off the grid hold too. Where
the ring is the whole grid (a side of at most 4 cells) there is no fill: the
background is a ring value, no box is uniform, and the maps are built and not
read, which the set-bit counts say.

Scans: 96 points (88 uniform in +-1.5 max(size) cells, 8 on rounding
boundaries and far off each side), and one of 600 points at (29, 33): over
kTailMaxBeams, the pair kernel's run-list form and the phase kernel's long
segments. Windows: the three sim levels over the whole scan at the grid's
middle, the high corner and the low corner.

Which kernel scores each (family, shape, level) follows from the rules in
csm_launch.cpp Launch::decide and csm_level_decision.hpp (level_decide,
launch_shape), restated in `_expected_kernel`; kernel_stats() must name it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

import grid_shapes as S  # noqa: E402
from search_helpers import check_same  # noqa: E402
from test_gpu_palette import _ctx, _stats  # noqa: E402
from test_gpu_score_sink import FAMILIES, _context  # noqa: E402

SHAPE_FAMILIES = ("default", "v8", "v8_gridi", "v4", "v2")
N_SCAN, N_LONG = 96, 600
TIGHT = (29, 33)


def _levels(n_points):
    from roborts_csm.params import SIM_YAML_LEVELS
    return [lv.with_(use_point_size=int(n_points)) for lv in SIM_YAML_LEVELS]


# the sim levels on a 0.05 m map (csm_window_dims): angles, steps per axis, step in cells
DIMS = [(30, 13, 1.0), (11, 11, 0.4), (21, 3, 0.2)]


def _map(g, version=1):
    import roborts_csm
    return roborts_csm.ScanMatchMap(g, S.RES, (0.0, 0.0), 0, version)


def _oracle(g, pts):
    """Per level and centre: (scores, (best score, flat index)), read only."""
    m = O.Map(g, S.RES, (0.0, 0.0))
    out = []
    for lv, (na, ns, _) in zip(_levels(len(pts)), DIMS):
        row = []
        for cen in S.centres(g.shape):
            want = O.score_window(m, pts, lv, cen, na * ns * ns)
            want.setflags(write=False)
            row.append((want, O.best_window(m, pts, lv, cen)))
        out.append(row)
    return out


class Case:
    def __init__(self, shape, kind, grid, pts, bg=None):
        self.shape, self.kind, self.grid, self.pts = shape, kind, grid, pts
        self.grid.setflags(write=False)
        self.bg = bg  # sparse: (set bits of the 13 x 13 map, of the 5 x 5 map, bits per map, both read)
        self.want = _oracle(grid, pts)

    def __repr__(self):
        return f"{self.kind}{self.shape}x{len(self.pts)}"


@pytest.fixture(scope="module")
def cases():
    import roborts_csm
    assert [roborts_csm.window_dims(lv)for lv in _levels(N_SCAN)] == [(na, ns) for na, ns, _ in DIMS]
    out = []
    for k, shape in enumerate(S.SHAPES):
        pts = S.scan(shape, N_SCAN, 500 + k)
        out.append(Case(shape, "ring4", S.ring4(shape, 300 + k), pts))
        g, fill, read = S.sparse(shape, 400 + k)
        (s13, bits), (s5, _) = S.uniform_corners(g, 13), S.uniform_corners(g, 5)
        # read wherever the grid has cells inside the ring at all; a background above the outside value
        # (a non-zero constant per dropped beam) where the shape admits one
        assert read == (min(shape) > 4), (shape, fill, s13 / bits, s5 / bits)
        assert (fill == S.VALS[1]) == (shape == (40, 49)) and fill in S.VALS[:2], (shape, fill)
        out.append(Case(shape, "sparse", g, pts, bg=(s13, s5, bits, read)))
        if shape == TIGHT:
            out.append(Case(shape, "values40", S.values40(shape, 77), pts))
            long = S.scan(shape, N_LONG, 78)
            out.append(Case(shape, "ring4", out[-3].grid.copy(), long))
            out.append(Case(shape, "sparse", g.copy(), long, bg=(s13, s5, bits, read)))
    assert {c.shape for c in out} == set(S.SHAPES)
    return out


def _expected_kernel(family, case, level):
    """The stats name's head for one level, from the decision rules.

    Launch::decide: every grid here has gridi_pitch's pitch, so pad_ok holds;
    the values are exactly summable and the windows a few hundred cells from
    the origin, so use_int holds (LevelCaps::int_grid, LevelSummary::in_range);
    96 or 600 points fit the box offsets (points_ok). Then, by CSM_KERNEL
    (csm_api.cpp):
      v8 and unset: box for a one-cell step of 9..16 steps (level 0), phase
        for the 0.4-cell step of 11 (level 1), tiny for a span under one cell
        (level 2), whatever the grid's size: none of the three rules reads it.
        Unset, the box is the pair kernel where the palette has at most 16
        values (ring4: 4, sparse: 4 or fewer) and the v6 box kernel otherwise
        (values40); under v8 always the v6 box kernel.
      v4: row segments, rows_pick_sq(n_space, floor(span) + 2): 13 steps of 1
        cell need 14 cells, Q = 4; 11 of 0.4 need 6, Q = 2; 3 of 0.2 need 2,
        Q = 1. `if (size_x < 4 * rows_sq) rows_sq = 0`: a grid narrower than
        the segment (16, 8 and 4 cells) falls to the column kernel.
      v2: the column kernel.
    The column kernel's name is `score_cols_kernel<kt,int,mode>`: kt, its rows
    per lane, equals n_space while the window is one 16-wide tile across
    (launch_shape: ktiles = 1 up to 16 steps), and `int` is the fixed-point sum."""
    na, ns, f = DIMS[level]
    sx = case.shape[1]
    cols = f"score_cols_kernel<{ns},int,"
    if family == "v2":
        return cols
    if family == "v4":
        q = (4, 2, 1)[level]
        return f"score_rowsd_kernel<{ns},{q}," if sx >= 4 * q else cols
    assert family in ("default", "v8", "v8_gridi")
    if level == 0:
        pair = family == "default" and case.kind != "values40"
        return f"score_box_pair_kernel<{ns}," if pair else f"score_box_kernel<{ns},"
    return f"score_phase_kernel<{ns}," if level == 1 else f"score_tiny_kernel<{ns},"


def _launches(c):
    return {k["name"]: k["launches"] for k in c.kernel_stats() if k["name"].startswith("score_")}


def _score_case(c, case, what):
    """Every level and centre of a case against the oracle; returns, per level,
    the scoring kernels that ran."""
    ran = []
    for level, lv in enumerate(_levels(len(case.pts))):
        before = _launches(c)
        for cen, (want, (bs, bflat)) in zip(S.centres(case.shape), case.want[level]):
            sc = c.score_window(case.pts, lv, cen)
            assert np.array_equal(sc, want), (what, case, level, cen, np.flatnonzero(sc != want)[:8])
            got = c.best_window(case.pts, lv, cen)
            assert (got.score, got.flat_index) == (bs, bflat), (what, case, level, cen)
        after = _launches(c)
        ran.append({n for n, k in after.items() if k > before.get(n, 0)})
    return ran


@pytest.mark.parametrize("family", SHAPE_FAMILIES)
def test_scores_and_best(cases, family):
    env, _ = FAMILIES[family]
    c = _context(env)
    try:
        c.set_profiling(True)
        for case in cases:
            seen = {k: _stats(c).get(k, {"scorings": 0})["scorings"] for k in ("grid:bg_map", "grid:bg_map5")}
            c.set_grid(_map(case.grid), force=True)
            ran = _score_case(c, case, family)
            for level, names in enumerate(ran):
                head = _expected_kernel(family, case, level)
                assert names == {head + "all>", head + "best>"}, (family, case, level, sorted(names), head)
            if family == "default" and case.kind == "sparse":
                # the maps of uniform boxes were built with the restated number of set corners, which is
                # over kBgMinShare (bg_map_used): the pair kernel and the phase strips read them
                s13, s5, bits, read = case.bg
                st = _stats(c)
                assert st["grid:bg_map"]["scorings"] - seen["grid:bg_map"] == s13, case
                assert st["grid:bg_map5"]["scorings"] - seen["grid:bg_map5"] == s5, case
                assert (min(s13, s5) / bits >= S.BG_MIN_SHARE) == read, case
    finally:
        c.close()


def _stack(shape):
    return np.ascontiguousarray(np.stack([S.ring4(shape, 300 + S.SHAPES.index(shape)), S.ring4(shape, 901),
                                          S.ring4(shape, 902)]))


@pytest.mark.parametrize("shape", [TIGHT, (5, 3)])
def test_grid_stack(shape):
    """Three grids back to back: a grid's pad rows are followed by the next
    grid's row 0, and nothing follows the last grid's. Windows on grids
    2, 0, 1, 1 in one call."""
    grids = _stack(shape)
    pts = S.scan(shape, N_SCAN, 500 + S.SHAPES.index(shape))
    cen = S.centres(shape)
    gi, centres = [2, 0, 1, 1], np.stack([cen[0], cen[1], cen[2], cen[1]])
    maps = [O.Map(g, S.RES, (0.0, 0.0)) for g in grids]
    want = [[O.best_window(maps[g], pts, lv, c) for g, c in zip(gi, centres)] for lv in _levels(N_SCAN)]
    for family in ("default", "v8"):
        c = _context(FAMILIES[family][0])
        try:
            c.set_grid_stack(grids, S.RES, version=1)
            for level, lv in enumerate(_levels(N_SCAN)):
                sc, flat, _, _, _ = c.best_windows(pts, lv, gi, centres)
                assert [(s, int(f)) for s, f in zip(sc, flat)] == [(s, int(f)) for s, f in want[level]], \
                    (family, shape, level)
        finally:
            c.close()


COUNTED = ("grid:analyze", "grid:palette", "grid:bg_map", "grid:istrips")


def _counts(c):
    st = _stats(c)
    return tuple(st[k]["launches"] if k in st else 0 for k in COUNTED)


@pytest.mark.parametrize("shape", [TIGHT, (31, 47)])
def test_refresh_at_the_pitch_edge(shape):
    """Row and cell refreshes of a resident grid whose pitch exceeds its width
    by the minimum: the last row alone (the pad rows follow it), rows 0..2, and
    the cells either side of the pitch gap, (sx - 1, 0) and (0, 1), with the
    first and last cell. New values are the grid's own (the fixed-point copy
    holds them exactly). After each step every score equals the oracle on the
    updated array and a fresh context that uploaded it whole; the palette
    family and the strips of gridi are rebuilt once per step, as
    test_gpu_grid_copies.py counts them (coarse level first: it builds the
    palette and its maps, the fine level the strips, nothing analyses again)."""
    sy, sx = shape
    pts = S.scan(shape, N_SCAN, 500 + S.SHAPES.index(shape))
    g = S.ring4(shape, 300 + S.SHAPES.index(shape)).copy()
    a = _map(g, version=1)

    def check(c, step, counts):
        case = Case(shape, f"ring4-step{step}", g.copy(), pts)
        _score_case(c, case, "resident")
        assert _counts(c) == counts, (shape, step, _counts(c))
        fresh = _ctx()
        try:
            fresh.set_grid(_map(case.grid))
            _score_case(fresh, case, "fresh")
        finally:
            fresh.close()

    c = _ctx()
    try:
        c.set_grid(a)
        check(c, 0, (1, 1, 1, 1))
        g[sy - 1, :] = S.VALS[1]  # the last row alone (the ring held 0.88 and 1.0 there)
        a.version = 2
        c.update_grid_rows(a, sy - 1, sy)
        check(c, 1, (1, 2, 2, 2))
        g[0:3, :] = np.tile(S.VALS[[1, 3, 0]], sx // 3 + 1)[:sx]
        a.version = 3
        c.update_grid_rows(a, 0, 3)
        check(c, 2, (1, 3, 3, 3))
        idx = np.array([0, sx * sy - 1, sx - 1, sx], dtype=np.int32)  # (0,0), the last, (sx-1,0), (0,1)
        new = S.VALS[[2, 3, 2, 3]]
        # every one of the four changes (they hold 0.41, 0.41, 0.3 or 1.0, and 0.41 after the row steps):
        # a write that is dropped or lands in another cell shows in the scores
        assert np.all(g.ravel()[idx] != new), (g.ravel()[idx], new)
        g.ravel()[idx] = new
        assert g[0, 0] == new[0] and g[sy - 1, sx - 1] == new[1] and g[0, sx - 1] == new[2] and g[1, 0] == new[3]
        a.version = 4
        c.update_grid_cells(a, idx)
        check(c, 3, (1, 4, 4, 4))
        st = _stats(c)
        assert st["grid:upload"]["launches"] == 1 and st["grid:rows"]["launches"] == 2
        assert st["grid:cells"]["launches"] == 1
    finally:
        c.close()


@pytest.mark.parametrize("shape", [TIGHT, (31, 47), (12, 13), (1, 1)])
def test_search_equals_exhaustive(shape):
    """A loop-closure-like window wider than the grid (4 cells more than its
    longer side, at least 17: more than 16 steps per axis), at every depth from
    0 to the one whose single node covers the window: the search's answer is
    the exhaustive device argmax and the oracle's."""
    import roborts_csm
    from roborts_csm.params import CorrelationScanMatchParam
    k = S.SHAPES.index(shape)
    g = S.ring4(shape, 300 + k)
    pts = S.scan(shape, N_SCAN, 500 + k)
    cells = max(max(shape) + 4, 17)
    p = CorrelationScanMatchParam(cells * S.RES, S.RES, 0.2, 0.0349, 0.5, N_SCAN, 0, True, 0)
    na, ns = roborts_csm.window_dims(p)
    assert ns > 16 and ns > max(shape), (ns, shape)
    deepest = int(np.ceil(np.log2(ns)))
    m = O.Map(g, S.RES, (0.0, 0.0))
    with roborts_csm.Context(0) as c:
        c.set_grid_stack(g[None], S.RES, version=1)
        for cen in S.centres(shape):
            want = O.best_window(m, pts, p, cen)
            for depth in range(deepest + 1):
                b, w, st = check_same(c, pts, p, [0], cen[None], max_depth=depth)
                assert (b.score, b.flat_index) == want and w == 0, (shape, cen, depth, st)
                assert st["depth"] == depth and not st["exhaustive"], (shape, depth, st)


def test_map_mirror_at_odd_size():
    """A 45 x 33 device map with blur, two short scans drawn into it without
    growth: csm_set_grid_gridmap hands the map's fixed-point mirror (fpm_pitch,
    at this width the tight pitch) to the matcher, and the three levels score
    the downloaded cells exactly."""
    import roborts_csm
    from roborts_csm.gridmap import OccuGridMap, set_matcher_grid
    sx, sy = 45, 33
    pose = np.array([1.0, 1.0, 0.3])
    off = (-(pose[0] - 0.5 * sx * S.RES), -(pose[1] - 0.5 * sy * S.RES))
    th = np.linspace(-np.pi, np.pi, 24, endpoint=False)
    scans = [np.stack([9.0 * np.cos(th), 6.0 * np.sin(th)], axis=1),
             np.stack([5.0 + 3.0 * np.cos(th[:12]), -2.0 + 4.0 * np.sin(th[:12])], axis=1)]
    pts = S.scan((sy, sx), N_SCAN, 61)
    with roborts_csm.Context(0) as ctx:
        m = OccuGridMap(S.RES, (sx, sy), off, 0.15, 0.3)
        m.set_options(True, True, 0.88, 0.2)
        for s in scans:
            m.UpdateMapByRange(s, pose, use_blur=True)
        assert (m.GetSizeX(), m.GetSizeY()) == (sx, sy)  # no growth: the odd size is what is scored
        ctx.set_profiling(True)
        set_matcher_grid(ctx, m)
        st = m.state()
        prob = m.cells()[0]
        assert prob.shape == (sy, sx) and np.unique(prob).size > 2
        om = O.Map(prob, st.resolution, (st.offset_x, st.offset_y), st.map_update_index)
        for lv, (na, ns, _) in zip(_levels(N_SCAN), DIMS):
            for cen in S.centres((sy, sx)):
                got = ctx.score_window(pts, lv, cen)
                assert np.array_equal(got, O.score_window(om, pts, lv, cen, na * ns * ns)), (lv, cen)
        names = {s["name"] for s in ctx.kernel_stats()}
        assert "grid:mirror" in names and "grid:analyze" not in names, names
