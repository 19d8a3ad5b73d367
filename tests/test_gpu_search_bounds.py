"""The admissible search's bounds themselves (csm_search_bounds, a test hook
over csrc/csm_pyramid.hip), pinned to a plain integer restatement
(tests/search_pyref.py, itself checked against the oracle on the CPU).

tests/test_gpu_search.py compares final answers only, on inputs whose bounds
sit far above every real score, so a pool one cell short, a tap dropped at an
edge, a rounded (not ceiled) quantisation, a 0.5 penalty floor or a threshold
off by one would all pass there. Here

  * the three kernels that compute the top level's bounds (beam boxes, whole-
    level gathers, node-list gathers) return exactly the restated values;
  * every device bound is >= the device's exact score of every candidate
    under the node;
  * the pooled levels are read out cell by cell;
  * end-to-end searches on three-valued grids (background, decoy, needle)
    have no slack: a bound one unit too low loses the needle.

Every assertion is exact equality or >= on integers and doubles.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402
import pyref  # noqa: E402
import search_pyref as R  # noqa: E402
from search_helpers import check_same  # noqa: E402

RES = 0.05
MRES = 1.0 / (1.0 / RES)
W, H = 93, 77
U = 2.0 ** -20  # one fixed-point unit of the E = 20 grids


def _param(ns, half_angle, penalty, use=100):
    from roborts_csm.params import CorrelationScanMatchParam
    p = CorrelationScanMatchParam((ns - 1) * RES, RES, half_angle, 0.0349, 0.5, use, 0, penalty, 0)
    assert pyref.dims(p)[1] == ns
    return p


def _center(origin, ns, frac=0.25):
    """Window centre whose candidate j sits at origin + j + frac cells."""
    half = ((ns - 1) * RES / MRES) * 0.5
    return (origin + frac) + half


@pytest.fixture(scope="module")
def stack():
    g = R.scene(W, H)
    assert R.fixed_point(g, 0.0)[1] == 20 and R.fixed_point(g, 0.75)[1] == 20
    return g


@pytest.fixture(scope="module")
def ctxs(stack):
    """One context per (outside value, shift), the scene minus shift resident."""
    import roborts_csm
    made, kept = {}, []

    def get(outside, shift=0.0):
        if (outside, shift) not in made:
            c = roborts_csm.Context(0)
            c.set_outside_value(outside)
            kept.append(stack - np.float32(shift))
            c.set_grid_stack(kept[-1], RES, version=1)
            made[(outside, shift)] = c
        return made[(outside, shift)]

    yield get
    for c in made.values():
        c.close()


def _scan(n, seed=3):
    """n points: a few on integer and half-integer cells (with the angle-0 row
    they put t on an integer: the box kernel's rejected path), the rest random."""
    rng = np.random.default_rng(seed)
    planted = np.array([[0.0, 0.0], [2.5, -1.5], [3.0, -2.0], [-7.5, 5.0], [4.0, 1.5], [-6.0, -3.0]])
    pts = np.concatenate([planted, rng.uniform(-25.0, 25.0, (max(n, 6), 2))])[:n]
    return np.ascontiguousarray(pts)


def _windows(ns, half):
    """Centres (x, y, angle): inside the grid with fractional parts 0, 0.5 and
    0.5 - 2^-21, off each edge, off a corner, wholly off the grid. The common
    angle puts the first angle row at exactly 0; the last window has its own."""
    h = (ns - 1) / 2.0
    far = ns + 80.0
    cx, cy = max(46.0, np.ceil(h) + 2.0), max(38.0, np.ceil(h) + 1.0)  # the first three: t >= 0 for a beam at 0
    c = [[cx, cy], [cx + 0.5, cy + 0.5], [cx + 0.5 - 2.0 ** -21, cy + 0.5 - 2.0 ** -21],
         [-h / 2 - 3.25, 30.0], [W + h / 2 + 1.75, 41.5], [50.5, -h / 2 - 2.0], [40.0, H + h / 2 + 0.5],
         [-3.0, -2.5], [W + far, H + far], [30.25, 50.75]]
    out = np.array([[x, y, half] for x, y in c])
    out[-1, 2] = 0.3
    return out


def _restated(stack, outside, pts, p, gi, centers, d):
    """(sums, bounds) of every top node, list order."""
    return R.top_bounds(stack, outside, pts, p, gi, centers, MRES, d)


def _beams_for(n_used):
    """(n_points, use_point_size) giving n_used beams; 9 and 64 by subsampling."""
    if n_used == 9:
        return 27, 9      # step 3
    if n_used == 64:
        return 128, 64    # step 2
    return n_used, max(100, n_used)


NJ = [1, 4, 9, 16, 21, 32]
N_USED = [1, 2, 3, 7, 8, 9, 63, 64, 65, 200]
CASES = []
for _i, (_d, _nj) in enumerate((d, nj) for d in (1, 2, 3, 4, 5) for nj in NJ):
    CASES.append((_d, _nj, N_USED[(_i * 3) % 10], bool(_i % 2), 0.75 if (_i // 2) % 2 else 0.0))
# every beam count at the deepest and the shallowest level too
CASES += [(1, 4, n, bool(k % 2), 0.75 if k % 3 else 0.0) for k, n in enumerate(N_USED)]
CASES += [(5, 9, n, bool((k + 1) % 2), 0.0 if k % 3 else 0.75) for k, n in enumerate(N_USED)]
assert {c[2] for c in CASES} == set(N_USED) and {c[1] for c in CASES} == set(NJ)


@pytest.mark.parametrize("d,nj,n_used,penalty,outside", CASES)
def test_three_kernels_equal_restatement(stack, ctxs, d, nj, n_used, penalty, outside):
    """The box sums (kernel 0) and the bounds of both gather kernels (1, 2)
    equal the restatement, node by node, bit for bit. Ten windows (inside,
    off every edge, off a corner, wholly off, fractional centres) on the three
    grids; nj picks the box kernel's instantiation, the beam count the lanes
    per node (2 lpn <= n_used), the 8-way loop's tail, the 64-beam chunks and
    (from 64 beams on, 40 waves) the split box launch."""
    n, use = _beams_for(n_used)
    ns = (nj - 1) * (1 << d) + (1 if nj % 2 else min(3, 1 << d))
    p = _param(ns, 0.06, penalty, use)
    pts = _scan(n)
    centers = _windows(ns, 0.06)
    gi = np.arange(centers.shape[0]) % 3
    win = [R.Window(pts, p, c, MRES, d) for c in centers]
    assert win[0].nj == nj and win[0].n_used == n_used and (win[0].step > 1) == (n_used in (9, 64))
    # the box kernel's clean test goes both ways on the fractional centres
    per_window = [np.concatenate([w.clean(a) for a in range(w.na)]) for w in win[:3]]
    clean = np.concatenate(per_window)
    assert (~clean).any() and clean.any()
    if n_used >= 2:  # each fractional part by itself (one beam cannot go both ways in one window)
        assert all((~c).any() and c.any() for c in per_window)
    sums, bounds = _restated(stack, outside, pts, p, gi, centers, d)
    c = ctxs(outside)
    got0 = c.search_bounds(pts, p, gi, centers, d, 0)
    assert got0.dtype == np.int64 and np.array_equal(got0, sums)
    for kernel in (1, 2):
        got = c.search_bounds(pts, p, gi, centers, d, kernel)
        assert np.array_equal(got.view(np.uint64), bounds.view(np.uint64)), kernel


@pytest.mark.parametrize("d,nj,n_used", [(1, 9, 7), (2, 16, 65), (3, 4, 200), (4, 21, 8)])
def test_negative_scores_take_the_0_45_floor(stack, ctxs, d, nj, n_used):
    """The scene shifted down by 1.25 (cells in [-1.25, -0.25], outside -0.25),
    the penalty on: every node's raw bound is negative and carries the factor
    0.45, in all three kernels' values."""
    n, use = _beams_for(n_used)
    ns = (nj - 1) * (1 << d) + 1
    p = _param(ns, 0.06, True, use)
    pts = _scan(n)
    centers = _windows(ns, 0.06)
    gi = np.arange(centers.shape[0]) % 3
    shifted = stack - np.float32(1.25)
    assert R.fixed_point(shifted, -0.25)[1] == 20
    sums, bounds = _restated(shifted, -0.25, pts, p, gi, centers, d)
    plain = R.top_bounds(shifted, -0.25, pts, _param(ns, 0.06, False, use), gi, centers, MRES, d)[1]
    assert (plain < 0).all() and np.unique(plain).size > 10 and np.array_equal(bounds, plain * 0.45)
    c = ctxs(-0.25, 1.25)
    assert np.array_equal(c.search_bounds(pts, p, gi, centers, d, 0), sums)
    for kernel in (1, 2):
        got = c.search_bounds(pts, p, gi, centers, d, kernel)
        assert np.array_equal(got.view(np.uint64), bounds.view(np.uint64)), kernel


def test_unsupported_box_width_is_reported(stack, ctxs):
    """nj = 33 has no box instantiation: kernel 0 reports CSM_ERR_UNSUPPORTED
    (no silent fall-back); the gather kernels still equal the restatement. A
    step other than one cell is outside the pooled search for every kernel.
    A search after the hook is unaffected."""
    import roborts_csm
    from roborts_csm import _abi
    d, ns = 1, 65
    p = _param(ns, 0.06, False)
    pts = _scan(9)
    centers = _windows(ns, 0.06)[:4]
    gi = np.arange(4) % 3
    c = ctxs(0.0)
    with pytest.raises(roborts_csm.CsmError) as e:
        c.search_bounds(pts, p, gi, centers, d, 0)
    assert e.value.status == _abi.CSM_ERR_UNSUPPORTED
    _, bounds = _restated(stack, 0.0, pts, p, gi, centers, d)
    for kernel in (1, 2):
        assert np.array_equal(c.search_bounds(pts, p, gi, centers, d, kernel), bounds)
    check_same(c, pts, p, gi, centers, max_depth=3)
    from roborts_csm.params import CorrelationScanMatchParam
    coarse = CorrelationScanMatchParam(1.0, 0.1, 0.06, 0.0349, 0.5, 100, 0, False, 0)
    for kernel in (0, 1, 2):
        with pytest.raises(roborts_csm.CsmError) as e:
            c.search_bounds(pts, coarse, gi, centers, 1, kernel)
        assert e.value.status == _abi.CSM_ERR_UNSUPPORTED


def test_many_windows_run_the_box_kernel_unsplit(stack, ctxs):
    """launch_pyr_topbox splits a (window, angle)'s beams over several waves
    while n_windows * n_angles < 4096 and a wave keeps 32 beams; 64 beams
    split in the cases above (10 windows x 4 angles). Here 1030 windows x 4
    angles = 4120 waves: the same 64 beams unsplit. nj = 4."""
    d, nj, outside = 2, 4, 0.75
    ns = 3 * 4 + 3
    p = _param(ns, 0.06, True, 64)
    assert pyref.dims(p)[0] == 4
    pts = _scan(64)
    rng = np.random.default_rng(8)
    n_win = 1030
    centers = np.column_stack([rng.uniform(-10.0, W + 10.0, n_win), rng.uniform(-10.0, H + 10.0, n_win),
                               np.full(n_win, 0.06)])
    centers[::7, :2] = np.floor(centers[::7, :2]) + 0.5
    gi = np.arange(n_win) % 3
    assert n_win * 4 >= 4096
    sums, bounds = _restated(stack, outside, pts, p, gi, centers, d)
    c = ctxs(outside)
    assert np.array_equal(c.search_bounds(pts, p, gi, centers, d, 0), sums)
    assert np.array_equal(c.search_bounds(pts, p, gi, centers, d, 1).view(np.uint64), bounds.view(np.uint64))


def _block_max(sc, na, ns, d):
    """Best candidate score under every top node, [angle, K, J]."""
    sh = 1 << d
    nj = (ns + sh - 1) >> d
    pad = np.full((na, nj * sh, nj * sh), -np.inf)
    pad[:, :ns, :ns] = sc.reshape(na, ns, ns)                 # (theta, x, y)
    return pad.reshape(na, nj, sh, nj, sh).max(axis=(2, 4)).transpose(0, 2, 1)


@pytest.mark.parametrize("d,ns", [(1, 7), (2, 14), (3, 27), (4, 50), (5, 70)])
@pytest.mark.parametrize("penalty", [False, True])
def test_device_bounds_are_admissible(stack, d, ns, penalty):
    """Every top node's device bound (gathers, and the box sums through the
    restated conversion) >= the device's exact score (score_window, pinned to
    the oracle elsewhere) of every in-window candidate under it."""
    import roborts_csm
    pts = _scan(9)
    p = _param(ns, 0.06, penalty)
    centers = _windows(ns, 0.06)[[0, 1, 2, 3, 4, 7, 9]]
    na = pyref.dims(p)[0]
    for outside in (0.0, 0.75):
        for g in (0, 1):
            _, E, oi = R.fixed_point(stack[g], outside)
            with roborts_csm.Context(0) as c:
                c.set_outside_value(outside)
                c.set_grid_stack(stack[g:g + 1], RES, version=-1)
                gi = np.zeros(centers.shape[0], dtype=np.int32)
                b1 = c.search_bounds(pts, p, gi, centers, d, 1).reshape(centers.shape[0], na, -1)
                s0 = c.search_bounds(pts, p, gi, centers, d, 0)
                b0 = R.bound(s0, 9, oi, E, 9, penalty).reshape(b1.shape)
                for w, ctr in enumerate(centers):
                    best = _block_max(c.score_window(pts, p, ctr), na, ns, d).reshape(na, -1)
                    assert np.all(b1[w] >= best) and np.all(b0[w] >= best), (outside, g, w)


@pytest.mark.parametrize("outside", [0.0, 0.75])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_pooled_levels_cell_by_cell(stack, ctxs, d, outside):
    """One beam at the origin, one angle, t on integers: a top node's bound is
    one cell of level d. 4^d windows per grid, shifted by every offset in
    [0, 2^d)^2, visit every anchor of the level (the negative ones and the
    last row and column included) through pyr_bound_kernel; the assembled
    level equals the brute-force pooled level on all three grids."""
    sh = 1 << d
    nj = (W + 2 * sh - 1) >> d
    ns = (nj - 1) * sh + 1
    p = _param(ns, 0.0, False)
    pts = np.zeros((1, 2))
    half = ((ns - 1) * RES / MRES) * 0.5
    offs = [(ox, oy) for oy in range(sh) for ox in range(sh)]
    centers = np.array([[(-sh + ox - 0.5) + half, (-sh + oy - 0.5) + half, 0.0] for _ in range(3) for ox, oy in offs])
    gi = np.repeat(np.arange(3), len(offs))
    got = ctxs(outside).search_bounds(pts, p, gi, centers, d, 2).reshape(len(gi), nj, nj)  # [w, K, J]
    fixed, E, oi = R.fixed_point(stack, outside)
    dev = np.full((3, H + sh, W + sh), np.nan)
    for w, ctr in enumerate(centers):
        win = R.Window(pts, p, ctr, MRES, d)
        assert win.na == 1 and win.n_used == 1 and win.use == 1
        gx, gy = win.anchor_cells(0)
        gx, gy = gx[0] + sh, gy[0] + sh
        ox, oy = offs[w % len(offs)]
        assert gx[0] == ox and gy[0] == oy and np.all(np.diff(gx) == sh) and np.all(np.diff(gy) == sh)
        okx, oky = gx < W + sh, gy < H + sh
        dev[gi[w]][np.ix_(gy[oky], gx[okx])] = got[w][np.ix_(oky, okx)]
        # anchors past the level read 0
        rest = got[w][~(oky[:, None] & okx[None, :])]
        assert np.all(rest == R.bound(np.zeros(1, np.int64), 1, oi, E, 1, False)[0])
    assert not np.isnan(dev).any()  # every anchor visited
    for g in range(3):
        want = R.bound(R.pooled_level(fixed[g], d), 1, oi, E, 1, False)
        assert np.array_equal(dev[g], want), g


def test_the_extra_tap_matters():
    """A node's last candidate can read column g0 + 2^d ("rounding < 2^-20" in
    csm_pyramid.hip's header). The search below finds such inputs at every
    depth among doubles |t| < 2^10: a beam at x = 0.5 - k 2^-53 under a window
    whose candidates sit on integers. Candidate 0 reads column 0 (t = 1 -
    k 2^-53 truncates to 0), candidate 2^d - 1 reads column 2^d (fl(x + 2^d -
    1) rounds up to 2^d - 0.5). The grid's only high cell is in that column:
    a [g0, g0 + 2^d - 1] pool bounds the node below that candidate's score;
    the device's bounds, all three kernels, do not."""
    import roborts_csm
    found = {}
    for d in (1, 2, 3, 4, 5):
        ns = 1 << d
        p = _param(ns, 0.0, False)
        for k in range(1, 9):
            for x0 in (0.0, 7.0, 100.0, 1000.0):
                bx = 0.5 - k * 2.0 ** -53
                half = ((ns - 1) * RES / MRES) * 0.5
                ctr = np.array([x0 + half, 5.0 + half, 0.0])
                win = R.Window(np.array([[bx, 0.25]]), p, ctr, MRES, d)
                lx, _ = win.rotated(0)
                cols = np.trunc((lx[0] + win.xs) + 0.5).astype(np.int64)
                if win.nj == 1 and abs(lx[0] + win.xs[-1]) < 2.0 ** 10 and cols[-1] == cols[0] + (1 << d):
                    found.setdefault(d, (bx, ctr, int(cols[0]), int(cols[-1])))
    assert sorted(found) == [1, 2, 3, 4, 5]
    with roborts_csm.Context(0) as c:
        c.set_outside_value(0.0)
        for d, (bx, ctr, g0, g1) in found.items():
            ns = 1 << d
            p = _param(ns, 0.0, False)
            pts = np.array([[bx, 0.25]])
            grid = np.zeros((1, 24, 40), dtype=np.float32)
            assert g0 == 0 and g1 == ns
            grid[0, 5, g1] = 1.0
            c.set_grid_stack(grid, RES, version=-1)
            sc = c.score_window(pts, p, ctr).reshape(ns, ns)     # (x, y), one angle
            assert sc[ns - 1, 0] == 1.0 and sc[:ns - 1].max() == 0.0
            fixed, E, oi = R.fixed_point(grid, 0.0)
            win = R.Window(pts, p, ctr, MRES, d)
            short = R.bound(R.node_sums(win, R.pooled_level(fixed[0], d, span=ns - 1)), 1, oi, E, 1, False)
            assert short.shape == (1, 1, 1) and short[0, 0, 0] < 1.0
            for kernel in (1, 2):
                assert c.search_bounds(pts, p, [0], [ctr], d, kernel)[0] >= 1.0
            s0 = c.search_bounds(pts, p, [0], [ctr], d, 0)
            assert R.bound(s0, 1, oi, E, 1, False)[0] >= 1.0


# ---- zero-slack end-to-end searches ---------------------------------------
ONE_BEAM = np.zeros((1, 2))
THREE_BEAMS = np.array([[0.0, 0.0], [20.0, 0.0], [0.0, 6.0]])


def _cells_read(pts, p, ctr, flat):
    """The grid cells candidate `flat` reads, one per beam."""
    win = R.Window(pts, p, ctr, MRES, 1)
    a, r = divmod(int(flat), win.ns * win.ns)
    j, k = divmod(r, win.ns)
    lx, ly = win.rotated(a)
    return [(int(np.trunc((x + win.xs[j]) + 0.5)), int(np.trunc((y + win.ys[k]) + 0.5))) for x, y in zip(lx, ly)]


def _grid3(B, cells, shape=(H, W)):
    g = np.full((1,) + shape, B, dtype=np.float32)
    for (x, y), v in cells.items():
        assert 0 <= x < shape[1] and 0 <= y < shape[0]
        g[0, y, x] = v
    return g


def _first_probed(grid, outside, pts, p, ctr, D):
    """(angle, J, K) of the top node the search probes first: the best restated
    bound, ties to the lowest index. A node's pool reaches the first row and
    column of its higher neighbours, so a decoy only raises the incumbent at
    once if this is the node whose candidates read it."""
    _, b = R.top_bounds(grid, outside, pts, p, [0], [ctr], MRES, D)
    win = R.Window(pts, p, ctr, MRES, D)
    b = b.reshape(win.na, win.nj, win.nj)                      # [a, K, J]
    a, K, J = np.meshgrid(np.arange(win.na), np.arange(win.nj), np.arange(win.nj), indexing="ij")
    low = (a * win.ns + (J << D)) * win.ns + (K << D)
    i = np.argmin(np.where(b == b.max(), low, np.iinfo(np.int64).max))
    return int(a.flat[i]), int(J.flat[i]), int(K.flat[i])


def _search(c, grid, pts, p, ctr, D, top_kernel):
    c.set_grid_stack(grid, RES, version=-1)
    b, _, st = check_same(c, pts, p, [0], np.asarray(ctr).reshape(1, 3), max_depth=D, top_kernel=top_kernel)
    assert not st["exhaustive"] and bool(st["top_box"]) == (top_kernel == 0)
    return b, st


def _placements(D, ns):
    """(needle candidate (j, k), decoy candidate (j, k)): the needle at offsets
    0, 1, 2^D - 1 of top node (1, 1) on both axes, and on the window's last
    row and column; the decoy in a node of lower index."""
    sh = 1 << D
    out = [((sh + ox, sh + oy), (sh - 1, 1)) for ox in (0, 1, sh - 1) for oy in (0, 1, sh - 1)]
    out.append(((ns - 1, ns - 1), (sh, 0)))
    return out


@pytest.mark.parametrize("top_kernel", [0, 1])
@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("beams", ["one", "three"])
def test_needle_is_found_at_every_offset(D, top_kernel, beams):
    """B < D < N: whatever cell of its top node holds the needle, on the
    window's last row and column and one cell inside each grid edge, the
    search returns the candidate that reads it. With the y = 0.5 - 2^-53 beam
    of test_the_extra_tap_matters the needle of node K = 0's last candidate
    sits in row g0 + 2^D, which only the pool's extra tap covers."""
    import roborts_csm
    pts = ONE_BEAM if beams == "one" else THREE_BEAMS
    sh = 1 << D
    ns = 2 * sh + 1
    p = _param(ns, 0.0, False)
    B, Dv, N = 0.25, 0.5, 0.5 + U
    with roborts_csm.Context(0) as c:
        c.set_outside_value(0.0)
        cases = [((4, 3), nd, dc) for nd, dc in _placements(D, ns)]
        # needle one cell inside each grid edge (the window over that edge)
        cases += [((-sh, 5), (sh + 1, 4), (sh, 2)), ((W - 2 - sh - 1, 5), (sh + 1, 4), (sh, 2)),
                  ((5, -sh), (4, sh + 1), (2, sh)), ((5, H - 2 - sh - 1), (4, sh + 1), (2, sh))]
        for origin, nd, dc in cases:
            ctr = [_center(origin[0], ns), _center(origin[1], ns), 0.0]
            n_cell = _cells_read(pts, p, ctr, nd[0] * ns + nd[1])[0]
            d_cell = _cells_read(pts, p, ctr, dc[0] * ns + dc[1])[0]
            assert dc[0] * ns + dc[1] < ((nd[0] >> D) << D) * ns + ((nd[1] >> D) << D) or nd[0] >> D == dc[0] >> D
            b, _ = _search(c, _grid3(B, {d_cell: Dv, n_cell: N}), pts, p, ctr, D, top_kernel)
            assert n_cell in _cells_read(pts, p, ctr, b.flat_index), (origin, nd, dc)
        if beams == "one":
            # the rounding beam: candidate k >= 1 reads row origin + k + 1, node K = 0's pool
            # must reach row origin + 2^D for its last candidate
            rpts = np.array([[0.25, 0.5 - 2.0 ** -53]])
            half = ((ns - 1) * RES / MRES) * 0.5
            ctr = [4.0 + half, 0.0 + half, 0.0]
            nd, dc = (sh + 1, sh - 1), (1, sh + 1)
            n_cell = _cells_read(rpts, p, ctr, nd[0] * ns + nd[1])[0]
            d_cell = _cells_read(rpts, p, ctr, dc[0] * ns + dc[1])[0]
            assert n_cell[1] == sh and _cells_read(rpts, p, ctr, nd[0] * ns)[0][1] == 0
            b, _ = _search(c, _grid3(B, {d_cell: Dv, n_cell: N}), rpts, p, ctr, D, top_kernel)
            assert b.flat_index == nd[0] * ns + nd[1]


@pytest.mark.parametrize("top_kernel", [0, 1])
@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("outside", [0.0, 0.75])
@pytest.mark.parametrize("beams", ["one", "three"])
def test_quantisation_takes_the_ceiling(D, top_kernel, outside, beams):
    """B = 0.25, D = 0.5 (a whole number of level units), N = 0.5 + 2^-20. The
    decoy's node comes first, so the incumbent is D when the needle's node is
    looked at: with a floor or a round-to-nearest that node's bound would tie
    it at a higher index and be pruned. The ceiling keeps it. The mirror: N =
    D exactly, the tie goes to the decoy's lower index. With outside = 0.75
    all three are negative in fixed point."""
    import roborts_csm
    pts = ONE_BEAM if beams == "one" else THREE_BEAMS
    sh = 1 << D
    ns = 2 * sh + 1
    p = _param(ns, 0.0, False)
    ctr = [_center(4, ns), _center(3, ns), 0.0]
    nd, dc = (sh + 1, sh + sh - 1), (sh - 1, 1)
    n_cell = _cells_read(pts, p, ctr, nd[0] * ns + nd[1])[0]
    d_cell = _cells_read(pts, p, ctr, dc[0] * ns + dc[1])[0]
    with roborts_csm.Context(0) as c:
        c.set_outside_value(outside)
        grid = _grid3(0.25, {d_cell: 0.5, n_cell: 0.5 + U})
        fixed, E, _ = R.fixed_point(grid, outside)
        assert E == 20 and fixed[0][d_cell[1], d_cell[0]] % 4096 == 0 and fixed[0][n_cell[1], n_cell[0]] % 4096 == 1
        b, _ = _search(c, grid, pts, p, ctr, D, top_kernel)
        assert n_cell in _cells_read(pts, p, ctr, b.flat_index)
        # the mirror needs E = 20 too: a far cell keeps the lattice
        far = (W - 1, H - 1)
        grid = _grid3(0.25, {d_cell: 0.5, n_cell: 0.5, far: 0.25 - U})
        assert R.fixed_point(grid, outside)[1] == 20
        b, _ = _search(c, grid, pts, p, ctr, D, top_kernel)
        cells = _cells_read(pts, p, ctr, b.flat_index)
        assert d_cell in cells and n_cell not in cells


@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("sign", [1, -1])
def test_values_at_the_int16_edge(sign, D):
    """E = 20 and cells at +(2^26 - 1) or -(2^26 - 1) fixed-point units, the
    largest the fixed-point grid accepts (level values 2^14 and -(2^14 - 1)):
    the hook's values equal the restatement and the search finds the needle,
    200 beams summed (nj = 10, 3, 1 top nodes per axis)."""
    import roborts_csm
    # |cell| + |outside| must stay below 2^26 units and float32 holds 24 bits: outside = -+48 and a
    # cell of +-(2^24 - 1) units are 2^26 - 1 units apart
    o = -sign * 48.0
    edge = sign * (2.0 ** 24 - 1) * U
    if sign > 0:
        B, N = -15.0, edge          # the needle is the edge value
    else:
        B, N = edge, 15.0           # the background is
    rng = np.random.default_rng(17)
    pts = np.round(rng.uniform(-20.0, 20.0, (200, 2)) * 4) / 4
    ns = 19
    p = _param(ns, 0.04, False, 200)
    ctr = np.array([[40.25, 36.25, 0.1]])
    grid = _grid3(B, {(44, 40): N, (30, 30): B + 0.5})
    fixed, E, oi = R.fixed_point(grid, o)
    assert E == 20 and sign * fixed.flat[np.argmax(np.abs(fixed))] == 2 ** 26 - 1
    lv = R.pooled_level(fixed[0], D)
    assert (lv.max() == 2 ** 14) if sign > 0 else (lv.min() == -(2 ** 14 - 1))
    with roborts_csm.Context(0) as c:
        c.set_outside_value(o)
        c.set_grid_stack(grid, RES, version=-1)
        sums, bounds = R.top_bounds(grid, o, pts, p, [0], ctr, MRES, D)
        assert np.array_equal(c.search_bounds(pts, p, [0], ctr, D, 0), sums)
        for kernel in (1, 2):
            assert np.array_equal(c.search_bounds(pts, p, [0], ctr, D, kernel).view(np.uint64), bounds.view(np.uint64))
        for top_kernel in (0, 1):
            b, _, st = check_same(c, pts, p, [0], ctr, max_depth=D, top_kernel=top_kernel)
            assert not st["exhaustive"]
            assert (44, 40) in _cells_read(pts, p, ctr[0], b.flat_index)


@pytest.mark.parametrize("top_kernel", [0, 1])
@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("beams", ["one", "three"])
def test_penalty_floor_is_0_45(D, top_kernel, beams):
    """Every value negative, the penalty on. The needle's candidate is the
    window's corner at the extreme angle, where dp = 0.5 and ap = 0.9: its
    score is 0.45 raw_N. The decoy at the window's centre scores strictly
    between 0.5 raw_N and 0.45 raw_N, and its node (the decoy one cell inside
    it on both axes, so no neighbour's pool sees it) is probed first: with a
    floor of 0.5 the needle's node, bounded at 0.5 raw_N, would be pruned.
    With three beams the needle and the decoy are three cells each, the ones
    the candidate's rotated beams read at that angle, so raw_N = N and raw_D =
    D still (with the other two beams on the background no negative decoy
    lies between 0.5 raw_N and 0.45 raw_N: (D + 2 B) / (N + 2 B) < 0.56 needs
    D > 0 when B < N < 0)."""
    import roborts_csm
    ns, dj = (65, 33) if D == 5 else (33, 17)   # nj = 17, 5, 3: the box path takes each
    origin, B, N, Dv = (20, 8), -1.0, -0.5, -17.0 / 64.0
    if beams == "three" and D == 5:
        # the beams lie 20 and 6 cells apart and a depth-5 pool is 33 wide: the decoy two nodes from the
        # needle's, so that node's pools see no decoy cell (nj = 4); further out dp is smaller, D lower
        ns, dj, origin, Dv = 97, 65, (4, 5), -11.0 / 32.0
    p = _param(ns, 0.4, True)
    pts = ONE_BEAM if beams == "one" else THREE_BEAMS
    ctr = np.array([_center(origin[0], ns), _center(origin[1], ns), 0.2])
    na = pyref.dims(p)[0]
    n_flat, d_flat = 0, dj * ns + dj            # angle 0: the extreme one
    n_cells = _cells_read(pts, p, ctr, n_flat)
    d_cells = _cells_read(pts, p, ctr, d_flat)
    assert len(set(n_cells) | set(d_cells)) == 2 * pts.shape[0]
    cells = {(W - 1, H - 1): B + U}
    cells.update({c: N for c in n_cells})
    cells.update({c: Dv for c in d_cells})
    grid = _grid3(B, cells)
    fixed, E, _ = R.fixed_point(grid, -1.0)
    assert E == 20 and all(fixed[0][y, x] % 4096 == 0 for x, y in n_cells + d_cells)
    use, step, angles, rows, xs, ys = pyref.geometry(pts.shape[0], p, ctr, MRES)
    assert use == pts.shape[0] and step == 1
    dp, ap = pyref.penalty_factors(p, ctr, MRES, angles, xs, ys)
    assert dp[n_flat] == 0.5 and ap[n_flat] == 0.9
    sc = O.score_window(O.Map(grid[0], RES, (0.0, 0.0), outside=-1.0), pts, p, ctr, na * ns * ns)
    assert sc[n_flat] == N * (0.5 * 0.9) == 0.45 * N and sc.max() == sc[n_flat] and (sc == sc.max()).sum() == 1
    assert 0.5 * N < sc[d_flat] < 0.45 * N
    assert _first_probed(grid, -1.0, pts, p, ctr, D) == (0, dj >> D, dj >> D)
    # what a floor of 0.5 would make of the needle's node: below the decoy's exact score
    win = R.Window(pts, p, ctr, MRES, D)
    raw = R.top_bounds(grid, -1.0, pts, _param(ns, 0.4, False), [0], [ctr], MRES, D)[1].reshape(win.na, win.nj, win.nj)
    assert raw[0, 0, 0] == N and 0.5 * raw[0, 0, 0] < sc[d_flat] < 0.45 * raw[0, 0, 0]
    with roborts_csm.Context(0) as c:
        c.set_outside_value(-1.0)
        b, _ = _search(c, grid, pts, p, ctr, D, top_kernel)
        assert b.flat_index == n_flat and b.score == 0.45 * N


@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("outside", [0.0, 0.75])
@pytest.mark.parametrize("beams", ["one", "three"])
def test_integer_thresholds_of_the_box_path(D, outside, beams):
    """pyr_expand_top_kernel prunes on integer sums against the incumbent's
    thresholds. The incumbent exactly on a node's bound, at both index orders
    (the tied node's lowest index above the incumbent's: pruned; below it:
    kept, and its cell wins the tie), then one level unit below a node's
    bound and one above another's: the exhaustive argmax each time, and the
    same nodes visited at every depth as the gather path, which compares
    doubles. With three beams the divisor is 3: the bound and the incumbent
    are rounded quotients. That the incumbent sits where each case wants it is
    asserted on the CPU: the incumbent the top probe leaves is the best oracle
    score under the node the probe takes (one window, one angle, 3 x 3 nodes:
    one partial, one probe root, in both paths)."""
    import roborts_csm
    # the second and third beam 100 cells away: further than a window and a pool together, so they read
    # background for every candidate and node and each case keeps its shape, now with a divisor of 3
    pts = ONE_BEAM if beams == "one" else np.array([[0.0, 0.0], [100.0, 0.0], [0.0, 100.0]])
    n = pts.shape[0]
    sh = 1 << D
    ns = 2 * sh + 1
    p = _param(ns, 0.0, False)
    ctr = [_center(4, ns), _center(3, ns), 0.0]
    shape = (205, 203)  # every pool of every beam inside the grid (with outside = 0.75 an off-grid cell is the best)

    def cell(j, k):
        return _cells_read(pts, p, ctr, j * ns + k)[0]

    far = (shape[1] - 1, shape[0] - 1)
    last = cell(ns - 1, ns - 1)
    grids = {
        # two cells of 0.5 = 128 level units exactly; node (0, 0) holds the first and is probed
        "above": ({cell(sh - 1, 1): 0.5, cell(sh + 1, sh + 1): 0.5, far: 0.25 - U}, (sh - 1, 1)),
        # the incumbent (j = 2^D - 1, k = 0) has a higher index than node (0, 1)'s lowest; that node's cell
        # (j = 0) wins the tie and must not be pruned
        "below": ({cell(sh - 1, 0): 0.5, cell(0, sh + 1): 0.5, far: 0.25 - U}, (0, sh + 1)),
        # the last node holds one candidate, the needle (129 units); its pool alone also reaches a cell
        # diagonally past the window (130 units after the ceiling) that no candidate reads: it is probed,
        # the incumbent becomes the needle, and its bound = incumbent + 1 unit;
        # the decoy's node (128) sits one unit below
        "one unit": ({last: 0.5 + 4096 * U, (last[0] + 1, last[1] + 1): 0.5 + 4097 * U, cell(1, 1): 0.5},
                     (ns - 1, ns - 1)),
    }
    win = R.Window(pts, p, ctr, MRES, D)
    J, K = np.meshgrid(np.arange(win.nj), np.arange(win.nj))          # [K, J], as the bounds
    low = (J << D) * ns + (K << D)
    with roborts_csm.Context(0) as c:
        c.set_outside_value(outside)
        for name, (cells, winner) in grids.items():
            grid = _grid3(0.25, cells, shape)
            _, E, oi = R.fixed_point(grid, outside)
            assert E == 20
            # the incumbent after the top probe, and the nodes on it / one unit from it
            sums, bnds = R.top_bounds(grid, outside, pts, p, [0], [ctr], MRES, D)
            sums, bnds = sums.reshape(win.nj, win.nj), bnds.reshape(win.nj, win.nj)
            _, pj, pk = _first_probed(grid, outside, pts, p, ctr, D)
            sc = O.score_window(O.Map(grid[0], RES, (0.0, 0.0), outside=outside), pts, p, ctr, ns * ns).reshape(ns, ns)
            blk = sc[pj << D:(pj + 1) << D, pk << D:(pk + 1) << D]
            inc = blk.max()
            bj, bk = np.argwhere(blk == inc)[0]
            inc_flat = ((pj << D) + bj) * ns + (pk << D) + bk
            other = (J != pj) | (K != pk)
            if name == "above":
                assert ((bnds == inc) & (low > inc_flat) & other).any()
            elif name == "below":
                assert ((bnds == inc) & (low < inc_flat) & other).any()
            else:
                assert (R.bound(sums - 1, n, oi, E, n, False) == inc).any()   # a bound one unit above it
                assert (R.bound(sums + 1, n, oi, E, n, False) == inc).any()   # and one one unit below
            b0, s0 = _search(c, grid, pts, p, ctr, D, 0)
            b1, s1 = _search(c, grid, pts, p, ctr, D, 1)
            assert b0.flat_index == b1.flat_index, name
            assert b0.flat_index == winner[0] * ns + winner[1], name
            assert s0["nodes"] == s1["nodes"], (name, s0["nodes"], s1["nodes"])
            if name == "one unit":
                lv = R.pooled_level(R.fixed_point(grid, outside)[0][0], D)
                vals = set(lv.reshape(-1).tolist()) - ({0} if outside else set())  # 0: pools reaching off the grid
                assert sorted(vals)[-2:] == [x + R.ceil_quant(int(-outside * 2 ** 20)) for x in (129, 130)]
