"""Plain restatement of the admissible search's top-level bounds (test-only).

What csm_pyramid.hip computes for a top node, in Python integers and numpy,
with nothing of the kernels' structure: no two-tap recursion, no phase-split
columns, no lanes. A window's candidates, beams, angle rows and divisor come
from pyref.geometry, the code the exact scores are restated with.

  fixed point  (float64(g) - float64(outside)) * 2^E, E the smallest E >= 0
               making every cell and outside an integer (csm_grid.cpp)
  level d      anchor (x, y), x, y in [-2^d, size): ceil(max over
               [x, x + 2^d] x [y, y + 2^d] / 2^12), off-grid cells 0
  node sum     over the used beams, level d at the anchor candidate's cell
               trunc(fl(fl(lx + x) + 0.5)), x = fl(x0 + J 2^d); 0 off the level
  bound        raw = fl(fl((sum 2^12 + n_used outside_i) 2^-E) / divisor);
               raw, or raw * 0.45 when the penalty is on and raw < 0
"""
from __future__ import annotations

import numpy as np

import pyref

QUANT = 12          # kPyrQuant
MARGIN = 2.0 ** -20  # kTopBoxMargin


class Unsupported(ValueError):
    pass


def scene(sx=93, sy=77, seed=5):
    """The bound tests' grid stack [3, sy, sx]: a blurred occupancy grid (values
    on a 2^-20 lattice), cells drawn from {0, 0.25, 0.5, 1}, and a copy of the
    first (cross-window ties). Both sides odd: no level width is a multiple of
    4, the levels' pad columns are in play."""
    rng = np.random.default_rng(seed)
    occ = (rng.random((sy + 4, sx + 4)) < 0.2).astype(np.float64)
    blur = sum(occ[dy:dy + sy, dx:dx + sx] for dy in range(5) for dx in range(5)) / 25.0
    blur = np.floor(np.minimum(1.0, 2.5 * blur) * 2.0 ** 20) / 2.0 ** 20
    steps = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), size=(sy, sx))
    return np.stack([blur, steps, blur]).astype(np.float32)


def fixed_point(grids, outside):
    """(int64 cells, E, outside_i) of a float32 grid or stack."""
    g = np.asarray(grids, dtype=np.float32).astype(np.float64)
    o = float(np.float32(outside))
    E = 0
    while True:
        s = 2.0 ** E
        if np.all(g * s == np.floor(g * s)) and o * s == np.floor(o * s):
            break
        E += 1
        if E > 60:
            raise Unsupported("no common binary lattice")
    s = 2.0 ** E
    if (float(np.abs(g).max()) + abs(o)) * s >= 2.0 ** 26:
        raise Unsupported("fixed-point values reach 2^26")
    gi = (g - o) * s
    assert np.all(gi == np.floor(gi)) and float(np.abs(gi).max()) < 2.0 ** 26
    return gi.astype(np.int64), E, int(o * s)


def ceil_quant(m):
    """ceil(m / 2^12) of Python or numpy integers."""
    return -((-m) >> QUANT)


def pooled_level(gi: np.ndarray, d: int, span: int | None = None) -> np.ndarray:
    """Level d of one int64 grid [H, W]: out[y + 2^d, x + 2^d] for anchors x in
    [-2^d, W), y in [-2^d, H). span: cells past the anchor the pool reaches
    (2^d; a test passes 2^d - 1 to state what a dropped tap would give)."""
    H, W = gi.shape
    sh = 1 << d
    span = sh if span is None else span
    pad = np.zeros((H + 2 * sh + 1, W + 2 * sh + 1), dtype=np.int64)  # off-grid: 0
    pad[sh:sh + H, sh:sh + W] = gi
    m = None
    for ty in range(span + 1):
        for tx in range(span + 1):
            v = pad[ty:ty + H + sh, tx:tx + W + sh]
            m = v.copy() if m is None else np.maximum(m, v)
    return ceil_quant(m)


class Window:
    """One window of a scan: geometry and the top level's shape at depth d."""

    def __init__(self, pts, p, center, mres, d):
        self.pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
        self.p, self.center, self.mres, self.d = p, np.asarray(center, dtype=np.float64), mres, d
        self.na, self.ns = pyref.dims(p)
        self.use, self.step, self.angles, self.rows, self.xs, self.ys = pyref.geometry(
            self.pts.shape[0], p, self.center, mres)
        self.beams = self.pts[::self.step]
        self.n_used = self.beams.shape[0]
        self.nj = (self.ns + (1 << d) - 1) >> d

    def rotated(self, a):
        c, s = self.rows[a]
        px, py = self.beams[:, 0], self.beams[:, 1]
        return c * px - s * py, s * px + c * py                   # :179-180

    def anchor_cells(self, a):
        """(gx [beam, J], gy [beam, K]): the anchor candidates' cells."""
        lx, ly = self.rotated(a)
        xa = self.xs[np.arange(self.nj) << self.d]
        ya = self.ys[np.arange(self.nj) << self.d]
        gx = np.trunc((lx[:, None] + xa[None, :]) + 0.5).astype(np.int64)  # :647
        gy = np.trunc((ly[:, None] + ya[None, :]) + 0.5).astype(np.int64)  # :648
        return gx, gy

    def clean(self, a):
        """pyr_topbox_kernel's test per beam: True = the box path takes the
        beam, False = it is summed node by node."""
        lx, ly = self.rotated(a)
        tx = (lx + self.xs[0]) + 0.5
        ty = (ly + self.ys[0]) + 0.5
        fx, fy = tx - np.floor(tx), ty - np.floor(ty)
        return ((tx >= 0.0) & (ty >= 0.0) & (fx >= MARGIN) & (fx <= 1.0 - MARGIN) &
                (fy >= MARGIN) & (fy <= 1.0 - MARGIN))


def node_sums(win: Window, level: np.ndarray) -> np.ndarray:
    """Integer sums [angle, K, J] of the window's top nodes on a pooled level
    (pooled_level's layout)."""
    sh = 1 << win.d
    Hl, Wl = level.shape
    out = np.zeros((win.na, win.nj, win.nj), dtype=np.int64)
    for a in range(win.na):
        gx, gy = win.anchor_cells(a)
        gx, gy = gx + sh, gy + sh
        okx = (gx >= 0) & (gx < Wl)
        oky = (gy >= 0) & (gy < Hl)
        v = level[np.clip(gy, 0, Hl - 1)[:, :, None], np.clip(gx, 0, Wl - 1)[:, None, :]]
        out[a] = np.where(oky[:, :, None] & okx[:, None, :], v, 0).sum(axis=0)
    return out


def bound(sums, n_used: int, outside_i: int, E: int, divisor: int, penalty: bool) -> np.ndarray:
    """The doubles the search compares, from integer node sums."""
    flat = np.asarray(sums, dtype=np.int64).reshape(-1)
    out = np.empty(flat.size)
    scale = 2.0 ** -E
    for i, s in enumerate(flat.tolist()):
        raw = (float(s * (1 << QUANT) + n_used * outside_i) * scale) / float(divisor)
        out[i] = raw * 0.45 if (penalty and raw < 0.0) else raw
    return out.reshape(np.shape(sums))


def top_bounds(grids, outside, pts, p, grid_index, centers, mres, d, levels=None):
    """(sums, bounds) of every top node in the search's list order (window,
    angle, K, J), J fastest; levels: pooled levels by grid index, if built."""
    gi, E, oi = fixed_point(grids, outside)
    gi = gi.reshape((-1,) + gi.shape[-2:])
    levels = {} if levels is None else levels
    sums = []
    for w, g in enumerate(grid_index):
        g = int(g)
        if g not in levels:
            levels[g] = pooled_level(gi[g], d)
        win = Window(pts, p, centers[w], mres, d)
        sums.append(node_sums(win, levels[g]))
    sums = np.stack(sums)
    return sums.reshape(-1), bound(sums, win.n_used, oi, E, win.use, bool(p.use_center_penalty)).reshape(-1)
