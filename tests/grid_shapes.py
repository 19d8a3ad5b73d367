"""The grid shapes at which the layouts' arithmetic is tight, and the grids and
scans the GPU tests score on them (test-only). tests/test_grid_geom.py proves
the bounds of every shape on the CPU; tests/test_gpu_grid_shapes.py scores them."""
import numpy as np

# numpy (size_y, size_x)
SHAPES = [
    (29, 33),  # sx = 1 mod 4: no spare pitch column; sx = 1 mod 16
    (33, 45),  # sx = 1 mod 4, 13 mod 16, 5 mod 8
    (31, 47),  # sx = 3 mod 4, 15 mod 16
    (40, 49),  # sx = 1 mod 4, 1 mod 8
    (17, 16),  # one strip wide
    (12, 13),  # lower than the 13 x 13 box
    (5, 3),    # narrower than every box; the row kernel's narrow-grid branch
    (1, 37),
    (37, 1),
    (1, 1),
]

RES = 0.05  # the sim levels' steps on it: 1, 0.4 and 0.2 cells
OUTSIDE = np.float32(0.3)  # the contexts' default outside value
# exactly summable (the suite's four): the outside value itself, then three above it
VALS = np.array([0.3, 0.41, 0.88, 1.0], dtype=np.float32)
BG_MIN_SHARE = 0.16  # csm_grid_copies.hpp kBgMinShare
PAD_LO = 16          # kStripPadLo


def _ring(g, rng):
    """The outermost two rows and columns hold only the two highest values: a
    read that wraps into the next row, or runs on past the last, meets a
    non-zero cell where the pad's zero belongs."""
    sy, sx = g.shape
    edge = np.ones(g.shape, dtype=bool)
    edge[2:sy - 2, 2:sx - 2] = False
    g[edge] = rng.choice(VALS[2:], size=int(edge.sum()))
    return edge


def ring4(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.choice(VALS, size=shape)
    _ring(g, rng)
    return np.ascontiguousarray(g, dtype=np.float32)


def values40(shape, seed):
    """40 distinct values k / 64: more than the pair kernel's 16-value palettes."""
    rng = np.random.default_rng(seed)
    vals = (np.arange(10, 50) / 64.0).astype(np.float32)
    g = rng.choice(vals, size=shape)
    g.ravel()[rng.choice(g.size, size=40, replace=False)] = vals  # every one of them
    return np.ascontiguousarray(g, dtype=np.float32)


def _sparse_of(shape, seed, fill, share=0.15, odd=3):
    rng = np.random.default_rng(seed)
    sy, sx = shape
    g = np.full(shape, fill, dtype=np.float32)
    edge = _ring(g, rng)
    inner = np.flatnonzero(~edge.ravel())
    others = VALS[VALS != np.float32(fill)]
    n_other = int(round(share * inner.size))
    # a band along the ring's upper inside (walls are bands), and `odd` odd cells further in
    n_odd = min(odd, n_other)
    band = inner[:n_other - n_odd]
    g.ravel()[band] = rng.choice(others, size=band.size)
    if n_odd:
        odd = rng.choice(inner[n_other - n_odd:], size=n_odd, replace=False)
        g.ravel()[odd] = rng.choice(others, size=n_odd)
    return g


def uniform_corners(g, n, outside=OUTSIDE):
    """The map of uniform n x n boxes as csm_palette.hip bg_map_kernel builds
    it, restated: (set bits, bits in the map). The padded image holds the grid,
    column -1 and row -1 repeating column 0 and row 0, and the outside value
    everywhere else; the background is the value most in-grid cells hold (of
    equal counts, the lowest palette index: the outside value, then ascending);
    a corner's bit is set when the n x n cells from it all hold the background.
    The map has a bit for every corner of its 8 x 8 tiles."""
    sy, sx = g.shape
    nx, ny = 8 * ((PAD_LO + sx + 7) // 8), 8 * ((PAD_LO + sy + 7) // 8)
    xs, ys = np.arange(nx + n - 1) - PAD_LO, np.arange(ny + n - 1) - PAD_LO
    inx, iny = (xs >= -1) & (xs < sx), (ys >= -1) & (ys < sy)
    img = np.where(iny[:, None] & inx[None, :], g[np.clip(ys, 0, sy - 1)][:, np.clip(xs, 0, sx - 1)],
                   np.float32(outside))
    vals, counts = np.unique(g, return_counts=True)
    order = sorted(range(vals.size), key=lambda i: (vals[i] != np.float32(outside), vals[i]))
    bg, best = None, 0
    for i in order:
        if counts[i] > best:
            bg, best = vals[i], counts[i]
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), dtype=np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(img == bg, axis=0), axis=1)
    box = s[n:n + ny, n:n + nx] - s[:ny, n:n + nx] - s[n:n + ny, :nx] + s[:ny, :nx]
    return int((box == n * n).sum()), nx * ny


def sparse(shape, seed):
    """About 85 % of the cells inside the ring hold one value, the fill. The
    fill is chosen here, from the shape: a value above the outside value where
    both maps of uniform boxes (13 x 13 and 5 x 5) then reach kBgMinShare, so
    the constant a dropped beam adds is not zero; with 90 % of it in one band
    (no odd cells) where 85 % does not reach the share; else the outside value,
    which the cells off the grid hold too. A map's bits cover the corners of
    whole 8 x 8 tiles, (16 + size) rounded up per axis, and a fill above the
    outside value sets only corners whose box lies inside the ring, at most
    (sx - 16) (sy - 16) of them: of the shapes here that reaches 16 % at
    (40, 49) alone (33 * 24 of 72 * 56). Returns (grid, fill, both maps are read)."""
    for fill, share, odd in ((VALS[1], 0.15, 3), (VALS[1], 0.10, 0), (VALS[0], 0.15, 3)):
        g = _sparse_of(shape, seed, fill, share, odd)
        shares = [s / n for s, n in (uniform_corners(g, 13), uniform_corners(g, 5))]
        if min(shares) >= BG_MIN_SHARE:
            return g, fill, True
    return g, fill, False


def scan(shape, n, seed):
    """n - 8 points uniform in +-1.5 max(size) cells (beams end on the grid, on
    its last row or column, and off every edge), then the eight of
    test_box_kernel_edge_beams scaled from its 2000-cell grid: two at the
    origin and one a quarter cell from it (rounding boundaries), and points
    far off each side."""
    rng = np.random.default_rng(seed)
    m = float(max(shape))
    far = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, -2.0], [-0.75 * m, 3.0], [2.0, -0.75 * m], [0.45 * m, 0.45 * m],
                    [-1.5 * m, -1.5 * m], [0.25, 0.0]])
    return np.ascontiguousarray(np.concatenate([rng.uniform(-1.5 * m, 1.5 * m, size=(n - 8, 2)), far]))


def centres(shape):
    """The grid's middle; the high corner, where every box straddles the last
    column, the last row and the pads; the low corner, with beams at negative
    cells (truncation is not a floor there)."""
    sy, sx = shape
    return [np.array([sx // 2 + 0.5, sy // 2 + 0.5, 1.3]), np.array([sx - 1 + 0.37, sy - 1 + 0.61, -0.4]),
            np.array([0.3, 0.2, 2.9])]
