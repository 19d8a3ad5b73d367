"""Shared by the chain-map tests: the small cases, the oracle build of a stack
(the yardstick) and a NumPy restatement of the splat rule of
csrc/csm_chain_maps.hip with switches that break it one way each (the
restatement is how the rule's mutations are tried without a GPU).

The small shape: grids of 64 x 48 cells at 0.08 m, eight kept scans of 7 to 64
points. Scan 0 is crafted around an axis-aligned pose whose map coordinates are
binary-exact: end points on and next to the in-map band's edge for half
kernels 2 and 7 on all four sides, in the start cell, at exactly .5, negative,
far off the map, NaN and infinite. The others are seeded: random poses, points
over the map and past its edges."""
import math

import numpy as np

import pyoracle as O
from libm import sincos

RES = 0.08
SIZE_X, SIZE_Y = 64, 48
MAP_OFFSET = (2.0, 1.5)
DEFAULT = 0.3
POSE0 = (0.5, 0.25, 0.0)  # map coordinates (31.25, 21.875): start cell (31, 22)

# (deviation, gaussian_blur_offset): half kernels 2 and 7; 1.2 puts table values above 1
BLURS = {"hk2": (0.24, 0.72), "hk7_over1": (0.7, 1.2), "hk2_over1": (0.24, 1.2)}

# grids of the 5-grid stack: an empty chain, one scan, four scans, a scan twice
# in a chain, and scans that other grids hold too
CHAINS5 = [[], [0], [0, 1, 2, 3], [2, 2, 4], [0, 5, 6, 7]]
CHAINS1 = [[0, 1, 2, 3]]


def half_kernel(dev, res=RES):
    return int((dev / res) * math.sqrt(math.log(2)))


def _crafted_scan():
    """Scan 0: metres in the sensor frame of POSE0, by the map cell wanted."""
    s = 1.0 / RES
    tx, ty = s * POSE0[0] + s * MAP_OFFSET[0], s * POSE0[1] + s * MAP_OFFSET[1]

    def at(cx, cy):
        return ((cx - tx) * RES, (cy - ty) * RES)

    pts = []
    for hk in (2, 7):
        tol = hk + 1
        # on the band's edge (skipped) and one cell inside it (drawn), four sides
        pts += [at(tol, 20), at(tol + 1, 21), at(SIZE_X - tol, 23), at(SIZE_X - tol - 1, 24),
                at(30, tol), at(33, tol + 1), at(34, SIZE_Y - tol), at(35, SIZE_Y - tol - 1)]
    pts += [(0.0, 0.0), (0.01, 0.01), (-0.02, 0.0)]          # the start cell
    pts += [(0.5, -0.75), (-1.5, 1.25), (0.5, 1.25)]          # map coordinates exactly k + .5
    pts += [at(-3, 10), at(10, -7), at(-0.5, -0.5), (-40.0, -55.0), (1.0e6, 2.0), (3.0, -1.0e12), (1.0e300, 1.0e300)]
    pts += [(float("nan"), 0.5), (0.5, float("nan")), (float("inf"), 0.0), (0.0, float("-inf"))]
    pts += [at(40, 30), at(41, 30), at(40, 31), at(20, 15)]  # overlapping splats well inside
    return np.array(pts, dtype=np.float64)


def small_scans():
    """-> (list of [n, 2] metre arrays, [8, 3] poses)."""
    rng = np.random.default_rng(91)
    scans, poses = [_crafted_scan()], [POSE0]
    for n in (7, 64, 33, 19, 50, 12, 41):
        pose = (float(rng.uniform(-0.6, 1.6)), float(rng.uniform(-0.6, 1.2)), float(rng.uniform(-math.pi, math.pi)))
        scans.append(rng.uniform(-2.9, 2.9, (n, 2)))
        poses.append(pose)
    assert all(7 <= s.shape[0] <= 64 for s in scans)
    return scans, np.array(poses, dtype=np.float64)


def moved_poses(poses):
    """The poses after a graph solve: every scan but the crafted one moves."""
    rng = np.random.default_rng(92)
    out = poses.copy()
    out[1:] += rng.uniform(-0.2, 0.2, (poses.shape[0] - 1, 3))
    return out


# ---- the yardstick -----------------------------------------------------------------
def oracle_stack(scans_m, poses, chains, dev, blur_offset, size=(SIZE_X, SIZE_Y), res=RES, map_offset=MAP_OFFSET,
                 default=DEFAULT):
    """Each grid as the oracle's ScanMatchMap: Reset(), then
    ResetScanMatchMapWithRangeVec (no auto resize, just_update_occu, the map
    offset) with the chain's scans scaled by CreateFrom(raw, 1 / resolution)."""
    out = []
    for chain in chains:
        g = O.GridMap(0, res, size, map_offset, dev, default)
        g.reset()
        g.set_options(False, True, blur_offset, 0)
        g.set_map_offset(map_offset[0], map_offset[1])
        g.init_with_range_vec([np.asarray(scans_m[i]) * (1 / res) for i in chain], [poses[i] for i in chain],
                              use_blur=True, speedup=True)
        out.append(g.cells()[0].copy())
    return np.stack(out)


# ---- the rule, restated ----------------------------------------------------------------
def _cells(v):
    """(int)(v + 0.5) where the cast is defined; elsewhere a cell far outside any grid."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = v + 0.5
        ok = (r > -2147483648.0) & (r < 2147483647.0)
        return np.where(ok, np.trunc(np.where(ok, r, 0.0)), -2147483648.0).astype(np.int64)


def pyref_stack(scans_m, poses, chains, dev, blur_offset, size=(SIZE_X, SIZE_Y), res=RES, map_offset=MAP_OFFSET,
                default=DEFAULT, mutate=None, stats=None):
    """The stack by the kernel's rule. mutate: None, or one of "band_hk" (the
    band test weakened from hk + 1 to hk), "no_centre", "no_le1" (table values
    above 1 drawn too), "no_start_skip". stats: a dict that collects how many
    points took each branch."""
    sx, sy = size
    hk = half_kernel(dev, res)
    ks = 2 * hk + 1
    tab = np.zeros((ks, ks), dtype=np.float32)  # [j + hk, i + hk]
    for i in range(-hk, hk + 1):
        for j in range(-hk, hk + 1):
            q = math.hypot(i * res, j * res) / dev
            tab[j + hk, i + hk] = np.float32(math.exp(-0.5 * (q * q)) * blur_offset)
    tol = hk if mutate == "band_hk" else hk + 1
    s = 1.0 / res
    grids = np.full((len(chains), sy, sx), np.float32(default), dtype=np.float32)
    st = stats if stats is not None else {}
    for g, chain in enumerate(chains):
        for i in chain:
            pose = poses[i]
            tx, ty = s * pose[0] + s * map_offset[0], s * pose[1] + s * map_offset[1]
            c, sn = sincos(pose[2])
            with np.errstate(invalid="ignore", over="ignore"):
                px, py = np.asarray(scans_m[i])[:, 0] * s, np.asarray(scans_m[i])[:, 1] * s
                ex = (c * px + (-sn) * py) + tx
                ey = (sn * px + c * py) + ty
                half = np.isfinite(ex) & np.isfinite(ey) & ((ex + 0.5 == np.floor(ex + 0.5)) | (ey + 0.5 == np.floor(ey + 0.5)))
            x1, y1 = _cells(ex), _cells(ey)
            x0, y0 = int(_cells(np.array([tx]))[0]), int(_cells(np.array([ty]))[0])
            start = (x1 == x0) & (y1 == y0)
            inside = (x1 > tol) & (x1 < sx - tol) & (y1 > tol) & (y1 < sy - tol)
            keep = inside & (~start if mutate != "no_start_skip" else True)
            st["start"] = st.get("start", 0) + int((start & inside).sum())
            st["half"] = st.get("half", 0) + int((half & keep).sum())
            st["nonfinite"] = st.get("nonfinite", 0) + int((~np.isfinite(ex) | ~np.isfinite(ey)).sum())
            for name, m in (("edge_x_lo", x1 == hk + 1), ("edge_x_hi", x1 == sx - hk - 1), ("edge_y_lo", y1 == hk + 1),
                            ("edge_y_hi", y1 == sy - hk - 1), ("in_x_lo", x1 == hk + 2), ("in_x_hi", x1 == sx - hk - 2),
                            ("in_y_lo", y1 == hk + 2), ("in_y_hi", y1 == sy - hk - 2)):
                other = (y1 > hk + 1) & (y1 < sy - hk - 1) if "_x_" in name else (x1 > hk + 1) & (x1 < sx - hk - 1)
                st[name] = st.get(name, 0) + int((m & other & ~start).sum())
            for x, y in zip(x1[keep].tolist(), y1[keep].tolist()):
                win = grids[g, y - hk:y + hk + 1, x - hk:x + hk + 1]
                if mutate != "no_centre":
                    grids[g, y, x] = max(grids[g, y, x], np.float32(1.0))
                ok = np.ones_like(tab, dtype=bool) if mutate == "no_le1" else tab <= np.float32(1.0)
                np.maximum(win, np.where(ok, tab, np.float32(0.0)), out=win)
    return grids


# ---- the mid-size case: ray-cast scans in a room world -------------------------------------
def mid_case(n_scans=11, n_grids=16, size=300, res=RES, seed=7):
    """-> (scans in metres, poses, chains, map_offset): n_scans scans of 1081
    ray-cast beams along a short drive, n_grids chains that share them, the
    maps centred on the last pose (ResetScanMatchMapWithRangeVec :452-454)."""
    from roborts_csm import worlds
    world = worlds.make_world(400, 400, resolution=0.05, seed=20261015)
    laser = worlds.LaserSpec()
    rng = np.random.default_rng(seed)
    p0 = worlds.sample_free_poses(world, 1, rng)[0]
    poses = np.stack([p0 + np.array([0.05 * k, 0.03 * k, 0.02 * k]) for k in range(n_scans)])
    ranges = worlds.raycast_ranges(world, poses, laser)
    scans = [worlds.scan_points(ranges[k], laser) for k in range(n_scans)]
    assert all(s.shape[0] > 100 for s in scans)
    chains = [[(g + k) % n_scans for k in range(1 + g % n_scans)] for g in range(n_grids - 1)] + [list(range(n_scans))]
    cell = 1 / (1.0 / res)
    cur = poses[-1]
    map_offset = (-(cur[0] - 0.5 * size * cell), -(cur[1] - 0.5 * size * cell))
    return scans, poses, chains, map_offset
