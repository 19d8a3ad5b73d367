#!/usr/bin/env python3
"""Share of beams and runs whose whole box holds the map's background value
(the pair kernel's map of uniform boxes, csrc/csm_palette.hip bg_map_kernel).
CPU only (numpy and scipy, no built library): the bench's config-2 world and
scans, or the willow map. The corners here come from the plain formulas, not
from the kernels' fixed-point path, so the shares are estimates.

  python tools/uniform_box_share.py [--world config2|willow] [--scans 48]

Coarse level: 13 x 13 boxes over the 30 angles of the window around each
scan's initial pose, runs being consecutive beams with one box corner, as the
kernel's run list has them. Fine level: 5 x 5 boxes over 11 angles around the
true pose. Also the share of set bits among the map's corners, which the
library compares with its threshold (csm_grid.cpp kBgMinShare).
"""
import argparse
import os
import sys

import numpy as np

import importlib.util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# worlds.py alone: importing the package would load the built library
_spec = importlib.util.spec_from_file_location(
    "csm_worlds", os.path.join(ROOT, "roborts-edu-slam_amd", "roborts_csm", "worlds.py"))
worlds = importlib.util.module_from_spec(_spec)
sys.modules["csm_worlds"] = worlds
_spec.loader.exec_module(worlds)

PAD = 16  # kStripPadLo


def uniform_map(grid, n, outside=np.float32(0.3)):
    """U[y, x] for padded corners (counted from -PAD): the n x n cells from the
    corner all hold the background, in the padded image the strips hold
    (column -1 and row -1 repeat the grid's first, the rest is outside)."""
    vals, counts = np.unique(grid, return_counts=True)
    bg = vals[np.argmax(counts)]
    sy, sx = grid.shape
    img = np.full((PAD + sy + n, PAD + sx + n), outside, dtype=np.float32)
    img[PAD:PAD + sy, PAD:PAD + sx] = grid
    img[PAD - 1, PAD:PAD + sx] = grid[0]
    img[PAD:PAD + sy, PAD - 1] = grid[:, 0]
    img[PAD - 1, PAD - 1] = grid[0, 0]
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), dtype=np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(img == bg, axis=0), axis=1)
    box = s[n:, n:] - s[:-n, n:] - s[n:, :-n] + s[:-n, :-n]
    return (box == n * n)[:PAD + sy, :PAD + sx], bg, float(counts.max()) / grid.size


def shares(U, pts, offs, poses_cells, half_cells, angle_off, angle_res, n_angles):
    beams = hit_beams = runs = hit_runs = 0
    for s in range(len(offs) - 1):
        p = pts[offs[s]:offs[s + 1]]
        cx, cy, ct = poses_cells[s]
        for a in range(n_angles):
            th = ct - angle_off + a * angle_res
            c, sn = np.cos(th), np.sin(th)
            ix = np.floor(c * p[:, 0] - sn * p[:, 1] + (cx - half_cells) + 0.5).astype(np.int64) + PAD
            iy = np.floor(sn * p[:, 0] + c * p[:, 1] + (cy - half_cells) + 0.5).astype(np.int64) + PAD
            ok = (ix >= 0) & (iy >= 0) & (ix < U.shape[1]) & (iy < U.shape[0])
            u = np.zeros(len(p), dtype=bool)
            u[ok] = U[iy[ok], ix[ok]]
            head = np.ones(len(p), dtype=bool)
            head[1:] = (ix[1:] != ix[:-1]) | (iy[1:] != iy[:-1])
            head &= ok
            beams += int(ok.sum())
            hit_beams += int(u.sum())
            runs += int(head.sum())
            hit_runs += int((head & u).sum())
    return beams, hit_beams, runs, hit_runs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--world", choices=["config2", "willow"], default="config2")
    ap.add_argument("--scans", type=int, default=48)
    args = ap.parse_args()
    w = worlds.make_world(2000, 2000, seed=20261015) if args.world == "config2" else worlds.willow_world()
    b = worlds.make_scan_batch(w, args.scans, seed=1000)

    def cells(poses):
        out = np.array(poses, dtype=np.float64)
        out[:, 0] = (out[:, 0] + w.offset[0]) / w.resolution
        out[:, 1] = (out[:, 1] + w.offset[1]) / w.resolution
        return out

    U13, bg, cover = uniform_map(w.grid, 13)
    print(f"{args.world}: {w.size_x} x {w.size_y} cells, background {bg:.4g} covers {100 * cover:.1f} % of them; "
          f"{100 * U13.mean():.1f} % of the 13 x 13 map's corners are set")
    nb, hb, nr, hr = shares(U13, b.points_cells, b.offsets, cells(b.init_poses), 6.0, 0.523, 0.0349, 30)
    print(f"coarse (13 x 13, 30 angles around the initial pose): {100 * hr / nr:.1f} % of runs, "
          f"{100 * hb / nb:.1f} % of beams uniform; {nr / (args.scans * 30):.0f} runs per wave")
    U5, _, _ = uniform_map(w.grid, 5)
    nb, hb, nr, hr = shares(U5, b.points_cells, b.offsets, cells(b.true_poses), 2.0, 0.175, 0.0349, 11)
    print(f"fine (5 x 5, 11 angles around the true pose): {100 * hb / nb:.1f} % of beams uniform")


if __name__ == "__main__":
    main()
