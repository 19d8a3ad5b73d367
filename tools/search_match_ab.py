#!/usr/bin/env python3
"""A/B of the full ScanMatch result on the loop-closure workloads (one GPU):

  new  csm_search_match over every window (phase 1 + the collect + the finish)
  old  csm_scan_match on the winning window: every score, 8 bytes each to the
       host, std::sort there -- the only way to the same result without
       csm_search_match
  ref  csm_search_windows alone (what phase 2 adds to it)

Interleaved in one process, `--repeats` each after `--warmup`; the two results
(response, world pose, covariance: 13 doubles) are written to
OUT/<workload>_new.bin and _old.bin and compared with cmp. One JSON line per
workload: medians, collected, the collect's nodes per depth, path.

  config3  bench.py's config 3: 512 submaps 800x800, window 181 x 321^2
  willow   bench.py's config 4 map as one window of --willow-window-m metres
           (0: the whole padded map, 181 x 1566^2; the old path then moves
           3.5 GB and sorts 444 M keys per repeat)

  python3 tools/search_match_ab.py --out profiles/search_match [--workloads config3,willow]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "roborts-edu-slam_amd"), ROOT]


def _median_ms(ts):
    return round(statistics.median(ts) * 1e3, 4)


def run(name, ctx, single, pts, param, gi, centers, pose_world, offset, res, args):
    """ctx holds every window's grid; single(w) returns a context whose one
    grid is window w's (with its offset) for the old path."""
    import roborts_csm
    cov0 = np.eye(3).reshape(9)
    t_new, t_old, t_ref = [], [], []
    new = old = None
    full = None
    old_ctx, old_w = None, -1
    for k in range(args.warmup + args.repeats):
        cov = cov0.copy()
        t0 = time.perf_counter()
        full = ctx.search_match(pts, param, gi, centers, cov, collect_capacity=args.capacity)
        t1 = time.perf_counter()
        w = full["window"]
        if old_w != w:
            old_ctx, old_w = single(w), w
        pose = np.array(pose_world, dtype=np.float64)
        cov2 = cov0.copy()
        t2 = time.perf_counter()
        resp = old_ctx.scan_match(pts, param, pose, cov2)
        t3 = time.perf_counter()
        ctx.search_windows(pts, param, gi, centers)
        t4 = time.perf_counter()
        if k >= args.warmup:
            t_new.append(t1 - t0)
            t_old.append(t3 - t2)
            t_ref.append(t4 - t3)
        s = 1.0 / res
        pw = np.array(pose_world, dtype=np.float64)
        if full["accepted"]:  # GetWorldCoordsPose (grid_map_base.h:83-87)
            tx, ty = s * offset[w][0], s * offset[w][1]
            inv = s * (1.0 / (s * s - 0.0 * 0.0))
            pm = full["pose_map"]
            pw = np.array([inv * pm[0] + -(inv * tx), inv * pm[1] + -(inv * ty), pm[2]])
        new = np.concatenate([[full["response"]], pw, cov])
        old = np.concatenate([[resp], pose, cov2])
    fn, fo = os.path.join(args.out, f"{name}_new.bin"), os.path.join(args.out, f"{name}_old.bin")
    new.tofile(fn)
    old.tofile(fo)
    same = subprocess.run(["cmp", fn, fo]).returncode == 0
    line = dict(workload=name, repeats=args.repeats, new_ms=_median_ms(t_new), old_ms=_median_ms(t_old),
                search_only_ms=_median_ms(t_ref), phase2_ms=round(_median_ms(t_new) - _median_ms(t_ref), 4),
                new_all_ms=[round(t * 1e3, 3) for t in t_new], old_all_ms=[round(t * 1e3, 3) for t in t_old],
                outputs_identical=same, passes=bool(same and _median_ms(t_new) <= _median_ms(t_old)),
                path=full["path"], collected=full["collected"], capacity=args.capacity or 10240,
                threshold=full["threshold"], response=full["response"], count=full["count"], window=full["window"],
                collect_nodes=full["collect_nodes"], search_nodes=full["search"]["nodes"],
                candidates=full["search"]["candidates"], library=roborts_csm.build_digest())
    print(json.dumps(line), flush=True)
    with open(os.path.join(args.out, f"{name}.json"), "w") as fh:
        json.dump(line, fh, indent=1)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/search_match")
    ap.add_argument("--workloads", default="config3,willow")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--submaps", type=int, default=512)
    ap.add_argument("--capacity", type=int, default=0, help="collect_capacity (0: the default, 10240)")
    ap.add_argument("--willow-window-m", type=float, default=0.0, help="0: the whole padded map")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    import bench
    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.loop_closure import world_to_map, worlds_to_map
    from roborts_csm.params import CorrelationScanMatchParam
    ok = True
    for name in args.workloads.split(","):
        if name == "config3":
            bases, stack, pts, pose, offsets, param, res = bench._lc_config3(args.submaps)
            centers = worlds_to_map(pose, res, offsets)
            with roborts_csm.Context(0) as ctx, roborts_csm.Context(0) as one:
                ctx.set_grid_stack(stack, res, version=1)

                def single(w):
                    one.set_grid(roborts_csm.ScanMatchMap(stack[w], res, tuple(offsets[w]), 0, 1 + w), force=True)
                    return one
                ok &= run(name, ctx, single, pts, param, np.arange(args.submaps, dtype=np.int32), centers, pose,
                          offsets, res, args)["passes"]
        elif name == "willow":
            w = worlds.willow_world()
            batch = worlds.make_scan_batch(w, 1, seed=31)
            pts = batch.points_cells[batch.offsets[0]:batch.offsets[1]]
            sy, sx = w.grid.shape
            whole = args.willow_window_m <= 0.0
            window_m = max(sx, sy) * w.resolution if whole else args.willow_window_m
            param = CorrelationScanMatchParam(window_m, 0.05, math.pi, 0.0349, 0.5, 1081, 0, False, 0)
            pose = np.array(batch.init_poses[0], dtype=np.float64)
            if whole:  # the map's centre, as bench.py --whole-map
                s = 1.0 / w.resolution
                pose[0] = (sx / 2.0) / s - w.offset[0]
                pose[1] = (sy / 2.0) / s - w.offset[1]
            c = world_to_map(pose, w.resolution, w.offset)
            with roborts_csm.Context(0) as ctx:
                ctx.set_grid(roborts_csm.ScanMatchMap(w.grid, w.resolution, w.offset, 0, 1))
                ok &= run(name, ctx, lambda _w: ctx, pts, param, [0], c.reshape(1, 3), pose, [w.offset], w.resolution,
                          args)["passes"]
        else:
            ap.error(f"unknown workload {name}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
