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

--capacity -1 is CSM_COLLECT_AUTO. Two further modes, for the list reduction
(profiles/list_reduce/speed.md):

  --parent-lib PATH   three legs of csm_search_match alone, interleaved:
                      PATH (another build of the library, e.g. the parent
                      commit's) at --capacity, this build at --capacity, this
                      build at -1; with --parent-default also PATH at its
                      default capacity. Medians, max - min, the 13 doubles of
                      every leg compared with cmp, and this build's split
                      (pyr_collect, list_select, the rest) from kernel_stats.
  --sweep             CSM_LIST_REDUCE_MIN: the reduced finish against the
                      whole-list finish on synthetic windows whose collected
                      sets hold about 1k .. 16k candidates.
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
                path=full["path"], collected=full["collected"], capacity=args.capacity if args.capacity else 10240,
                threshold=full["threshold"], response=full["response"], count=full["count"], window=full["window"],
                collect_nodes=full["collect_nodes"], search_nodes=full["search"]["nodes"],
                candidates=full["search"]["candidates"], library=roborts_csm.build_digest())
    print(json.dumps(line), flush=True)
    with open(os.path.join(args.out, f"{name}.json"), "w") as fh:
        json.dump(line, fh, indent=1)
    return line


class UseLib:
    """roborts_csm's calls go to `lib` inside the block (every Context method
    reads the module's _lib when it is called)."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        import roborts_csm
        self.old, roborts_csm._lib = roborts_csm._lib, self.lib

    def __exit__(self, *a):
        import roborts_csm
        roborts_csm._lib = self.old


def load_other(path):
    """Another build of the library, bound with this tree's prototypes. A
    build older than an entry point lacks its symbol: the name gets a stand-in
    that nothing here calls."""
    import ctypes as C
    from roborts_csm import _abi
    lib = C.CDLL(path)
    for name in _abi.EXPORTED:  # entry points newer than that build
        if not hasattr(lib, name):
            setattr(lib, name, lib.csm_abi_version)
    return _abi._bind(lib)


def _stats_ms(ctx, names):
    got = {s["name"]: s for s in ctx.kernel_stats()}
    return {n: (round(got[n]["total_ms"], 4) if n in got else 0.0) for n in names}, \
           {n: (int(got[n]["launches"]) if n in got else 0) for n in names}


def run_legs(name, make_ctx, pts, param, gi, centers, args):
    """The list reduction's A/B: csm_search_match on the parent build and on
    this one. make_ctx() -> a context holding the workload's grids, made by
    whichever library is current."""
    import roborts_csm
    parent = load_other(args.parent_lib)
    with UseLib(parent):
        pctx = make_ctx()
        parent_digest = parent.csm_build_digest().decode() if hasattr(parent, "csm_build_digest") else "?"
    nctx = make_ctx()
    cov0 = np.eye(3).reshape(9)
    legs = [("parent_explicit", pctx, parent, args.capacity), ("new_explicit", nctx, None, args.capacity),
            ("new_auto", nctx, None, -1)]
    if args.parent_default:
        legs.append(("parent_default", pctx, parent, 0))
    times = {n: [] for n, *_ in legs}
    out, info = {}, {}
    for k in range(args.warmup + args.repeats):
        for leg, ctx, lib, cap in legs:
            cov = cov0.copy()
            if lib is not None:
                with UseLib(lib):
                    t0 = time.perf_counter()
                    full = ctx.search_match(pts, param, gi, centers, cov, collect_capacity=cap)
                    t1 = time.perf_counter()
            else:
                t0 = time.perf_counter()
                full = ctx.search_match(pts, param, gi, centers, cov, collect_capacity=cap)
                t1 = time.perf_counter()
            if k >= args.warmup:
                times[leg].append(t1 - t0)
            out[leg] = np.concatenate([[full["response"]], full["pose_map"], cov])
            info[leg] = dict(path=full["path"], collected=full["collected"], window=full["window"])
    same = True
    for leg in out:
        out[leg].tofile(os.path.join(args.out, f"{name}_{leg}.bin"))
    for leg in out:
        same &= subprocess.run(["cmp", os.path.join(args.out, f"{name}_{leg}.bin"),
                                os.path.join(args.out, f"{name}_parent_explicit.bin")]).returncode == 0
    # this build's split, from one profiled call per leg (profiling adds event waits: not timed above)
    split = {}
    nctx.set_profiling(True)
    names = ["pyramid_search", "pyr_collect", "list_select"]
    for leg, cap in (("new_explicit", args.capacity), ("new_auto", -1)):
        before, _ = _stats_ms(nctx, names)
        t0 = time.perf_counter()
        nctx.search_match(pts, param, gi, centers, cov0.copy(), collect_capacity=cap)
        wall = (time.perf_counter() - t0) * 1e3
        after, launches = _stats_ms(nctx, names)
        d = {n: round(after[n] - before[n], 4) for n in names}
        d["wall_profiled_ms"] = round(wall, 4)
        d["host_rest_ms"] = round(wall - sum(after[n] - before[n] for n in names), 4)
        split[leg] = d
    counters = _stats_ms(nctx, ["search_match:reduced", "search_match:reduce_overflow", "search_match:regrown",
                                "search_match:exhaustive", "list_select"])[1]
    nctx.set_profiling(False)
    med = {leg: _median_ms(ts) for leg, ts in times.items()}
    spread = {leg: round((max(ts) - min(ts)) * 1e3, 4) for leg, ts in times.items()}
    limit = med["parent_explicit"] + spread["parent_explicit"]
    line = dict(workload=name, repeats=args.repeats, capacity=args.capacity, median_ms=med, max_minus_min_ms=spread,
                all_ms={leg: [round(t * 1e3, 3) for t in ts] for leg, ts in times.items()}, limit_ms=round(limit, 4),
                passes=bool(same and med["new_explicit"] <= limit and med["new_auto"] <= limit),
                outputs_identical=bool(same), legs=info, split_ms=split, counters=counters,
                library=roborts_csm.build_digest(), parent_library=parent_digest)
    print(json.dumps(line), flush=True)
    with open(os.path.join(args.out, f"{name}_legs.json"), "w") as fh:
        json.dump(line, fh, indent=1)
    with UseLib(parent):
        pctx.close()
    nctx.close()
    return line


def run_sweep(args):
    """CSM_LIST_REDUCE_MIN: csm_search_match with every set reduced (minimum 0)
    against none reduced, on synthetic 9-angle windows over a grid whose
    background keeps nearly every candidate at or above T = 0.5."""
    import roborts_csm
    from roborts_csm.params import CorrelationScanMatchParam
    rng = np.random.default_rng(3)
    q, sx, sy, res, ares = 2.0 ** -16, 157, 141, 0.05, 0.0349
    g = (36045 + rng.integers(-1500, 1501, (sy, sx))) * q
    wall = np.zeros((sy, sx), dtype=bool)
    cx, cy = sx // 2, sy // 2
    wall[cy - 8:cy + 9, cx - 10:cx + 11] = True
    wall[cy - 6:cy + 7, cx - 8:cx + 9] = False
    g[wall] = (58982 + rng.integers(-1500, 1501, int(wall.sum()))) * q
    ys, xs = np.nonzero(wall)
    pick = rng.choice(xs.size, size=100, replace=False)
    pts = np.stack([xs[pick] + rng.uniform(-0.3, 0.3, 100) - (cx + 0.3), ys[pick] + rng.uniform(-0.3, 0.3, 100) - (cy + 0.2)],
                   axis=1)
    centre = np.array([[cx + 1.3, cy - 0.8, 0.0]])
    ctxs = {}
    for label, v in (("reduced", "0"), ("whole", str(1 << 40))):
        os.environ["CSM_LIST_REDUCE_MIN"] = v
        c = roborts_csm.Context(0)
        c.set_outside_value(0.0)
        c.set_grid_stack(g[None].astype(np.float32), res, version=1)
        ctxs[label] = c
    os.environ.pop("CSM_LIST_REDUCE_MIN", None)
    rows = []
    for ns in (11, 15, 21, 31, 43, 61):
        param = CorrelationScanMatchParam((ns - 1) * res, res, 4 * ares + 0.002, ares, 0.0, 200, 0, False, 0)
        times = {k: [] for k in ctxs}
        full = {}
        for k in range(args.warmup + args.sweep_repeats):
            for label, c in ctxs.items():
                cov = np.eye(3).reshape(9)
                t0 = time.perf_counter()
                full[label] = c.search_match(pts, param, [0], centre, cov, collect_capacity=65536)
                t1 = time.perf_counter()
                if k >= args.warmup:
                    times[label].append(t1 - t0)
        row = dict(n_space=ns, collected=full["reduced"]["collected"], path=[full[k]["path"] for k in ctxs],
                   reduced_ms=_median_ms(times["reduced"]), whole_ms=_median_ms(times["whole"]),
                   reduced_spread_ms=round((max(times["reduced"]) - min(times["reduced"])) * 1e3, 4),
                   whole_spread_ms=round((max(times["whole"]) - min(times["whole"])) * 1e3, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    for c in ctxs.values():
        c.close()
    with open(os.path.join(args.out, "reduce_min_sweep.json"), "w") as fh:
        json.dump(rows, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/search_match")
    ap.add_argument("--workloads", default="config3,willow")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--submaps", type=int, default=512)
    ap.add_argument("--capacity", type=int, default=0,
                    help="collect_capacity (0: the default, 10240; -1: CSM_COLLECT_AUTO)")
    ap.add_argument("--parent-lib", default="", help="another build of the library: the three-leg A/B")
    ap.add_argument("--parent-default", action="store_true", help="... and that build at its default capacity")
    ap.add_argument("--sweep", action="store_true", help="the CSM_LIST_REDUCE_MIN sweep")
    ap.add_argument("--sweep-repeats", type=int, default=15)
    ap.add_argument("--willow-window-m", type=float, default=0.0, help="0: the whole padded map")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    import bench
    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.loop_closure import world_to_map, worlds_to_map
    from roborts_csm.params import CorrelationScanMatchParam
    ok = True
    if args.sweep:
        run_sweep(args)
        return
    for name in args.workloads.split(","):
        if name == "config3":
            bases, stack, pts, pose, offsets, param, res = bench._lc_config3(args.submaps)
            centers = worlds_to_map(pose, res, offsets)
            if args.parent_lib:
                def make_stack_ctx():
                    c = roborts_csm.Context(0)
                    c.set_grid_stack(stack, res, version=1)
                    return c
                ok &= run_legs(name, make_stack_ctx, pts, param, np.arange(args.submaps, dtype=np.int32), centers,
                               args)["passes"]
                continue
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
            if args.parent_lib:
                def make_map_ctx():
                    x = roborts_csm.Context(0)
                    x.set_grid(roborts_csm.ScanMatchMap(w.grid, w.resolution, w.offset, 0, 1))
                    return x
                tag = "willow_whole" if whole else "willow"
                ok &= run_legs(tag, make_map_ctx, pts, param, [0], c.reshape(1, 3), args)["passes"]
                continue
            with roborts_csm.Context(0) as ctx:
                ctx.set_grid(roborts_csm.ScanMatchMap(w.grid, w.resolution, w.offset, 0, 1))
                ok &= run(name, ctx, lambda _w: ctx, pts, param, [0], c.reshape(1, 3), pose, [w.offset], w.resolution,
                          args)["passes"]
        else:
            ap.error(f"unknown workload {name}")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
