"""A/B of the throughput path's input upload: fp64 points against float32
ranges against no upload at all.

Config 2's world and 4096-scan batch (make_world(2000, 2000, 0.05,
seed=20261015); the poses make_scan_batch(seed=1000) draws, their scans
ray-cast again as ranges), one process, bench.py's host-inputs loop
(double-buffered pinned inputs: queue batch i + 1, submit batch i) in three
forms that compute the same thing:

  points    csm_load_scans_async   the host-converted endpoints, 16 bytes a kept beam
  ranges    csm_load_ranges_async  the raw ranges, 4 bytes a beam; endpoints built on the device
  resident  no upload              the same endpoints loaded once before the loop

The forms run interleaved (their order rotates every repeat), each warmed up
first; per form the median and max - min of the repeats' ms/step are reported,
the last step's outputs of every form are compared byte for byte (and written
to --out for cmp), and the three ingest kernels' HIP-event times for one
batch are read from csm_kernel_stats. One JSON line on stdout.

  python tools/ranges_upload_ab.py [--scans 4096] [--steps 30] [--repeats 5] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="folder for the last step's outputs of each form (.bin, for cmp)")
    args = ap.parse_args()

    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.params import headline_levels

    levels = headline_levels()
    world = worlds.make_world(2000, 2000, 0.05, seed=20261015)
    batch = worlds.make_scan_batch(world, args.scans, seed=1000)
    spec = worlds.LaserSpec()
    laser = spec.to_c()
    factor = 1 / world.resolution
    ranges = worlds.raycast_ranges(world, batch.true_poses, spec)
    pts, off = roborts_csm.ranges_to_points(laser, ranges, factor)
    n = args.scans

    ctx = roborts_csm.Context(args.device)
    ctx.set_grid(roborts_csm.ScanMatchMap(world.grid, world.resolution, world.offset, 0, 1))
    poses0 = np.ascontiguousarray(batch.init_poses)
    covs0 = np.ascontiguousarray(np.tile(np.eye(3).reshape(1, 9), (n, 1)))
    sets = [(np.empty_like(poses0), np.empty_like(covs0), np.zeros(n)) for _ in range(2)]
    k_step = [0]

    def step():
        p, c, sc = sets[k_step[0] % 2]
        k_step[0] += 1
        np.copyto(p, poses0)
        np.copyto(c, covs0)
        ctx.scan_matchers_submit(levels, p, c, sc)
        return sc, p, c

    pin_pts = [roborts_csm.PinnedArray(pts.shape) for _ in range(2)]
    pin_rng = [roborts_csm.PinnedArray(ranges.shape, dtype=np.float32) for _ in range(2)]
    for p in pin_pts:
        np.copyto(p.array, pts)
    for p in pin_rng:
        np.copyto(p.array, ranges)

    def queue_points(i):
        ctx.load_scans_async(pin_pts[i % 2].array, off)

    def queue_ranges(i):
        ctx.load_ranges_async(laser, pin_rng[i % 2].array, factor)

    queue_s = {"points": [], "ranges": []}  # host time of each queueing call

    def run_uploaded(queue, k):
        queue(0)
        res = None
        for i in range(k):
            if i + 1 < k:
                t = time.perf_counter()
                queue(i + 1)
                queue_s["points" if queue is queue_points else "ranges"].append(time.perf_counter() - t)
            res = step()
        ctx.scan_matchers_wait()
        return tuple(np.array(a, copy=True) for a in res)

    def run_resident(k):
        res = None
        for _ in range(k):
            res = step()
        ctx.scan_matchers_wait()
        return tuple(np.array(a, copy=True) for a in res)

    forms = {
        "points": lambda k: run_uploaded(queue_points, k),
        "ranges": lambda k: run_uploaded(queue_ranges, k),
        "resident": run_resident,
    }

    def prepare(name):  # untimed: the resident form's one load
        if name == "resident":
            ctx.load_scans(pts, off)

    for name, fn in forms.items():
        prepare(name)
        fn(args.warmup)
    ms = {name: [] for name in forms}
    last = {}
    order = list(forms)
    for rep in range(args.repeats):
        for name in order[rep % 3:] + order[:rep % 3]:
            prepare(name)
            t = time.perf_counter()
            last[name] = forms[name](args.steps)
            ms[name].append((time.perf_counter() - t) / args.steps * 1e3)

    # the three ingest kernels, HIP events, one batch
    ctx.set_profiling(1)
    ctx.load_ranges(laser, pin_rng[0].array, factor)
    ingest = {s["name"]: s["total_ms"] / max(1, s["launches"]) for s in ctx.kernel_stats()
              if s["name"].startswith("ranges_")}
    ctx.set_profiling(0)
    back = ctx.loaded_scans()
    device_points_equal_host = bool(np.array_equal(back[1], off) and
                                    np.array_equal(back[0].view(np.uint64), pts.view(np.uint64)))

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(last[a], last[b]))

    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for name, res in last.items():
            with open(os.path.join(args.out, f"outputs_{name}.bin"), "wb") as fh:
                for a in res:  # scores, poses, covs
                    fh.write(a.tobytes())

    per_scan = 5070 + 1331 + 189
    out = {
        "tool": "ranges_upload_ab",
        "scans": n, "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
        "points_kept": int(off[-1]),
        "bytes_per_step": {"points": int(pts.nbytes), "ranges": int(ranges.nbytes), "resident": 0},
        "ms_per_step": {k: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}
                        for k, v in ms.items()},
        "scorings_per_s_at_median": {k: n * per_scan / (statistics.median(v) * 1e-3) for k, v in ms.items()},
        "ranges_outputs_equal_points": same("ranges", "points"),
        "resident_outputs_equal_points": same("resident", "points"),
        "device_points_equal_host": device_points_equal_host,
        "ingest_kernel_ms_one_batch": ingest,
        "queue_call_host_ms_median": {k: statistics.median(v) * 1e3 for k, v in queue_s.items() if v},
        "build": roborts_csm.build_digest(),
    }
    p, r = out["ms_per_step"]["points"], out["ms_per_step"]["ranges"]
    out["ranges_not_slower_than_points"] = bool(r["median"] <= p["median"] + p["spread_max_minus_min"])
    print(json.dumps(out))
    ctx.close()
    return 0 if out["ranges_outputs_equal_points"] and out["ranges_not_slower_than_points"] else 1


if __name__ == "__main__":
    sys.exit(main())
