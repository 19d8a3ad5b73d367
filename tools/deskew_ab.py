"""A/B of the motion de-skew in front of the ranges upload: on the host before
csm_load_ranges_async against csm_load_ranges_deskewed_async (DESIGN.md
section 11).

Config 2's world and 4096-scan batch (make_world(2000, 2000, 0.05,
seed=20261015); the poses make_scan_batch(seed=1000) draws, their scans
ray-cast as ranges), every scan given five segments of seeded odometry motion,
one process, bench.py's host-inputs loop (double-buffered pinned inputs: queue
batch i + 1, submit batch i) in three forms:

  host    csm_deskew_ranges over the batch on 16 threads inside the timed step,
          into the pinned buffer, then csm_load_ranges_async: what a caller
          could do before the device path existed
  device  csm_load_ranges_deskewed_async
  plain   csm_load_ranges_async of the raw ranges (no de-skew: other outputs;
          how far `device` sits above it is reported without a threshold)

The forms run interleaved (their order rotates every repeat), each warmed up
first; per form the median and max - min of the repeats' ms/step, the queueing
call's host cost, the de-skew kernel's HIP-event time for one batch and the
scans the host repaired per batch are reported; the last step's outputs of
`host` and `device` are compared byte for byte (and written to --out for cmp).
One JSON line on stdout; exit status 0 when the outputs are identical and
`device`'s median is at or below `host`'s.

  python tools/deskew_ab.py [--scans 4096] [--steps 30] [--repeats 5] [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))

SEGMENTS = 5
THREADS = 16


def odometry(rng, n_scans, n_beams):
    """Five segments a scan: 0.25-0.75 m/s, up to +-1.5 rad/s, 5 ms a segment, from a seeded start."""
    close = [((k + 1) * (n_beams - 1)) // SEGMENTS for k in range(SEGMENTS)]
    poses = np.empty((n_scans, SEGMENTS + 1, 3))
    poses[:, 0, 0:2] = rng.uniform(-3, 3, (n_scans, 2))
    poses[:, 0, 2] = rng.uniform(-3, 3, n_scans)
    v = rng.uniform(0.25, 0.75, n_scans)
    w = rng.uniform(-1.5, 1.5, n_scans)
    for k in range(SEGMENTS):
        yaw = poses[:, k, 2]
        poses[:, k + 1, 0] = poses[:, k, 0] + v * 0.005 * np.cos(yaw) + rng.normal(0, 1e-4, n_scans)
        poses[:, k + 1, 1] = poses[:, k, 1] + v * 0.005 * np.sin(yaw) + rng.normal(0, 1e-4, n_scans)
        poses[:, k + 1, 2] = yaw + w * 0.005 + rng.normal(0, 1e-4, n_scans)
    off = np.arange(n_scans + 1, dtype=np.int64) * SEGMENTS
    return off, np.array(close * n_scans, dtype=np.int32), np.ascontiguousarray(poses.reshape(-1, 3))


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
    from roborts_csm import _abi, worlds
    from roborts_csm.params import headline_levels

    lib = _abi.load_library()
    levels = headline_levels()
    world = worlds.make_world(2000, 2000, 0.05, seed=20261015)
    batch = worlds.make_scan_batch(world, args.scans, seed=1000)
    spec = worlds.LaserSpec()
    laser = spec.to_c()
    factor = 1 / world.resolution
    ranges = worlds.raycast_ranges(world, batch.true_poses, spec)
    n, nb = args.scans, spec.n_beams
    seg_off, seg_close, seg_poses = odometry(np.random.default_rng(20261019), n, nb)

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

    pin_raw = [roborts_csm.PinnedArray(ranges.shape, dtype=np.float32) for _ in range(2)]
    pin_dsk = [roborts_csm.PinnedArray(ranges.shape, dtype=np.float32) for _ in range(2)]
    for p in pin_raw:
        np.copyto(p.array, ranges)

    # csm_deskew_ranges over THREADS slices of the batch (ctypes releases the GIL)
    pool = ThreadPoolExecutor(THREADS)
    cuts = [n * t // THREADS for t in range(THREADS + 1)]

    def host_deskew(dst):
        def one(t):
            s0, s1 = cuts[t], cuts[t + 1]
            if s1 == s0:
                return 0
            so = np.ascontiguousarray(seg_off[s0:s1 + 1] - seg_off[s0])
            k0, k1 = int(seg_off[s0]), int(seg_off[s1])
            return lib.csm_deskew_ranges(C.byref(laser), s1 - s0, ranges[s0:s1].ctypes.data_as(_abi._f32p),
                                         so.ctypes.data_as(_abi._i64p),
                                         seg_close[k0:k1].ctypes.data_as(_abi._i32p),
                                         seg_poses[k0 + s0:k1 + s1].ctypes.data_as(_abi._dp),
                                         dst[s0:s1].ctypes.data_as(_abi._f32p))
        if any(pool.map(one, range(THREADS))):
            raise RuntimeError("csm_deskew_ranges failed")

    def queue_host(i):
        host_deskew(pin_dsk[i % 2].array)
        ctx.load_ranges_async(laser, pin_dsk[i % 2].array, factor)

    def queue_device(i):
        ctx.load_ranges_deskewed_async(laser, pin_raw[i % 2].array, factor, seg_off, seg_close, seg_poses)

    def queue_plain(i):
        ctx.load_ranges_async(laser, pin_raw[i % 2].array, factor)

    queues = {"host": queue_host, "device": queue_device, "plain": queue_plain}
    queue_s = {k: [] for k in queues}  # host time of each queueing call
    batches = {k: 0 for k in queues}

    def run(name, k):
        queue = queues[name]
        queue(0)
        batches[name] += 1
        res = None
        for i in range(k):
            if i + 1 < k:
                t = time.perf_counter()
                queue(i + 1)
                queue_s[name].append(time.perf_counter() - t)
                batches[name] += 1
            res = step()
        ctx.scan_matchers_wait()
        return tuple(np.array(a, copy=True) for a in res)

    def stat(name):
        return sum(s["launches"] for s in ctx.kernel_stats() if s["name"] == name)

    for name in queues:
        run(name, args.warmup)
    for k in queue_s:
        queue_s[k].clear()
    ms = {name: [] for name in queues}
    last = {}
    order = list(queues)
    repaired0, device_batches0 = stat("deskew:host_scans"), batches["device"]
    for rep in range(args.repeats):
        for name in order[rep % 3:] + order[:rep % 3]:
            t = time.perf_counter()
            last[name] = run(name, args.steps)
            ms[name].append((time.perf_counter() - t) / args.steps * 1e3)
    repaired = stat("deskew:host_scans") - repaired0
    device_batches = batches["device"] - device_batches0
    host_batches = stat("deskew:host_batches")

    # the de-skew kernel and the ingest kernels, HIP events, one batch; and the device's points against the host's
    ctx.set_profiling(1)
    ctx.load_ranges_deskewed(laser, pin_raw[0].array, factor, seg_off, seg_close, seg_poses)
    kernels = {s["name"]: s["total_ms"] / max(1, s["launches"]) for s in ctx.kernel_stats()
               if s["name"] == "deskew" or s["name"].startswith("ranges_")}
    ctx.set_profiling(0)
    back = ctx.loaded_scans()
    host_deskew(pin_dsk[0].array)
    want = roborts_csm.ranges_to_points(laser, pin_dsk[0].array, factor)
    device_points_equal_host = bool(np.array_equal(back[1], want[1]) and
                                    np.array_equal(back[0].view(np.uint64), want[0].view(np.uint64)))
    t = time.perf_counter()
    host_deskew(pin_dsk[0].array)
    host_deskew_ms = (time.perf_counter() - t) * 1e3

    same = all(x.tobytes() == y.tobytes() for x, y in zip(last["host"], last["device"]))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        for name, res in last.items():
            with open(os.path.join(args.out, f"outputs_{name}.bin"), "wb") as fh:
                for a in res:  # scores, poses, covs
                    fh.write(a.tobytes())

    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "tool": "deskew_ab",
        "scans": n, "beams": nb, "segments": SEGMENTS, "steps": args.steps, "repeats": args.repeats,
        "warmup": args.warmup, "host_threads": THREADS,
        "ms_per_step": {k: {"median": med[k], "spread_max_minus_min": max(v) - min(v), "runs": v}
                        for k, v in ms.items()},
        "queue_call_host_ms_median": {k: statistics.median(v) * 1e3 for k, v in queue_s.items() if v},
        "host_deskew_ms_one_batch_16_threads": host_deskew_ms,
        "kernel_ms_one_batch": kernels,
        "deskew_host_scans_per_batch": repaired / max(1, device_batches),
        "deskew_host_batches": host_batches,
        "device_outputs_equal_host": same,
        "device_points_equal_host": device_points_equal_host,
        "device_median_at_or_below_host": bool(med["device"] <= med["host"]),
        "device_above_plain_ms": med["device"] - med["plain"],
        "build": roborts_csm.build_digest(),
    }
    print(json.dumps(out))
    ctx.close()
    pool.shutdown()
    return 0 if same and device_points_equal_host and out["device_median_at_or_below_host"] else 1


if __name__ == "__main__":
    sys.exit(main())
