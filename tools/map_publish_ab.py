"""A/B of the map publisher's OccupancyGrid: the cell planes downloaded and
classified on the host against csm_gridmap_occupancy_grid (DESIGN.md section
11), on one MI355X.

A PubMap of config 5's size is built by an online drive (bench.py's online
world, make_world(2000, 2000, 0.05, seed=20261015), --build scans through the
device front end). Then, in one process, interleaved (the order flips every
repeat), each form warmed up first:

  download  csm_gridmap_download of `prob` + `pass_count` (whole planes of the
            allocated map, 8 B a cell) and the numpy classification of the
            bound box: what a caller could do before the device path existed
  device    csm_gridmap_occupancy_grid: the states kernel, one device-to-host
            copy of 1 B a cell of the box, a memcpy

Per form the median and max - min of the repeats' ms per call; the two grids
must be identical. Reported without a gate: the states kernel alone by HIP
events with the bytes it must move (9 B a cell of the box for CountCell) over
that time as a share of the HBM peak; the host time of the _begin call (how
long the front end can be blocked); and csm_frontend_process's latency for
scans during which a publish ran in a second thread against scans during which
none did. One JSON line on stdout; exit status 0 when the grids are identical
and `device`'s median is at or below `download`'s.

  python tools/map_publish_ab.py [--build 300] [--calls 50] [--repeats 5] [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, GB/s


def classify_box(prob, pas, size_x, box, thr, mp, out):
    """The node's loop (roborts_slam_node.cpp:444-469) in numpy over the
    downloaded planes: CountCell GetGridStates (grid_map_cell.h:125-136) at the
    linear index y * size_x + x, -1 outside the array."""
    sx, sy, w, h = box
    size_y = prob.shape[0]
    if sx >= 0 and sy >= 0 and sx + w <= size_x and sy + h <= size_y:
        v, p = prob[sy:sy + h, sx:sx + w], pas[sy:sy + h, sx:sx + w]
        np.copyto(out, np.where(p >= mp, np.where(v < thr, 0, 100), -1))
        return out
    x = sx + np.arange(w, dtype=np.int64)[None, :]
    y = sy + np.arange(h, dtype=np.int64)[:, None]
    lin = y * size_x + x
    ok = (x >= 0) & (y >= 0) & (lin < prob.size)
    lin = np.where(ok, lin, 0)
    v, p = prob.ravel()[lin], pas.ravel()[lin]
    np.copyto(out, np.where(ok & (p >= mp), np.where(v < thr, 0, 100), -1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", type=int, default=300, help="scans of the drive that builds the map")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--latency-scans", type=int, default=200)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="folder for the two grids (.bin, for cmp)")
    args = ap.parse_args()
    if args.calls < 50 or args.repeats < 5:
        print("note: fewer than 5 repeats of 50 calls: not a measurement", file=sys.stderr)

    import roborts_csm
    from roborts_csm import _abi, worlds
    from roborts_csm.frontend import FrontEndParam, SlamFrontEnd

    lib = _abi.load_library()
    prm = FrontEndParam()
    world = worlds.make_world(2000, 2000, 0.05, seed=20261015)
    stream = worlds.make_scan_stream(world, args.build + args.latency_scans, seed=77)
    fe = SlamFrontEnd(prm, device=args.device)
    for k in range(args.build):
        fe.process(stream.points_m[k], stream.odom_poses[k])
    pub = fe.map(SlamFrontEnd.PUB_MAP)
    st = pub.state()
    info = pub.OccupancyGridInfo()
    box = (info.start_x, info.start_y, info.width, info.height)
    n = info.width * info.height
    thr, mp = np.float32(prm.map_occu_threshold), np.float32(prm.map_min_passthrough)

    prob = np.empty((st.size_y, st.size_x), dtype=np.float32)
    pas = np.empty_like(prob)
    grid_a = np.empty((info.height, info.width), dtype=np.int8)
    grid_b = np.empty((info.height, info.width), dtype=np.int8)
    info_b = _abi.CsmOccupancyGridInfo()

    def download():
        if lib.csm_gridmap_download(pub.handle, prob.ctypes.data, pas.ctypes.data, None, None, None) != 0:
            raise RuntimeError("csm_gridmap_download failed")
        classify_box(prob, pas, st.size_x, box, thr, mp, grid_a)

    def device():
        if lib.csm_gridmap_occupancy_grid(pub.handle, 0, C.byref(info_b), grid_b.ctypes.data, n) != 0:
            raise RuntimeError("csm_gridmap_occupancy_grid failed")

    forms = {"download": download, "device": device}
    for f in forms.values():
        for _ in range(args.warmup):
            f()
    ms = {k: [] for k in forms}
    order = list(forms)
    for rep in range(args.repeats):
        for name in (order if rep % 2 == 0 else order[::-1]):
            f = forms[name]
            t = time.perf_counter()
            for _ in range(args.calls):
                f()
            ms[name].append((time.perf_counter() - t) / args.calls * 1e3)
    same = bool(np.array_equal(grid_a, grid_b)) and \
        (info_b.start_x, info_b.start_y, info_b.width, info_b.height) == box
    states = {str(v): int((grid_b == v).sum()) for v in (-1, 0, 100)}
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        grid_a.tofile(os.path.join(args.out, "grid_download.bin"))
        grid_b.tofile(os.path.join(args.out, "grid_device.bin"))

    # the kernel alone, HIP events around 200 launches
    kms = C.c_double(0.0)
    if lib.csm_gridmap_occupancy_grid_kernel_ms(pub.handle, 0, 200, C.byref(kms)) != 0:
        raise RuntimeError("csm_gridmap_occupancy_grid_kernel_ms failed")
    kernel_bytes = 9 * n
    kernel_gbs = kernel_bytes / (kms.value * 1e-3) / 1e9

    # the _begin call's host time (the front end can be blocked for this long), _end's wait after it
    begin_ms, end_ms = [], []
    p = C.c_void_p()
    for _ in range(200):
        t0 = time.perf_counter()
        lib.csm_gridmap_occupancy_grid_begin(pub.handle, 0, C.byref(info_b))
        t1 = time.perf_counter()
        lib.csm_gridmap_occupancy_grid_end(pub.handle, C.byref(p))
        t2 = time.perf_counter()
        begin_ms.append((t1 - t0) * 1e3)
        end_ms.append((t2 - t1) * 1e3)

    # csm_frontend_process beside a publisher thread: every other scan, a publish starts with the scan
    go, done, quit_ = threading.Event(), threading.Event(), threading.Event()

    def publisher():
        while True:
            go.wait()
            go.clear()
            if quit_.is_set():
                return
            fe.publish_map(-1)
            done.set()

    th = threading.Thread(target=publisher, daemon=True)
    th.start()
    lat = {"publishing": [], "alone": []}
    for i in range(args.latency_scans):
        k = args.build + i
        with_pub = i % 2 == 1
        if with_pub:
            done.clear()
            go.set()
        t = time.perf_counter()
        fe.process(stream.points_m[k], stream.odom_poses[k])
        lat["publishing" if with_pub else "alone"].append((time.perf_counter() - t) * 1e3)
        if with_pub:
            done.wait()
    quit_.set()
    go.set()
    th.join(timeout=30)

    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {
        "tool": "map_publish_ab",
        "build_scans": args.build, "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup,
        "map": [st.size_x, st.size_y], "box": list(box), "states": states,
        "bytes_download": 8 * st.size_x * st.size_y, "bytes_device": n,
        "ms_per_call": {k: {"median": med[k], "spread_max_minus_min": max(v) - min(v), "runs": v}
                        for k, v in ms.items()},
        "grids_identical": same,
        "device_median_at_or_below_download": bool(med["device"] <= med["download"]),
        "kernel_ms": kms.value, "kernel_bytes": kernel_bytes, "kernel_GBps": kernel_gbs,
        "kernel_share_of_hbm_peak": kernel_gbs / HBM_PEAK_GBS, "hbm_peak_GBps": HBM_PEAK_GBS,
        "begin_call_host_ms": {"median": statistics.median(begin_ms), "p99": float(np.percentile(begin_ms, 99)),
                               "max": max(begin_ms)},
        "end_call_wait_ms_median": statistics.median(end_ms),
        "process_latency_ms": {k: {"median": statistics.median(v), "p95": float(np.percentile(v, 95)),
                                   "max": max(v), "scans": len(v)} for k, v in lat.items()},
        "build": roborts_csm.build_digest(),
    }
    print(json.dumps(out))
    fe.close()
    return 0 if same and out["device_median_at_or_below_download"] else 1


if __name__ == "__main__":
    sys.exit(main())
