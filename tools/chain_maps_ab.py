"""A/B of the loop closure's submaps built from chains of kept scans, on one
MI355X: what a caller could do before csm_set_grid_stack_chains against it.

Shape (config 3's): --chains 512 chains of --chain-len 11 consecutive kept
scans of a willow drive (1081 beams a scan), maps of 300 x 300 cells at 0.08 m
centred on the drive's middle pose (ResetScanMatchMapWithRangeVec,
slam_processor.cpp:448-462), deviation 0.24 (25-cell splats), blur offset 0.72.
Both forms run in one process, interleaved (the order flips every repeat), each
warmed up first, and end with a device synchronise:

  gridmaps  512 resident csm_gridmap objects (made and Reset() once, outside the
            timing): per query csm_gridmap_set_map_offset and
            csm_gridmap_init_with_range_vec (speed-up reset) each, then
            csm_set_grid_stack_gridmaps. The scans' scaled points and the
            argument arrays are prepared outside the timing.
  chains    csm_set_grid_stack_chains over a resident csm_scan_store

Per form the repeats' ms per query, their median and max - min; the two stacks
must be identical. Reported without a gate: the fill and the splat by HIP
events (csm_set_profiling), the kernel cells the splat visits times 4 B over
its time beside the chip-wide rate of global float atomics (an upper bound of the bytes
raised: a visit that would not change its cell issues no atomic), the cells
the build raised, and `chains` followed by csm_search_gated against
the search alone on the resident stack. One JSON line on stdout, also written
to --out/chain_maps_ab.json with the two stacks (stack_gridmaps.bin,
stack_chains.bin, for cmp) when --out is given; exit status 0 when the stacks
are identical and `chains`' median is at or below `gridmaps`'.

  python tools/chain_maps_ab.py [--chains 512] [--repeats 5] [--warmup 1] [--out DIR]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))

ATOMIC_RATE_GBS = 1300.0  # chip-wide global float atomic rate of an MI355X, added bytes (about 1.3 TB/s)
RES, SIZE, DEV, BLUR_OFFSET, DEFAULT = 0.08, 300, 0.24, 0.72, 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=512)
    ap.add_argument("--chain-len", type=int, default=11)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=115, help="of the willow drive")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        print("note: fewer than 5 repeats: not a measurement", file=sys.stderr)

    import roborts_csm
    from roborts_csm import _abi, _lib, worlds
    from roborts_csm.chain_maps import ChainMapParam, ScanStore, grid_download, set_grid_stack_chains
    from roborts_csm.gridmap import OccuGridMap
    from roborts_csm.loop_closure import world_to_map
    from roborts_csm.params import CorrelationScanMatchParam

    hip = C.CDLL("libamdhip64.so")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            raise RuntimeError("hipDeviceSynchronize failed")

    n_chains, n_len = args.chains, args.chain_len
    n_scans = n_chains + n_len - 1
    # seed 115: a drive that stays inside the building (most seeds start in the open
    # space around it, where few beams return): 522 scans keep 994 to 1081 beams each
    drive = worlds.make_scan_stream(worlds.willow_world(), n_scans, seed=args.seed)
    scans, poses = drive.points_m, np.ascontiguousarray(drive.true_poses)
    kept = [s.shape[0] for s in scans]
    if min(kept) < 500:
        raise RuntimeError(f"the drive of seed {args.seed} leaves the building: a scan keeps {min(kept)} beams")
    chains = [list(range(g, g + n_len)) for g in range(n_chains)]
    cur = poses[n_scans // 2]
    cell = 1 / (1.0 / RES)
    map_offset = np.array([-(cur[0] - 0.5 * SIZE * cell), -(cur[1] - 0.5 * SIZE * cell)])

    ctx = roborts_csm.Context(args.device)
    dp, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    # ---- form (a): one csm_gridmap per chain ----
    maps, jobs = [], []
    for ch in chains:
        m = OccuGridMap(RES, (SIZE, SIZE), tuple(map_offset), DEV, DEFAULT, device=args.device)
        m.set_options(False, True, BLUR_OFFSET, 0.0)
        m.Reset()
        maps.append(m)
        pts = np.ascontiguousarray(np.concatenate([scans[i] * (1 / RES) for i in ch]))  # CreateFrom(raw, 1 / resolution)
        off = np.zeros(len(ch) + 1, dtype=np.int64)
        off[1:] = np.cumsum([scans[i].shape[0] for i in ch])
        jobs.append((pts, off, np.ascontiguousarray(poses[ch])))
    handles = (C.c_void_p * n_chains)(*[m.handle for m in maps])

    def gridmaps():
        for m, (pts, off, ps) in zip(maps, jobs):
            if _lib.csm_gridmap_set_map_offset(m.handle, map_offset[0], map_offset[1]) != 0 or \
               _lib.csm_gridmap_init_with_range_vec(m.handle, n_len, pts.ctypes.data_as(dp), off.ctypes.data_as(i64p),
                                                    None, ps.ctypes.data_as(dp), 1, 1) != 0:
                raise RuntimeError("csm_gridmap_init_with_range_vec failed")
        if _lib.csm_set_grid_stack_gridmaps(ctx._h, handles, n_chains) != 0:
            raise RuntimeError("csm_set_grid_stack_gridmaps failed")
        sync()

    # ---- form (b): the resident store and one call ----
    store = ScanStore(args.device)
    for s, q in zip(scans, poses):
        store.add(s, q)
    mp = ChainMapParam(RES, DEV, BLUR_OFFSET, SIZE, SIZE, default_cell_prob=DEFAULT).to_c()
    c_off = np.arange(0, n_chains * n_len + 1, n_len, dtype=np.int32)
    c_ids = np.ascontiguousarray([i for ch in chains for i in ch], dtype=np.int32)

    def chains_build():
        if _lib.csm_set_grid_stack_chains(ctx._h, store._h, C.byref(mp), n_chains, c_off.ctypes.data_as(i32p),
                                          c_ids.ctypes.data_as(i32p), map_offset.ctypes.data_as(dp), None) != 0:
            raise RuntimeError("csm_set_grid_stack_chains failed")

    def chains_form():
        chains_build()
        sync()

    def stack():
        return np.stack([grid_download(ctx, g, (SIZE, SIZE)) for g in range(n_chains)])

    forms = {"gridmaps": gridmaps, "chains": chains_form}
    got = {}
    for name, f in forms.items():
        for _ in range(max(1, args.warmup)):
            f()
        got[name] = stack()
    same = bool(np.array_equal(got["gridmaps"].view(np.uint32), got["chains"].view(np.uint32)))
    ms = {k: [] for k in forms}
    order = list(forms)
    for rep in range(args.repeats):
        for name in (order if rep % 2 == 0 else order[::-1]):
            t = time.perf_counter()
            forms[name]()
            ms[name].append((time.perf_counter() - t) * 1e3)

    # ---- the kernels by HIP events ----
    ctx.set_profiling(True)
    for _ in range(args.repeats):
        chains_form()
    stats = {s["name"]: s for s in ctx.kernel_stats() if s["name"].startswith("chain_maps:")}
    ctx.set_profiling(False)
    per = {k: v["total_ms"] / v["launches"] for k, v in stats.items()}
    visits = stats["chain_maps:splat"]["scorings"] / stats["chain_maps:splat"]["launches"]
    visited_gbs = visits * 4 / (per["chain_maps:splat"] * 1e-3) / 1e9
    fill_gbs = n_chains * SIZE * SIZE * 4 / (per["chain_maps:fill"] * 1e-3) / 1e9
    raised_cells = int((got["chains"] != np.float32(DEFAULT)).sum())

    # ---- the build followed by the gated search, against the search alone ----
    param = CorrelationScanMatchParam(16.0, RES, math.pi, 0.0349, 0.5, 100, 0, False, 0)
    query = scans[n_scans // 2] * (1 / RES)
    gi = np.arange(n_chains)
    centers = np.stack([world_to_map(cur, RES, map_offset)] * n_chains)
    chains_form()
    best = ctx.search_gated(query, param, gi, centers, -1.0)[1]
    gate = float(np.median(best))
    legs = {"search_alone": [], "chains_then_search": []}
    for rep in range(args.repeats + max(1, args.warmup)):
        for name in (list(legs) if rep % 2 == 0 else list(legs)[::-1]):
            t = time.perf_counter()
            if name == "chains_then_search":
                chains_build()
            n_pass = ctx.search_gated(query, param, gi, centers, gate)[6]
            if rep >= max(1, args.warmup):
                legs[name].append((time.perf_counter() - t) * 1e3)

    def summary(v):
        return {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}

    n_pts = sum(scans[i].shape[0] for ch in chains for i in ch)
    out = {
        "tool": "chain_maps_ab", "chains": n_chains, "chain_len": n_len, "kept_scans": n_scans,
        "points_drawn": n_pts, "beams_kept_per_scan": [min(kept), max(kept)], "seed": args.seed, "grid": [SIZE, SIZE], "resolution": RES, "deviation": DEV,
        "repeats": args.repeats, "warmup": max(1, args.warmup),
        "ms_per_query": {k: summary(v) for k, v in ms.items()},
        "stacks_identical": same,
        "chains_median_at_or_below_gridmaps": bool(statistics.median(ms["chains"]) <= statistics.median(ms["gridmaps"])),
        "stack_bytes": int(got["chains"].nbytes), "cells_raised": raised_cells,
        "kernel_ms": per, "fill_GBps": fill_gbs,
        "splat_cells_visited": visits, "splat_visited_GBps": visited_gbs, "atomic_rate_GBps": ATOMIC_RATE_GBS,
        "gate": gate, "gate_passes": int(n_pass),
        "search_ms": {k: summary(v) for k, v in legs.items()},
        "build": roborts_csm.build_digest(),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        got["gridmaps"].tofile(os.path.join(args.out, "stack_gridmaps.bin"))
        got["chains"].tofile(os.path.join(args.out, "stack_chains.bin"))
        with open(os.path.join(args.out, "chain_maps_ab.json"), "w") as fh:
            fh.write(line + "\n")
    store.close()
    ctx.close()
    for m in maps:
        m.close()
    return 0 if same and out["chains_median_at_or_below_gridmaps"] else 1


if __name__ == "__main__":
    sys.exit(main())
