"""A/B of ScanMatchInterface's result for many chains, on one MI355X: what a
caller could do before csm_loop_closure_scan_match against it.

Shape (config 3's submaps): --chains chains of --chain-len consecutive kept
scans of a willow drive (1081 beams a scan), maps of 300 x 300 cells at 0.08 m
centred on the drive's middle pose (range_max 10 m: the back end's own size),
a coarse window of 1.2 m / +-pi/8 at one-cell steps, then
config/simulatin_param.yaml's fine and super-fine levels, the Gauss-Newton
matcher off, the map check on a CountCell PubMap of 0.05 m cells. The query is
the drive's middle scan, a kept scan of both forms.

  backend    csm_backend_scan_match with one job per chain (its batched path:
             per job two csm_gridmap rebuilds, a stack of the fine maps, the
             3-level driver from level 0, one batched map check)
  interface  csm_loop_closure_scan_match on a one-device handle, per query
             csm_loop_closure_set_submaps_chains and the call at a gate every
             chain passes

Both forms run in one process, interleaved (the order flips every repeat), each
warmed up first. Outputs (pose, covariance, score, penalty of every chain) are
compared on each form's first call: the back end's maps are fresh there (0.5
where nothing is drawn, which is what the handle's maps are drawn over here);
from its second call on, its speed-up reset has left 0.3 in the cells it
touched, and cells whose kernel value lies between the two differ. Reported
without a gate: the call alone on resident submaps, its level 0 alone
(csm_loop_closure_match_gated_full at the same gate), and the call at
interface_wide_gate(T) (csrc/csm_lc_interface.hpp) for a T between the best and
the second-best final score. One JSON line on stdout, also written to
--out/lc_interface_ab.json; exit status 0 when the outputs are identical and
the interface's median is at or below the back end's.

  python tools/lc_interface_ab.py [--chains 512] [--repeats 5] [--warmup 1] [--out DIR]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))

RES, SIZE, DEV, BLUR_OFFSET, BACKGROUND = 0.08, 300, 0.24, 0.72, 0.5
RANGE_MAX, MAP_RES, CHECK = 10.0, 0.05, (100, 2.5, 0.015)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=512)
    ap.add_argument("--chain-len", type=int, default=11)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=115, help="of the willow drive")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        print("note: fewer than 5 repeats: not a measurement", file=sys.stderr)

    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.backend import BackEndParam, ScanMatchService
    from roborts_csm.chain_maps import ChainMapParam
    from roborts_csm.gridmap import OccuGridMap
    from roborts_csm.loop_closure import DeviceLoopClosure
    from roborts_csm.params import SIM_YAML_LEVELS, CorrelationScanMatchParam

    n_chains, n_len = args.chains, args.chain_len
    n_scans = n_chains + n_len - 1
    drive = worlds.make_scan_stream(worlds.willow_world(), n_scans, seed=args.seed)
    scans, poses = drive.points_m, np.ascontiguousarray(drive.true_poses)
    chains = [list(range(g, g + n_len)) for g in range(n_chains)]
    q = n_scans // 2
    cur = poses[q]
    pose = cur + np.array([0.06, -0.04, 0.03])
    levels = (CorrelationScanMatchParam(1.2, RES, math.pi / 8, 0.0349, 0.5, 100, 0, False, 0), SIM_YAML_LEVELS[1],
              SIM_YAML_LEVELS[2])

    pub_size = (480, 480)
    pub = OccuGridMap(MAP_RES, pub_size, (-(cur[0] - 0.5 * pub_size[0] * MAP_RES), -(cur[1] - 0.5 * pub_size[1] * MAP_RES)),
                      0.0, 0.5, kind=1)
    pub.set_options(True, False, 0.72, 0.2)
    for k in (q - 5, q, q + 5):
        pub.UpdateMapByRange(scans[k] * (1 / MAP_RES), poses[k])

    prm = BackEndParam(range_max=RANGE_MAX, gaussian_blur_offset=BLUR_OFFSET, map_resolution=MAP_RES,
                       coarse_map_resolution=RES, coarse_map_deviation=DEV, fine_map_resolution=RES,
                       fine_map_deviation=DEV, use_map_check_feedback=True, map_check_point_num=CHECK[0],
                       map_check_bound_tolerance=CHECK[1], map_check_penalty_gain=CHECK[2], levels=levels,
                       use_optimize_scan_match=False)
    svc = ScanMatchService(prm)
    lc = DeviceLoopClosure([0])
    for s, p in zip(scans, poses):
        svc.AddRangeData(s, p)
        lc.add_scan(s, p)
    mp = ChainMapParam(RES, DEV, BLUR_OFFSET, SIZE, SIZE, default_cell_prob=BACKGROUND)
    queries, starts = [scans[q]] * n_chains, [pose] * n_chains

    def backend():
        return svc.scan_match_jobs(queries, chains, starts, cur, pub, True)

    def call(gate=-1.0):
        return lc.scan_match(pub, q, levels, pose, gate, n_chains, RANGE_MAX, check=CHECK)

    def interface():
        lc.set_submaps_chains(mp, chains, cur)
        return call()

    def rows_backend(r):
        return np.array([np.concatenate([j.pose, j.cov.reshape(9), [j.score, j.map_penalty]]) for j in r])

    def rows_interface(r):
        return np.array([np.concatenate([g["pose"], g["cov"].reshape(9), [g["score"], g["map_penalty"]]]) for g in r[0]])

    first = {"backend": rows_backend(backend()), "interface": rows_interface(interface())}
    same = first["backend"].shape == first["interface"].shape and bool(
        np.array_equal(first["backend"].view(np.uint64), first["interface"].view(np.uint64)))
    forms = {"backend": backend, "interface": interface}
    for f in forms.values():
        for _ in range(max(0, args.warmup - 1)):
            f()
    ms = {k: [] for k in forms}
    order = list(forms)
    for rep in range(args.repeats):
        for name in (order if rep % 2 == 0 else order[::-1]):
            t = time.perf_counter()
            forms[name]()
            ms[name].append((time.perf_counter() - t) * 1e3)

    # the call alone on resident submaps, and at the wide gate of a threshold between the two best scores
    got, _ = interface()
    final = sorted(g["score"] for g in got)
    T = 0.5 * (final[-1] + final[-2])
    gate = float(roborts_csm._lib.csm_loop_closure_wide_gate(T, 3))  # interface_wide_gate(T, 3)
    cells = scans[q] * (1 / RES)
    legs = {"call_resident": [], "call_wide_gate": [], "level0_gated_full": []}
    n_gate = 0
    for rep in range(args.repeats + 1):
        for name in (list(legs) if rep % 2 == 0 else list(legs)[::-1]):
            t = time.perf_counter()
            if name == "level0_gated_full":  # level 0 alone: the gate and one csm_search_match per passer
                covs = np.ascontiguousarray(np.tile(np.eye(3).reshape(9), (n_chains, 1)))
                r = lc.match_gated_full(cells, levels[0], pose, -1.0, n_chains, covs)
            else:
                r = call(gate if name == "call_wide_gate" else -1.0)
            if rep >= 1:
                legs[name].append((time.perf_counter() - t) * 1e3)
            if name == "call_wide_gate":
                n_gate = r[1]
                above = [g["submap"] for g in r[0] if g["score"] > T]
    kept = [g["submap"] for g in got if g["score"] > T]

    def summary(v):
        return {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v), "runs": v}

    out = {
        "tool": "lc_interface_ab", "chains": n_chains, "chain_len": n_len, "kept_scans": n_scans, "seed": args.seed,
        "grid": [SIZE, SIZE], "resolution": RES, "repeats": args.repeats, "warmup": max(1, args.warmup),
        "ms_per_query": {k: summary(v) for k, v in ms.items()},
        "outputs_identical_on_first_call": same,
        "interface_median_at_or_below_backend": bool(statistics.median(ms["interface"]) <= statistics.median(ms["backend"])),
        "call_ms": {k: summary(v) for k, v in legs.items()},
        "threshold_T": T, "wide_gate": gate, "wide_gate_passes": int(n_gate),
        "above_T_at_wide_gate": above, "above_T_ungated": kept, "wide_gate_lost_nothing": above == kept,
        "final_score_range": [final[0], final[-1]],
        "build": roborts_csm.build_digest(),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "lc_interface_ab.json"), "w") as fh:
            fh.write(line + "\n")
    lc.close()
    svc.close()
    pub.close()
    return 0 if same and out["interface_median_at_or_below_backend"] else 1


if __name__ == "__main__":
    sys.exit(main())
