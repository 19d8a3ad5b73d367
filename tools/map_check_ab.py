"""A/B of the map check for J poses: J calls of csm_gridmap_feedback_penalty
against one csm_gridmap_feedback_penalty_batch and one
csm_gridmap_feedback_penalty_store, on one MI355X.

Config 2's world (make_world(2000, 2000, 0.05, seed=20261015)); a 2000 x 2000
CountCell PubMap drawn with full lines from --build scans of a drive through
it; the sim YAML's check (check_point_num 100, bound_tolerance 2.5,
penalty_gain 0.015); scans of 1081 beams. Pose k checks scan k mod --scans at
that scan's pose moved by a seeded offset of up to +-0.3 m and +-0.1 rad. In
one process, interleaved (the order flips every repeat), each form warmed up
first, for J = 8 (the back end's job count), 256 (config 3's median gate) and
4096 (a config-2 batch):

  single  J calls of csm_gridmap_feedback_penalty, one after the other, on
          points scaled to cells beforehand (outside the timing)
  batch   one csm_gridmap_feedback_penalty_batch over the scans in metres
  store   one csm_gridmap_feedback_penalty_store over a resident store

Per form and J the median and max - min of the repeats' ms per J poses; the
three forms' coefficients must be identical (also written to --out for cmp).
The batch kernel alone by HIP events is reported without a gate. One JSON line
on stdout; exit status 0 when the coefficients are identical and, at every J,
`batch` and `store` have medians at or below `single`'s.

  python tools/map_check_ab.py [--build 64] [--scans 256] [--repeats 5] [--out DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))

SIZES = (8, 256, 4096)
CHECK = (100, 2.5, 0.015)  # config/simulatin_param.yaml


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", type=int, default=64, help="scans drawn into the PubMap")
    ap.add_argument("--scans", type=int, default=256, help="distinct scans the poses check")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="", help="folder for the forms' coefficients (.bin, for cmp)")
    args = ap.parse_args()
    if args.repeats < 5:
        print("note: fewer than 5 repeats: not a measurement", file=sys.stderr)

    import roborts_csm
    from roborts_csm import _abi, worlds
    from roborts_csm.chain_maps import ScanStore
    from roborts_csm.gridmap import COUNT_CELL, OccuGridMap

    lib = _abi.load_library()
    dp, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    res = 0.05
    world = worlds.make_world(2000, 2000, res, seed=20261015)
    stream = worlds.make_scan_stream(world, max(args.build, args.scans), seed=77, step_m=0.25)
    n_beams = int(stream.points_m[0].shape[0])
    pub = OccuGridMap(res, (world.size_x, world.size_y), world.offset, 0.0, 0.5, kind=COUNT_CELL, device=args.device)
    pub.set_options(True, False, 0.72, 0.2)
    pub.set_cell_params(0.3, 0.7, 0.2, 3.0)
    for k in range(args.build):
        pub.UpdateMapByRange(stream.points_m[k] * (1 / res), stream.true_poses[k])
    st = pub.state()
    store = ScanStore(args.device)
    for k in range(args.scans):
        store.add(stream.points_m[k], stream.true_poses[k])

    scans_m = [np.ascontiguousarray(stream.points_m[k], dtype=np.float64) for k in range(args.scans)]
    scans_c = [np.ascontiguousarray(s * (1 / res)) for s in scans_m]  # CreateFrom, outside the timing
    pts_m = np.ascontiguousarray(np.concatenate(scans_m))
    off = np.zeros(args.scans + 1, dtype=np.int64)
    off[1:] = np.cumsum([s.shape[0] for s in scans_m])
    prm = _abi.CsmMapCheckParam(CHECK[0], 0, 0, 0, CHECK[1], CHECK[2])
    rng = np.random.default_rng(5)
    results, same_all, pass_all = {}, True, True
    for J in SIZES:
        idx = (np.arange(J) % args.scans).astype(np.int32)
        poses = np.ascontiguousarray(stream.true_poses[idx] + rng.uniform(-1.0, 1.0, (J, 3)) * [0.3, 0.3, 0.1])
        coeff = {k: np.full(J, -1.0) for k in ("single", "batch", "store")}
        counts = np.zeros(J, dtype=np.int32)
        one = C.c_double(0.0)
        single_args = [(scans_c[i].ctypes.data_as(dp), scans_c[i].shape[0], poses[k:k + 1].ctypes.data_as(dp))
                       for k, i in enumerate(idx)]

        def single():
            out = coeff["single"]
            for k, (p, n, w) in enumerate(single_args):
                if lib.csm_gridmap_feedback_penalty(pub.handle, p, n, None, w, CHECK[0], CHECK[1], CHECK[2], 0,
                                                    C.byref(one)) != 0:
                    raise RuntimeError("csm_gridmap_feedback_penalty failed")
                out[k] = one.value

        def batch():
            if lib.csm_gridmap_feedback_penalty_batch(pub.handle, args.scans, pts_m.ctypes.data_as(dp),
                                                      off.ctypes.data_as(i64p), J, idx.ctypes.data_as(i32p),
                                                      poses.ctypes.data_as(dp), C.byref(prm),
                                                      coeff["batch"].ctypes.data_as(dp),
                                                      counts.ctypes.data_as(i32p)) != 0:
                raise RuntimeError("csm_gridmap_feedback_penalty_batch failed")

        def stored():
            if lib.csm_gridmap_feedback_penalty_store(pub.handle, store._h, J, idx.ctypes.data_as(i32p),
                                                      poses.ctypes.data_as(dp), C.byref(prm),
                                                      coeff["store"].ctypes.data_as(dp), None) != 0:
                raise RuntimeError("csm_gridmap_feedback_penalty_store failed")

        forms = {"single": single, "batch": batch, "store": stored}
        for f in forms.values():
            for _ in range(args.warmup):
                f()
        ms = {k: [] for k in forms}
        order = list(forms)
        for rep in range(args.repeats):
            for name in (order if rep % 2 == 0 else order[::-1]):
                t = time.perf_counter()
                forms[name]()
                ms[name].append((time.perf_counter() - t) * 1e3)
        same = bool(np.array_equal(coeff["single"].view(np.uint64), coeff["batch"].view(np.uint64)) and
                    np.array_equal(coeff["single"].view(np.uint64), coeff["store"].view(np.uint64)))
        kms = pub.feedback_penalty_store_kernel_ms(store, idx, poses, *CHECK, repeats=50)
        med = {k: statistics.median(v) for k, v in ms.items()}
        ok = med["batch"] <= med["single"] and med["store"] <= med["single"]
        same_all, pass_all = same_all and same, pass_all and ok
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            for k, v in coeff.items():
                v.tofile(os.path.join(args.out, f"coeff_{k}_{J}.bin"))
        results[str(J)] = {
            "ms": {k: {"median": med[k], "spread_max_minus_min": max(v) - min(v), "runs": v} for k, v in ms.items()},
            "coefficients_identical": same,
            "batch_and_store_at_or_below_single": bool(ok),
            "kernel_ms": kms,
            "counts": {"min": int(counts.min()), "median": float(np.median(counts)), "max": int(counts.max()),
                       "outside": int((counts < 0).sum())},
            "at_floor": int((coeff["batch"] == 0.1).sum()),
        }
    out = {
        "tool": "map_check_ab", "build_scans": args.build, "distinct_scans": args.scans, "beams": n_beams,
        "repeats": args.repeats, "warmup": args.warmup, "map": [st.size_x, st.size_y], "check": list(CHECK),
        "sizes": results, "coefficients_identical": same_all, "batch_and_store_at_or_below_single": pass_all,
        "build": roborts_csm.build_digest(),
    }
    print(json.dumps(out))
    store.close()
    pub.close()
    return 0 if same_all and pass_all else 1


if __name__ == "__main__":
    sys.exit(main())
