"""A/B of the Gauss-Newton matcher's two forms: the host
loop, one round trip per iteration (csm_optimize_scan_match_batch), against
the whole solve in one launch (csm_optimize_scan_match_batch_grids).

One process, both forms interleaved (their order swaps every repeat), each
warmed up first, on the 64 ray-cast scans at 2000 x 2000 of
tests/test_optimize.py's batch test (SIM_YAML_OPTIMIZE: 10 iterations at most)
and on its first scan alone. Per form the median and max - min of the
repeats' ms per call; the results of the two forms are compared byte for byte.
The single-scan pair gives the per-iteration round trip the host loop pays:
(host loop - one launch) / (iterations - 1).

With --backend-trees PARENT BRANCH (two checkouts with built libraries) it also
times csm_backend_scan_match with 8 jobs and the Gauss-Newton matcher on, one
child process per tree and repeat, alternating; pass when the branch's median
is not above the parent's by more than the parent's own max - min (DESIGN.md
section 11 item 7).

One JSON line on stdout, the same as markdown with --md; exit status 0 when
the results are identical, the batch's one-launch median is at or below the
host loop's and the back-end rule (when run) holds.

  python tools/optimize_ab.py [--calls 200] [--repeats 5] [--md FILE] [--backend-trees PARENT BRANCH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKEND_JOBS = 8


def backend_child(tree, calls, warmup):
    """ms per csm_backend_scan_match call (8 jobs, Gauss-Newton on) with the library of `tree`."""
    sys.path.insert(0, os.path.join(tree, "roborts-edu-slam_amd"))
    from roborts_csm import worlds
    from roborts_csm.backend import BackEndParam, ScanMatchService
    from roborts_csm.params import PARAM_CONFIG_OPTIMIZE
    n_scans = 48
    w = worlds.make_world(400, 400, 0.05, seed=8)
    st = worlds.make_scan_stream(w, n_scans, seed=9)
    rng = np.random.default_rng(10)
    kept = st.true_poses + rng.normal(size=st.true_poses.shape) * [0.01, 0.01, 0.003]
    d = np.array([0.06, -0.04, 0.03])
    jobs = [(47 - j, list(range(36 - j, 46 - j)), st.true_poses[47 - j] + (d if j % 2 else -d))
            for j in range(BACKEND_JOBS)]
    svc = ScanMatchService(BackEndParam(use_optimize_scan_match=True, optimize=PARAM_CONFIG_OPTIMIZE,
                                        optimize_failed_cost=20.0))
    for k in range(n_scans):
        svc.AddRangeData(st.points_m[k], kept[k])
    q, c, p = [st.points_m[a] for a, _, _ in jobs], [b for _, b, _ in jobs], [x for _, _, x in jobs]
    cur = st.true_poses[-1]
    res = None
    for _ in range(warmup):
        res = svc.scan_match_jobs(q, c, p, cur)
    t = time.perf_counter()
    for _ in range(calls):
        res = svc.scan_match_jobs(q, c, p, cur)
    ms = (time.perf_counter() - t) / calls * 1e3
    digest = np.concatenate([np.concatenate([r.pose, r.cov.reshape(-1), [r.score, r.optimize_cost]]) for r in res])
    svc.close()
    print(json.dumps({"ms_per_call": ms, "results": digest.tobytes().hex()}))
    return 0


def backend_ab(parent, branch, repeats, calls, warmup):
    runs = {"parent": [], "branch": []}
    results = {}
    trees = {"parent": parent, "branch": branch}
    for rep in range(repeats):
        for name in (("parent", "branch") if rep % 2 == 0 else ("branch", "parent")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--backend-child", trees[name], "--calls",
                                str(calls), "--warmup", str(warmup)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"back-end child ({name}) failed: {r.stderr[-2000:]}")
            o = json.loads(r.stdout.strip().splitlines()[-1])
            runs[name].append(o["ms_per_call"])
            results[name] = o["results"]
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = max(runs["parent"]) - min(runs["parent"])
    return {"jobs": BACKEND_JOBS, "calls": calls, "repeats": repeats,
            "ms_per_call": {k: {"median": med[k], "spread_max_minus_min": max(v) - min(v), "runs": v}
                            for k, v in runs.items()},
            "results_equal_parent": results["parent"] == results["branch"],
            "pass": bool(med["branch"] <= med["parent"] + spread)}


def markdown(o):
    L = ["# Gauss-Newton matcher: host loop against one launch", "",
         f"`tools/optimize_ab.py`, build `{o['build']}`. One process, forms interleaved, {o['repeats']} repeats of "
         f"{o['calls']} calls after {o['warmup']} warm-up calls each. ms per call.", "",
         "| case | scans | iterations (max) | host loop median | host loop max - min | one launch median | "
         "one launch max - min | same bytes |", "|---|---|---|---|---|---|---|---|"]
    for name, c in o["cases"].items():
        a, b = c["ms_per_call"]["host_loop"], c["ms_per_call"]["one_launch"]
        L.append(f"| {name} | {c['scans']} | {c['iterations_max']} | {a['median']:.4f} | "
                 f"{a['spread_max_minus_min']:.4f} | {b['median']:.4f} | {b['spread_max_minus_min']:.4f} | "
                 f"{c['results_equal']} |")
    L += ["", f"Pass (batch: one launch at or below the host loop, no margin): **{o['batch_one_launch_at_or_below']}**.",
          "", f"Single scan: {o['cases']['single']['iterations_max']} iterations; the host loop pays "
          f"**{o['round_trip_ms_per_iteration']:.4f} ms per iteration** more than the loop inside the kernel "
          "((host loop - one launch) / (iterations - 1)): the copy up, launch, copy down and synchronize of one "
          "iteration.", "", f"Kernel time by HIP events, one 64-scan call: {json.dumps(o['kernel_ms_one_call'])}."]
    if "backend" in o:
        be = o["backend"]
        p, b = be["ms_per_call"]["parent"], be["ms_per_call"]["branch"]
        L += ["", "## csm_backend_scan_match, 8 jobs, Gauss-Newton on", "",
              f"Parent library against this one, one process per run, alternating, {be['repeats']} runs of "
              f"{be['calls']} calls each. ms per call.", "",
              "| library | median | max - min | runs |", "|---|---|---|---|",
              f"| parent | {p['median']:.3f} | {p['spread_max_minus_min']:.3f} | "
              f"{', '.join(f'{v:.3f}' for v in p['runs'])} |",
              f"| branch | {b['median']:.3f} | {b['spread_max_minus_min']:.3f} | "
              f"{', '.join(f'{v:.3f}' for v in b['runs'])} |", "",
              f"Results equal the parent's byte for byte: {be['results_equal_parent']}. Pass (branch median not above "
              f"the parent's by more than the parent's max - min): **{be['pass']}**."]
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--md", default="", help="also write the result as markdown")
    ap.add_argument("--backend-trees", nargs=2, metavar=("PARENT", "BRANCH"), default=None)
    ap.add_argument("--backend-calls", type=int, default=20)
    ap.add_argument("--backend-child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.backend_child:
        return backend_child(args.backend_child, args.calls, args.warmup)

    sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))
    import roborts_csm
    from roborts_csm import worlds
    from roborts_csm.params import SIM_YAML_OPTIMIZE as PRM

    w = worlds.make_world(2000, 2000, 0.05, seed=11)
    b = worlds.make_scan_batch(w, 64, seed=12)
    ctx = roborts_csm.Context(args.device)
    ctx.set_grid(roborts_csm.ScanMatchMap(w.grid, w.resolution, w.offset, 0, 1))
    shapes = {"batch": (b.points_cells, b.offsets, b.init_poses),
              "single": (b.points_cells[:b.offsets[1]], b.offsets[:2], b.init_poses[:1])}

    def host_loop(pts, off, init):
        poses = np.ascontiguousarray(init).copy()
        return (*ctx.optimize_scan_match_batch(pts, off, PRM, poses), poses)

    def one_launch(pts, off, init):
        poses = np.ascontiguousarray(init).copy()
        return (*ctx.optimize_scan_match_batch_grids(pts, off, None, PRM, poses), poses)

    forms = {"host_loop": host_loop, "one_launch": one_launch}
    cases = {}
    for cname, shape in shapes.items():
        last = {}
        for f in forms.values():
            for _ in range(args.warmup):
                f(*shape)
        ms = {k: [] for k in forms}
        for rep in range(args.repeats):
            for name in (("host_loop", "one_launch") if rep % 2 == 0 else ("one_launch", "host_loop")):
                t = time.perf_counter()
                for _ in range(args.calls):
                    last[name] = forms[name](*shape)
                ms[name].append((time.perf_counter() - t) / args.calls * 1e3)
        same = all(x.tobytes() == y.tobytes() for x, y in zip(last["host_loop"], last["one_launch"]))
        cases[cname] = {"scans": len(shape[1]) - 1, "iterations_max": int(last["one_launch"][1].max()),
                        "ms_per_call": {k: {"median": statistics.median(v), "spread_max_minus_min": max(v) - min(v),
                                            "runs": v} for k, v in ms.items()},
                        "results_equal": same}
    ctx.set_profiling(1)
    for f in forms.values():
        f(*shapes["batch"])
    kernels = {s["name"]: {"launches": s["launches"], "total_ms": s["total_ms"]} for s in ctx.kernel_stats()
               if s["name"].startswith("optimize")}
    ctx.set_profiling(0)
    single = cases["single"]
    med = {k: {f: c["ms_per_call"][f]["median"] for f in forms} for k, c in cases.items()}
    out = {"tool": "optimize_ab", "calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "cases": cases,
           "kernel_ms_one_call": kernels,
           "batch_one_launch_at_or_below": bool(med["batch"]["one_launch"] <= med["batch"]["host_loop"]),
           "round_trip_ms_per_iteration": (med["single"]["host_loop"] - med["single"]["one_launch"]) /
           max(1, single["iterations_max"] - 1),
           "build": roborts_csm.build_digest()}
    ctx.close()
    ok = out["batch_one_launch_at_or_below"] and all(c["results_equal"] for c in cases.values())
    if args.backend_trees:
        out["backend"] = backend_ab(*args.backend_trees, args.repeats, args.backend_calls, 3)
        ok = ok and out["backend"]["pass"] and out["backend"]["results_equal_parent"]
    print(json.dumps(out))
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(markdown(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
