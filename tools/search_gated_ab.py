#!/usr/bin/env python3
"""A/B of the gated search on config 3's shape (one GPU): bench.py's
loop-closure workload as it builds it -- 1 query scan, its stack of submaps
(800 x 800), its window (181 x 321^2 candidates per submap).

  a  csm_best_windows, every candidate of every window scored, plus the host
     filter by score >= gate: the only single call to the same answer before
     csm_search_gated
  b  csm_search_gated
  c  csm_search_windows (the best submap only), for scale

Interleaved in one process, `--repeats` each after `--warmup`. Two gates, both
computed from (a)'s own per-window bests:

  T_one   the midpoint between the best and the second-best window's best
  T_half  the median of the bests

(b)'s windows, scores, flats and poses are compared with (a)'s filtered ones
bit for bit. The pass rule: identical outputs, and (b) at T_one at or below
(a)'s median time -- no margin. T_half and (c) are reported. Writes
OUT/search_gated.json and OUT/speed.md.

  python3 tools/search_gated_ab.py --out profiles/search_gated [--submaps 512]

--resources BEFORE.s AFTER.s (no GPU): OUT/kernel_resources.md from two
assembly listings of csm_pyramid.hip (`make asm` on the parent commit and on
this one) and, with --select-asm, csm_select.hip's: registers, LDS, scratch and
code size of pyr_collect_kernel before and after, and of the two new kernels.
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "roborts-edu-slam_amd"), ROOT]


def _ms(ts):
    return round(statistics.median(ts) * 1e3, 4)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def kernel_resources(path):
    """{kernel name: figures} from a device-only assembly listing."""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", s, re.S):
        d = {}
        for k in ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
                  "private_segment_fixed_size"):
            mm = re.search(r"\.amdhsa_%s (\S+)" % k, m.group(2))
            d[k] = mm.group(1) if mm else "-"
        out[m.group(1)] = d
    for m in re.finditer(r"\n(\S+):\s*; @\1\n(.*?; Occupancy: \d+)", s, re.S):
        d = out.setdefault(m.group(1), {})
        for k in ("codeLenInByte", "TotalNumSgprs", "NumVgprs", "ScratchSize", "LDSByteSize", "Occupancy"):
            mm = re.search(r"; %s[:=] *(\d+)" % k, m.group(2).replace(" = ", "="))
            d[k] = mm.group(1) if mm else "-"
    return out


def write_resources(args):
    before, after = args.resources
    rows = []

    def pick(path, needle, label):
        for name, d in kernel_resources(path).items():
            if needle in name:
                rows.append((label, d))
    pick(before, "pyr_collect_kernel", "pyr_collect_kernel, parent")
    pick(after, "pyr_collect_kernel", "pyr_collect_kernel, this commit")
    pick(after, "pyr_gate_kernel", "pyr_gate_kernel")
    if args.select_asm:
        pick(args.select_asm, "gate_window_best_kernel", "gate_window_best_kernel")
        pick(args.select_asm, "gate_init_kernel", "gate_init_kernel")
    keys = ["NumVgprs", "TotalNumSgprs", "next_free_vgpr", "next_free_sgpr", "accum_offset", "LDSByteSize",
            "ScratchSize", "Occupancy", "codeLenInByte"]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "kernel_resources.md"), "w") as fh:
        fh.write("# Gated search: kernel resources (gfx950, `make asm`)\n\n")
        fh.write("Static LDS is 0 for all of them: the beams are staged in dynamic LDS, 16 bytes a beam, as\n"
                 "pyr_bound_kernel's. pyr_collect_kernel now calls the leaf walk it shares with pyr_gate_kernel;\n"
                 "its figures must not move.\n\n")
        fh.write("| kernel | " + " | ".join(keys) + " |\n|---|" + "---|" * len(keys) + "\n")
        for label, d in rows:
            fh.write(f"| {label} | " + " | ".join(str(d.get(k, "-")) for k in keys) + " |\n")
        fixed = ["NumVgprs", "TotalNumSgprs", "next_free_vgpr", "next_free_sgpr", "accum_offset", "LDSByteSize",
                 "ScratchSize", "Occupancy"]
        same = len(rows) >= 2 and all(rows[0][1].get(k) == rows[1][1].get(k) for k in fixed)
        fh.write(f"\npyr_collect_kernel: registers, LDS, scratch and occupancy unchanged: **{same}**; code length "
                 f"{rows[0][1].get('codeLenInByte')} -> {rows[1][1].get('codeLenInByte')} bytes (the same "
                 "instructions' schedule around the inlined walk; csm_search_match is timed against the parent in "
                 "speed.md).\n")
    print(open(os.path.join(args.out, "kernel_resources.md")).read())
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/search_gated")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--submaps", type=int, default=512)
    ap.add_argument("--resources", nargs=2, metavar=("BEFORE.s", "AFTER.s"))
    ap.add_argument("--select-asm", default="")
    args = ap.parse_args()
    if args.resources:
        sys.exit(write_resources(args))
    os.makedirs(args.out, exist_ok=True)
    import bench
    import roborts_csm
    from roborts_csm.loop_closure import worlds_to_map
    _, stack, pts, pose, offsets, param, res = bench._lc_config3(args.submaps)
    centers = worlds_to_map(pose, res, offsets)
    gi = np.arange(args.submaps, dtype=np.int32)
    times = {"a": [], "b_one": [], "b_half": [], "c": []}
    same = True
    info = {}
    with roborts_csm.Context(0) as ctx:
        ctx.set_grid_stack(stack, res, version=1)
        sc = ctx.best_windows(pts, param, gi, centers)[0]  # also builds nothing the forms share but the grid
        top = np.sort(sc)[::-1]
        gates = {"one": float(0.5 * (top[0] + top[1])), "half": float(np.median(sc))}
        for k in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            truth = ctx.best_windows(pts, param, gi, centers)
            keep = {g: np.nonzero(truth[0] >= T)[0] for g, T in gates.items()}
            t1 = time.perf_counter()
            got = {}
            tb = {}
            for g, T in gates.items():
                t2 = time.perf_counter()
                got[g] = ctx.search_gated(pts, param, gi, centers, T)
                tb[g] = time.perf_counter() - t2
            t3 = time.perf_counter()
            b, w, _ = ctx.search_windows(pts, param, gi, centers)
            t4 = time.perf_counter()
            if k >= args.warmup:
                times["a"].append(t1 - t0)
                times["b_one"].append(tb["one"])
                times["b_half"].append(tb["half"])
                times["c"].append(t4 - t3)
            for g in gates:
                wins, gs, gf, gx, gy, ga, n, st = got[g]
                kk = keep[g]
                same &= bool(n == kk.size and np.array_equal(wins, kk) and np.array_equal(gf, truth[1][kk]) and
                             np.array_equal(_bits(gs), _bits(truth[0][kk])) and
                             np.array_equal(_bits(gx), _bits(truth[2][kk])) and
                             np.array_equal(_bits(gy), _bits(truth[3][kk])) and
                             np.array_equal(_bits(ga), _bits(truth[4][kk])))
                info[g] = dict(gate=gates[g], n_pass=int(n), path=st["path"], descents=st["descents"],
                               listed=st["listed"], nodes=st["nodes"], candidates=st["candidates"], depth=st["depth"])
            same &= bool(w == int(np.argmax(truth[0])))
    med = {k: _ms(v) for k, v in times.items()}
    line = dict(workload="config3", submaps=args.submaps, repeats=args.repeats, median_ms=med,
                all_ms={k: [round(t * 1e3, 3) for t in v] for k, v in times.items()},
                max_minus_min_ms={k: round((max(v) - min(v)) * 1e3, 4) for k, v in times.items()},
                gates=info, outputs_identical=bool(same), passes=bool(same and med["b_one"] <= med["a"]),
                library=roborts_csm.build_digest())
    print(json.dumps(line), flush=True)
    with open(os.path.join(args.out, "search_gated.json"), "w") as fh:
        json.dump(line, fh, indent=1)
    with open(os.path.join(args.out, "speed.md"), "a" if os.path.exists(os.path.join(args.out, "speed.md")) else "w") as fh:
        fh.write(f"\n## tools/search_gated_ab.py, config 3's shape, {args.submaps} submaps, library {line['library']}\n\n")
        fh.write("| form | median ms | max - min ms | runs (ms) |\n|---|---|---|---|\n")
        names = {"a": "(a) csm_best_windows + host filter", "b_one": "(b) csm_search_gated at T_one",
                 "b_half": "(b) csm_search_gated at T_half", "c": "(c) csm_search_windows"}
        for k, nm in names.items():
            fh.write(f"| {nm} | {med[k]} | {line['max_minus_min_ms'][k]} | {line['all_ms'][k]} |\n")
        for g, d in info.items():
            fh.write(f"\nT_{g} = {d['gate']!r}: {d['n_pass']} of {args.submaps} windows pass, path {d['path']}, "
                     f"{d['descents']} descent(s), {d['listed']} listed, depth {d['depth']}, "
                     f"leaves scored {d['nodes'][0]} of {d['candidates']} candidates.\n")
        fh.write(f"\nOutputs identical to (a)'s filter: **{same}**. Gate ((b) at T_one <= (a)): "
                 f"**{'pass' if line['passes'] else 'FAIL'}**.\n")
    sys.exit(0 if line["passes"] else 1)


if __name__ == "__main__":
    main()
