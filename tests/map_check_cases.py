"""Shared cases of the batched map check's tests (test infrastructure): the
scans of map_scenarios in metres and in cells, the 24 checked poses and the
three parameter sets, and the Python restatement of one MapCheckPenalize call
with its count (map_pyref.PyMap.penalty returns the coefficient alone)."""
from __future__ import annotations

import math

import numpy as np

import map_scenarios as S

# (check_point_num, bound_tolerance, penalty_gain): the two of count_lines' penalty ops
# (the first is config/simulatin_param.yaml's) and prob_reset_speedup's
PARAMS = [(50, 2.5, 0.015), (100, 1.0, 0.05), (30, 2.0, 0.05)]
N_SCANS = 4


def scans():
    """(scans in metres, the same scans in cells of 0.05 m, their poses):
    make_scans(res=1.0) multiplies by 1 / 1.0, so the metres are the raw points
    and metres * (1 / 0.05) is make_scans()'s own product, bit for bit."""
    scans_m, poses = S.make_scans(N_SCANS, res=1.0)
    return scans_m, [s * (1 / 0.05) for s in scans_m], poses


def check_poses(poses, n_extra=20, seed=5):
    """24 poses: the four scan poses exact, then n_extra seeded perturbations
    of up to +-1 m and +-1.5 rad around them in turn -> (poses [24, 3], the
    scan each one checks)."""
    rng = np.random.default_rng(seed)
    out = [np.array(p, dtype=np.float64) for p in poses]
    idx = list(range(len(poses)))
    for k in range(n_extra):
        b = k % len(poses)
        d = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(-1.5, 1.5)])
        out.append(np.asarray(poses[b], dtype=np.float64) + d)
        idx.append(b)
    return np.array(out), np.array(idx, dtype=np.int32)


def logistic(c: float) -> float:
    """MapCheckPenalize's logistic (slam_processor.cpp:590)."""
    return 1 / (1 + math.exp(-10 * (c - 0.4)))


def count_of(coeff: float, gain: float, n_max: int) -> int:
    """The count a coefficient above the floor stands for: the k <= n_max with
    max(1 + 2 gain - k gain, 0.1) == coeff (the first, so a floored
    coefficient gives the smallest count that reaches the floor)."""
    for k in range(n_max + 1):
        pen = float(k) * gain
        if max(1.0 + 2 * gain - pen, 0.1) == coeff:
            return k
    raise AssertionError((coeff, gain))
