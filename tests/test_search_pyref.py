"""The restated search bounds (tests/search_pyref.py) against the CPU oracle.

tests/test_gpu_search_bounds.py pins the device's bounds to the restatement
bit for bit; here the restatement itself is checked: every restated bound is
at least the oracle's score of every candidate under the node, and on a
one-beam scan it is exactly the best of the node's (2^d + 1)^2 cells, rounded
as the levels round.
"""
import numpy as np
import pytest

import pyoracle as O
import search_pyref as R
from roborts_csm.params import CorrelationScanMatchParam

RES = 0.05
MRES = 1.0 / (1.0 / RES)


def _param(ns, half_angle, penalty, use=100):
    return CorrelationScanMatchParam((ns - 1) * RES, RES, half_angle, 0.0349, 0.5, use, 0, penalty, 0)


def _block_max(sc, na, ns, d):
    """Best candidate score under every top node, [angle, K, J]."""
    sh = 1 << d
    nj = (ns + sh - 1) >> d
    pad = np.full((na, nj * sh, nj * sh), -np.inf)
    pad[:, :ns, :ns] = sc.reshape(na, ns, ns)                 # (theta, x, y)
    m = pad.reshape(na, nj, sh, nj, sh).max(axis=(2, 4))      # [a, J, K]
    return m.transpose(0, 2, 1)


@pytest.fixture(scope="module")
def small():
    g = R.scene(29, 23, seed=11)
    rng = np.random.default_rng(12)
    pts = np.concatenate([rng.uniform(-9.0, 9.0, (11, 2)), [[0.0, 0.0], [3.0, -2.0], [-4.5, 2.5]]])
    return g, pts


def test_fixed_point_is_exact_and_refuses_wide_values():
    g = np.array([[0.0, 0.25], [0.5 + 2.0 ** -20, 1.0]], dtype=np.float32)
    gi, E, oi = R.fixed_point(g, 0.75)
    assert E == 20 and oi == 3 << 18
    assert gi.tolist() == [[-(3 << 18), -(1 << 19)], [1 - (1 << 18), 1 << 18]]
    assert R.fixed_point(np.zeros((2, 2), np.float32), 0.0)[1] == 0
    with pytest.raises(R.Unsupported):
        R.fixed_point(np.array([[2.0 ** -20, 64.0]], dtype=np.float32), 0.0)
    # the largest accepted magnitude: |v| + |outside| = (2^26 - 1) 2^-20
    gi, E, _ = R.fixed_point(np.array([[3 * 2.0 ** -20]], dtype=np.float32), -(2.0 ** 26 - 4) * 2.0 ** -20)
    assert E == 20 and gi[0, 0] == 2 ** 26 - 1


def test_pooled_level_brute_force_by_hand():
    gi = np.array([[0, 5000, -3], [-4097, -9000, 1]], dtype=np.int64)
    lv = R.pooled_level(gi, 1)
    assert lv.shape == (4, 5)
    # anchor (-2, -2) sees only the corner cell and off-grid zeros
    assert lv[0, 0] == 0
    # anchor (0, 1): rows 1..3, columns 0..2 -> max(-4097, -9000, 1, off-grid 0) = 1 -> ceil = 1
    assert lv[1 + 2, 0 + 2] == 1
    # anchor (1, 0): columns 1..3 (3 off the grid: 0), rows 0..2 -> 5000 -> ceil(5000 / 4096) = 2
    assert lv[0 + 2, 1 + 2] == 2
    assert R.ceil_quant(-4097) == -1 and R.ceil_quant(-4096) == -1 and R.ceil_quant(-4095) == 0
    assert R.ceil_quant(4096) == 1 and R.ceil_quant(4097) == 2


@pytest.mark.parametrize("outside", [0.3, 0.75])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_restated_bounds_dominate_oracle_scores(small, d, outside):
    """Every node's restated bound >= the oracle's score of every candidate
    under it, penalty off and on; windows inside the grid, hanging off its low
    corner and off its high corner."""
    g, pts = small
    ns, half = 13, 0.06
    centers = np.array([[14.0, 11.5, 0.2], [2.25, -1.0, -0.4], [27.0 - 2.0 ** -21, 24.5, 0.06]])
    for penalty in (False, True):
        p = _param(ns, half, penalty, use=7)
        for gidx in (0, 1):
            _, b = R.top_bounds(g, outside, pts, p, [gidx] * 3, centers, MRES, d)
            win = R.Window(pts, p, centers[0], MRES, d)
            b = b.reshape(3, win.na, win.nj, win.nj)
            m = O.Map(g[gidx], RES, (0.0, 0.0), outside=outside)
            for w in range(3):
                sc = O.score_window(m, pts, p, centers[w], win.na * ns * ns)
                assert np.all(b[w] >= _block_max(sc, win.na, ns, d))


@pytest.mark.parametrize("outside", [0.3, 0.75])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_one_beam_bound_is_the_best_pooled_cell(small, d, outside):
    """One beam at the origin, one angle, candidates at t >= 0 (so their cells
    are consecutive): the unpenalised bound of node (J, K) is the maximum over
    j in [J 2^d, J 2^d + 2^d], k likewise, of the candidate's score taken up to
    the level's lattice: (2^12 ceil((s - outside) 2^E / 2^12) + outside_i) 2^-E.
    Candidates inside the window come from the oracle; past its end the cell
    the candidate would read is taken from the grid directly."""
    g, _ = small
    pts = np.zeros((1, 2))
    ns = 21
    sh = 1 << d
    for gidx in (0, 1):
        gi, E, oi = R.fixed_point(g[gidx], outside)
        H, W = gi.shape
        for center in ([12.25, 11.0, 0.0], [22.0, 16.5, 0.0]):   # the second hangs off the high corner
            p = _param(ns, 0.0, False)
            win = R.Window(pts, p, center, MRES, d)
            assert win.na == 1 and win.use == 1 and win.xs[0] + 0.5 >= 0.0 and win.ys[0] + 0.5 >= 0.0
            _, b = R.top_bounds(g[gidx], outside, pts, p, [0], [center], MRES, d)
            b = b.reshape(win.nj, win.nj)
            m = O.Map(g[gidx], RES, (0.0, 0.0), outside=outside)
            sc = O.score_window(m, pts, p, center, ns * ns).reshape(ns, ns)   # (x, y)
            o64 = float(np.float32(outside))

            def lifted(s):
                f = (s - o64) * 2.0 ** E
                assert f == int(f)
                return float(R.ceil_quant(int(f)) * 4096 + oi) * 2.0 ** -E

            xs = win.xs[0] + np.arange(ns + sh + 1) * 1.0
            ys = win.ys[0] + np.arange(ns + sh + 1) * 1.0
            for K in range(win.nj):
                for J in range(win.nj):
                    best = -np.inf
                    for k in range(K * sh, K * sh + sh + 1):
                        for j in range(J * sh, J * sh + sh + 1):
                            if j < ns and k < ns:
                                s = sc[j, k]
                            else:
                                cx, cy = int(np.trunc(xs[j] + 0.5)), int(np.trunc(ys[k] + 0.5))
                                s = float(g[gidx][cy, cx]) if (0 <= cx < W and 0 <= cy < H) else o64
                            best = max(best, lifted(s))
                    assert b[K, J] == best, (d, gidx, center, K, J)
