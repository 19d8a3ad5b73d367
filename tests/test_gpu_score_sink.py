"""What the scoring kernels' shared epilogue decides (csrc/csm_score_sink.hpp),
family by family: every score stored in all mode, the (max, lowest flat index
among equals) pair in best mode, and the lane max / NaN flag the fused finish
takes over, against the CPU oracle bit for bit.

Windows: the shipped sim levels (30 x 13^2 one-cell step, 11^2 at 0.4 cell, 3^2
super-fine), the only shapes that reach every family, at both beam rules, on
400 x 400 grids. Two grids: four random values, and one constant value on which
(penalty off) every score of a window is equal, so the tie rule alone picks
flat index 0. The column kernel also takes a grid that is not exactly summable
(values over many binades), which its fp64 form scores.

Not reached here or anywhere: a NaN score in a fused family (the sink's NaN
flag). The divisor is at least 1, fixed-point sums are finite, and non-finite
grids or points go to the fp64 column kernel, so no input produces one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402


def _map(grid, res, off):
    import roborts_csm
    return roborts_csm.ScanMatchMap(grid, float(res), tuple(off), 0, 0)


def _context(env):
    """A context of one kernel family, single windows through the throughput kernels (CSM_SMALL=0)."""
    import roborts_csm
    env = dict(env, CSM_SMALL="0")
    assert not any(k.startswith("CSM_") for k in os.environ)
    os.environ.update(env)
    try:
        return roborts_csm.Context(0)
    finally:
        for k in env:
            del os.environ[k]


# context -> the kernels its three levels must run (a stats name's head; "all" and "best" of each)
FAMILIES = {
    "v2": ({"CSM_KERNEL": "v2"}, ["score_cols_kernel<"]),
    "v4": ({"CSM_KERNEL": "v4"}, ["score_rowsd_kernel<13,", "score_rowsd_kernel<11,", "score_rowsd_kernel<3,"]),
    "v6": ({"CSM_KERNEL": "v6"}, ["score_box_kernel<13,", "score_rowsd_kernel<11,", "score_rowsd_kernel<3,"]),
    "v7": ({"CSM_KERNEL": "v7"}, ["score_box_kernel<13,", "score_phase_kernel<11,", "score_rowsd_kernel<3,"]),
    "v8": ({"CSM_KERNEL": "v8"}, ["score_box_kernel<13,", "score_phase_kernel<11,", "score_tiny_kernel<3,"]),
    "default": ({}, ["score_box_pair_kernel<13,", "score_phase_kernel<11,", "score_tiny_kernel<3,"]),
    "v8_gridi": ({"CSM_KERNEL": "v8", "CSM_PHASE_STRIPS": "0"},
                 ["score_box_kernel<13,", "score_phase_kernel<11,", "score_tiny_kernel<3,"]),
}


@pytest.fixture(scope="module")
def f1(golden_dir):
    return np.load(os.path.join(golden_dir, "f1_config1.npz"))


def _levels(penalty=None):
    from roborts_csm.params import SIM_YAML_LEVELS
    lv = list(SIM_YAML_LEVELS) + [l.with_(use_point_size=1081) for l in SIM_YAML_LEVELS]
    return lv if penalty is None else [l.with_(use_center_penalty=penalty) for l in lv]


@pytest.fixture(scope="module")
def cases(f1):
    """Per grid kind: the grid, the scan, the window centre and, per level, the
    oracle's scores and best, computed once. The constant grid's scan is f1's
    shrunk to 150 cells around the grid's middle: no candidate's beam leaves
    the grid (the outside value would break the tie)."""
    import roborts_csm
    from roborts_csm import worlds
    rng = np.random.default_rng(23)
    pts, cen = f1["points"], f1["center"]
    near = np.ascontiguousarray(pts * (150.0 / np.abs(pts).max()))
    mid = np.array([200.3, 199.6, cen[2]])
    grids = {"values4": (rng.choice(np.array([0.3, 0.41, 0.88, 1.0], dtype=np.float32), size=(400, 400)), pts, cen,
                         _levels()),
             "constant": (np.full((400, 400), 0.88, dtype=np.float32), near, mid, _levels(penalty=False)),
             "hostile": (worlds.hostile_grid(400, 400), pts, cen, _levels())}
    out = {}
    for kind, (g, q, c, levels) in grids.items():
        m = O.Map(g, float(f1["resolution"]), tuple(f1["offset"]))
        rows = []
        for p in levels:
            na, ns = roborts_csm.window_dims(p)
            want = O.score_window(m, q, p, c, na * ns * ns)
            want.setflags(write=False)
            rows.append((p, want, O.best_window(m, q, p, c)))
        out[kind] = (g, q, c, rows)
    return out


def _check(c, pts, cen, rows, what, constant=False):
    for p, want, (bs, bflat) in rows:
        if constant:  # the tie case is really exercised: every score of the window is the same
            assert np.all(want == want[0]) and bflat == 0, (what, p)
        sc = c.score_window(pts, p, cen)
        assert np.array_equal(sc, want), (what, p, np.flatnonzero(sc != want)[:8])
        got = c.best_window(pts, p, cen)
        assert (got.score, got.flat_index) == (bs, bflat), (what, p)
        # the wave's and the window's reduction agree with this context's own stored scores
        assert (got.score, got.flat_index) == (sc.max(), int(np.argmax(sc))), (what, p)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_sink_all_and_best(f1, cases, family):
    env, kernels = FAMILIES[family]
    c = _context(env)
    try:
        c.set_profiling(True)
        for kind in ("values4", "constant") + (("hostile",) if family == "v2" else ()):
            g, pts, cen, rows = cases[kind]
            c.set_grid(_map(g, f1["resolution"], f1["offset"]), force=True)
            _check(c, pts, cen, rows, (family, kind), constant=kind == "constant")
        names = {k["name"] for k in c.kernel_stats() if k["name"].startswith("score_")}
    finally:
        c.close()
    for head in kernels:
        for mode in ("all>", "best>"):
            assert any(n.startswith(head) and n.endswith(mode) for n in names), (family, head, mode, sorted(names))
    if family == "v2":  # the fp64 column kernel (the hostile grid) as well as the fixed-point one
        for sums in (",int,", ",f64,"):
            for mode in ("all>", "best>"):
                assert any(n.startswith("score_cols_kernel<") and sums in n and n.endswith(mode) for n in names), \
                    (sums, mode, sorted(names))


N_SCANS = 33  # the smallest batch that leaves the few-window path


@pytest.fixture(scope="module")
def batch_world():
    from roborts_csm import worlds
    w = worlds.make_world(400, 400, 0.05)
    b = worlds.make_scan_batch(w, N_SCANS, seed=41, min_points=600)
    return w, b


@pytest.mark.parametrize("beams,finish", [(109, "fused"), (513, "separate")])
def test_sink_fused_and_separate_finish(batch_world, beams, finish):
    """33 scans through the 3-level driver, finished inside the scoring launches
    (109 beams) and by the separate fast pass (513, one past the fused finish's
    limit and under the phase kernel's 576-beam segment). Penalty off, and scan
    7 starts far off the grid, where every beam reads the outside value: all of
    its windows' scores are equal, the degenerate case of the lane max."""
    import roborts_csm
    from roborts_csm.params import headline_levels
    w, b = batch_world
    scans = []
    for k in range(N_SCANS):
        p = b.points_cells[b.offsets[k]:b.offsets[k + 1]]
        assert p.shape[0] >= beams
        q = p[::p.shape[0] // beams][:beams]
        assert q.shape[0] == beams
        scans.append(q)
    pts = np.ascontiguousarray(np.concatenate(scans, axis=0))
    off = np.arange(N_SCANS + 1, dtype=np.int64) * beams
    init = np.ascontiguousarray(b.init_poses.copy())
    init[7, :2] = (-60.0, -45.0)
    levels = [l.with_(use_center_penalty=False) for l in headline_levels()]
    eye = np.tile(np.eye(3).reshape(1, 9), (N_SCANS, 1))
    m = O.Map(w.grid, w.resolution, w.offset)
    want = O.scan_matchers_batch(m, pts, off, levels, init, eye.copy())
    lv0 = levels[0]
    na, ns = roborts_csm.window_dims(lv0)
    cen = O.world_to_map(m, init[7])
    sc7 = O.score_window(m, scans[7], lv0, np.array([cen[0], cen[1], init[7, 2]]), na * ns * ns)
    assert np.all(sc7 == sc7[0])  # the off-grid window's scores are equal
    assert not any(k.startswith("CSM_") for k in os.environ)
    c = roborts_csm.Context(0)
    try:
        c.set_grid(roborts_csm.ScanMatchMap(np.asarray(w.grid, dtype=np.float32), float(w.resolution),
                                            tuple(w.offset), 0, 1))
        c.set_profiling(True)
        poses, covs = init.copy(), eye.copy()
        s = c.scan_matchers_batch(pts, off, levels, poses, covs)
        st = {k["name"]: k for k in c.kernel_stats()}
    finally:
        c.close()
    for a, e, nm in zip((s, poses, covs), want, ("scores", "poses", "covariances")):
        bad = np.flatnonzero(np.any(np.atleast_2d(a.T != e.T), axis=0))
        assert np.array_equal(a, e), (beams, nm, bad[:8].tolist())
    fused = sum(k["launches"] for n, k in st.items() if n.startswith("finish:fused<"))
    sep = sum(k["launches"] for n, k in st.items() if n.startswith("finish:separate<"))
    assert (fused > 0, sep > 0) == (finish == "fused", finish == "separate"), (fused, sep, sorted(st))
