"""The finish's writers on the GPU after the rules moved to
csrc/csm_finish_rules.hpp: the separate fast pass in its 1024-thread form (8
scans on the few-window path, 48 through the 3-level driver) and its 256 /
128-thread forms (80 scans, above kFinishWideWindows), the fused fast pass
inside the scoring kernels (80 scans of 109 beams, at most 512 summed), the
exact pass behind each of them, and the host's std::sort. Each case runs the
three sim levels (every beam summed) over a 300 x 300 map whose left half is
a blurred field on a 2^-12 lattice (distinct scores: the fast finish settles
the window) and whose right half holds one draw from {0.3, 0.5, 0.7, 1.0} per
column (a window there holds its best score more than once: the exact pass
takes it), with poses on both halves, and must equal the oracle bit for bit
(response, pose, covariance through scan_matchers_batch; argmax, response,
pose and covariance of every level through scan_match_batch) and a
CSM_FINISH=host and a CSM_FINISH=exact context. kernel_stats() names the
finish that ran, and in every level 0 < exact windows < windows, so neither
decision goes untested (the few-window path reports no such counts).

Inputs picked on the CPU with tools/tie_reasons.classify over the oracle's
scores along the 3-level chain (cap 512 for the separate pass, 128 for the
fused one); the windows it sends to the exact pass are stated at CASES below.
On the device the levels counted 24 / 26 / 12 of 48, 40 / 42 / 14 of 80 and,
fused, 40 / 47 / 42 of 80 (its caps are 128 per set, classify's positional
cap is looser)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

RES, OFFSET = 0.05, (7.5, 7.5)
SEED = 20261019
# case: (scans, beams, the fast finish kernel_stats() must name). classify's windows for the exact pass per
# level (coarse, fine, super-fine), left half + right half:
#   few_1024      8 scans:  0 + 4 of 8, 0 + 4 of 8, 0 + 1 of 8. At most 32 windows take the few-window path
#                 (split kernel, launch_finish's 1024-thread form); it reports no finish:* counts, so the
#                 case checks the results and the kernels' names only.
#   driver_1024   48 scans, one launch of at most kFinishWideWindows = 64 windows: the 1024-thread form through
#                 the 3-level driver, with its counts (the first 48 of the 80 below).
#   wide_256_128  80 scans: 0 + 40, 2 + 40, 3 + 11 of 80 (cap 512).
#   fused         80 scans of 109 beams: 0 + 40, 0 + 40, 5 + 13 of 80 (cap 128).
CASES = {
    "few_1024": (8, 600, None),
    "driver_1024": (48, 600, "separate"),
    "wide_256_128": (80, 600, "separate"),
    "fused": (80, 109, "fused"),
}


def levels():
    from roborts_csm.params import SIM_YAML_LEVELS
    return [lv.with_(use_point_size=1081) for lv in SIM_YAML_LEVELS]  # every beam of these scans


def make_grid():
    rng = np.random.default_rng(SEED)
    f = rng.random((300, 300))
    for _ in range(2):  # a 3 x 3 box blur, twice
        f = sum(np.roll(np.roll(f, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    f = 0.2 + 0.8 * (f - f.min()) / (f.max() - f.min())
    g = (np.round(f * 4096.0) / 4096.0).astype(np.float32)
    # one draw per column: a window there scores alike along y, so its best score is held more than once
    # (a draw per cell gave sums of 109 or 600 cells that hardly ever repeat: no window for the exact pass)
    g[:, 150:] = rng.choice(np.array([0.3, 0.5, 0.7, 1.0], dtype=np.float32), size=150)[None, :]
    return g


def make_batch(n_scans, beams):
    """n_scans scans of `beams` points (the first `beams` of 600: the same scans at either length),
    poses alternating between the map's halves, at least 5 cells of margin to the seam."""
    rng = np.random.default_rng(SEED + 1)
    pts = rng.uniform(-40.0, 40.0, size=(80, 600, 2))[:n_scans, :beams]
    x = rng.uniform(2.6, 4.5, size=80) * np.where(np.arange(80) % 2 == 0, -1.0, 1.0)
    init = np.stack([x, rng.uniform(-4.0, 4.0, size=80), rng.uniform(-1.0, 1.0, size=80)], axis=1)[:n_scans]
    off = np.arange(n_scans + 1, dtype=np.int64) * beams
    return np.ascontiguousarray(pts.reshape(-1, 2)), off, np.ascontiguousarray(init)


@pytest.fixture(scope="module")
def grid():
    O.set_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    yield make_grid()
    O.set_threads(1)


def _context(g, mode):
    import roborts_csm
    if mode:
        os.environ["CSM_FINISH"] = mode
    try:
        c = roborts_csm.Context(0)
    finally:
        os.environ.pop("CSM_FINISH", None)
    c.set_grid(roborts_csm.ScanMatchMap(g, RES, OFFSET, 0, 1), force=True)
    return c


def _chain(c, pts, off, init):
    """The 3-level driver: (scores, poses, covariances)."""
    poses = np.ascontiguousarray(init.copy())
    covs = np.tile(np.eye(3).reshape(1, 9), (init.shape[0], 1))
    s = c.scan_matchers_batch(pts, off, levels(), poses, covs)
    return s, poses, covs


def _per_level(c, pts, off, init):
    """Each level on its own from the initial poses: (responses, argmax, poses, covariances) per level."""
    out = []
    for lv in levels():
        poses = np.ascontiguousarray(init.copy())
        covs = np.tile(np.eye(3).reshape(1, 9), (init.shape[0], 1))
        r, am = c.scan_match_batch(pts, off, lv, poses, covs)
        out.append((r, am, poses, covs))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_every_finish_writer_equals_the_oracle(grid, case):
    n_scans, beams, fast = CASES[case]
    pts, off, init = make_batch(n_scans, beams)
    m = O.Map(grid, RES, OFFSET)
    eye = np.tile(np.eye(3).reshape(1, 9), (n_scans, 1))
    want = O.scan_matchers_batch(m, pts, off, levels(), init, eye)
    want_lv = []
    for lv in levels():
        rows = [O.scan_match(m, pts[off[k]:off[k + 1]], lv, init[k], np.eye(3)) for k in range(n_scans)]
        want_lv.append((np.array([r[0] for r in rows]), np.array([r[3] for r in rows]),
                        np.stack([r[1] for r in rows]), np.stack([np.asarray(r[2]).reshape(9) for r in rows])))
    ctxs = [_context(grid, mode) for mode in (None, "host", "exact")]
    try:
        ctxs[0].set_profiling(True)
        got = [_chain(c, pts, off, init) for c in ctxs]
        st = {k["name"]: k for k in ctxs[0].kernel_stats()}
        ctxs[0].set_profiling(False)
        got_lv = [_per_level(c, pts, off, init) for c in ctxs]
    finally:
        for c in ctxs:
            c.close()
    for mode, g3, gl in zip(("device", "host", "exact"), got, got_lv):
        for a, e, nm in zip(g3, want, ("scores", "poses", "covariances")):
            assert np.array_equal(a, e), (case, mode, nm)
        for l, (a, e) in enumerate(zip(gl, want_lv)):
            for x, y, nm in zip(a, e, ("response", "argmax", "pose", "covariance")):
                assert np.array_equal(np.asarray(x).reshape(np.asarray(y).shape), y), (case, mode, l, nm)
    # which fast finish ran, and both of its decisions in every level
    if fast is None:  # the few-window path: the split kernel, then launch_finish (16 waves a window)
        assert any(n.startswith("score_split_kernel<") for n in st), sorted(st)
        assert all(f"finish_kernel<{n}>" in st for n in (5070, 1331, 189)), sorted(st)
        return
    for n_cand in (30 * 13 * 13, 11 * 11 * 11, 21 * 3 * 3):
        ran = [w for w in ("fused", "separate") if f"finish:{w}<{n_cand}>" in st]
        print(case, n_cand, ran, st.get(f"finish:exact_windows<{n_cand}>"))
        assert ran == [fast], (case, n_cand, ran)
        ex = st[f"finish:exact_windows<{n_cand}>"]
        assert 0 < ex["scorings"] < ex["algorithmic_bytes"], (case, n_cand, ex)
