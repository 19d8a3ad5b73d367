"""GPU: a context owns what it allocates (csrc/csm_resources.hpp): eight
cycles of create, use, destroy in one process, each leaving its resources in
the states csm_destroy has to cope with, and every cycle's answers equal to
the first cycle's and to the oracle's, bit for bit.

A cycle: 4 parts in flight over a 64-scan batch (CSM_PIPELINE=16,
CSM_PIPELINE_PARTS=4: every alternate launch slot is swapped in), profiling on
(all ten events of every slot exist), five host grids through csm_set_grid (one
slot evicted, three parked), one csm_search_windows call, one csm_gridmap grown
through ExtendSize and destroyed, and at csm_destroy one submitted batch still
pending and one csm_load_ranges_async batch queued and never taken.

No free-memory assertion: hipMemGetInfo is device-wide and the device may be
shared."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

CYCLES = 8
N_SCANS = 64


@pytest.fixture(scope="module")
def scene():
    """A 600 x 600 world at 5 cm, 64 scans on it with the oracle's 3-level
    answers, the five grids of a cycle (the world's last: the match runs on
    it), and 8 scans' raw ranges."""
    from roborts_csm import worlds
    from roborts_csm.params import headline_levels
    w = worlds.make_world(600, 600, 0.05, seed=20261015)
    b = worlds.make_scan_batch(w, N_SCANS, seed=17)
    grids = [np.ascontiguousarray(np.roll(w.grid, 13 * s, axis=0)) for s in (1, 2, 3, 4)] + [w.grid]
    spec = worlds.LaserSpec()
    true = worlds.sample_free_poses(w, 8, np.random.default_rng(5))
    ranges = np.ascontiguousarray(worlds.raycast_ranges(w, true, spec), dtype=np.float32)
    O.set_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    try:
        want = O.scan_matchers_batch(O.Map(w.grid, w.resolution, w.offset), b.points_cells, b.offsets,
                                     headline_levels(), b.init_poses, _eye(N_SCANS))
    finally:
        O.set_threads(1)
    return w, b, grids, spec.to_c(), ranges, want


def _eye(n):
    return np.tile(np.eye(3).reshape(1, 9), (n, 1))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cycle(scene):
    """One context's life. Returns the synchronous match, the batch that was
    pending at csm_destroy, the search's answer and the grown map's cells."""
    import roborts_csm
    from roborts_csm import gridmap
    from roborts_csm.loop_closure import world_to_map
    from roborts_csm.params import CorrelationScanMatchParam, headline_levels
    w, b, grids, laser, ranges, _ = scene
    env = {"CSM_PIPELINE": "16", "CSM_PIPELINE_PARTS": "4"}
    os.environ.update(env)
    try:
        c = roborts_csm.Context(0)
    finally:
        for k in env:
            del os.environ[k]
    pin = roborts_csm.PinnedArray(ranges.shape, dtype=np.float32)
    try:
        c.set_profiling(True)
        for g in grids:  # the fifth evicts the first; the three between stay parked
            c.set_grid(roborts_csm.ScanMatchMap(g, w.resolution, w.offset, 0, 1))
        poses, covs = np.ascontiguousarray(b.init_poses.copy()), _eye(N_SCANS)
        s = c.scan_matchers_batch(b.points_cells, b.offsets, headline_levels(), poses, covs)
        stats = {k["name"]: k["launches"] for k in c.kernel_stats()}
        assert stats["host:wait"] == 3 * 4 and stats["grid:upload"] == 5  # 3 levels x 4 parts; five grids
        sync = (s, poses, covs)

        pts0 = b.points_cells[b.offsets[0]:b.offsets[1]]
        p = CorrelationScanMatchParam(3.0, 0.05, math.pi / 4, 0.0349, 0.5, 1081, 0, False, 0)
        center = world_to_map(b.init_poses[0], w.resolution, w.offset)
        best, win, st = c.search_windows(pts0, p, [0], center.reshape(1, 3))
        ex = c.best_window(pts0, p, center)
        assert win == 0 and not st["exhaustive"] and (best.score, best.flat_index) == (ex.score, ex.flat_index)
        search = (best.score, best.flat_index, best.x, best.y, best.angle)

        m = gridmap.OccuGridMap(0.05, (100, 100), (2.5, 2.5), 0.0, 0.3)
        assert not m.UpdateBound((-40.0, -40.0), (140.0, 140.0))  # outside the map: ExtendSize
        size = (m.GetSizeX(), m.GetSizeY())
        assert size[0] > 180 and size[1] > 180
        prob = m.cells()[0]
        assert prob.shape == size[::-1]
        h, m._h = m._h, None
        assert gridmap._lib.csm_gridmap_destroy(h) == 0

        # left for csm_destroy: a submitted batch pending, a queued batch never taken
        c.load_scans(b.points_cells, b.offsets)
        pend = (np.zeros(N_SCANS), np.ascontiguousarray(b.init_poses.copy()), _eye(N_SCANS))
        c.scan_matchers_submit(headline_levels(), pend[1], pend[2], pend[0])
        np.copyto(pin.array, ranges)
        c.load_ranges_async(laser, pin.array, 1 / w.resolution)
    except BaseException:
        c.close()
        pin.close()
        raise
    h, c._h = c._h, None
    assert roborts_csm._lib.csm_destroy(h) == 0  # completes the pending batch into `pend`
    pin.close()
    return sync, pend, search, prob


def test_create_use_destroy_cycles(scene):
    want = scene[5]
    first = None
    for k in range(CYCLES):
        sync, pend, search, prob = _cycle(scene)
        for a, e in zip(sync, want):
            assert np.array_equal(_bits(a), _bits(e)), ("synchronous call against the oracle", k)
        for a, e in zip(pend, want):
            assert np.array_equal(_bits(a), _bits(e)), ("batch pending at csm_destroy against the oracle", k)
        if first is None:
            first = (sync, search, prob)
        for a, e in zip(sync, first[0]):
            assert np.array_equal(_bits(a), _bits(e)), ("cycle against cycle 0", k)
        assert search == first[1] and np.array_equal(prob, first[2]), k
