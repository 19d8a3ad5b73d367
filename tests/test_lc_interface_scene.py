"""The scene of tests/test_gpu_lc_interface.py (tests/lc_interface_ref.py), checked on the CPU
with the oracle alone: no back-end map grows at the chosen numbers, the maps the oracle matches
on are the chain maps drawn over 0.5 but for cell (0, 0), the cases the GPU tests rely on are
there (distinct bests to gate between, a wide level that is accepted and one that is not, poses
that move). No GPU."""
import numpy as np

import chain_maps_ref as R
import lc_interface_ref as L


def test_scene_numbers_and_oracle_maps():
    scans, poses, chains, map_offset = L.scene()
    assert int((L.RANGE_MAX + 2.0) * 2 / R.RES) == L.SIZE  # the back end's own size
    assert L.levels()[0].search_space_size <= 2.0
    pose = poses[-1] + L.DELTA
    grids = []
    want = L.truth(L.levels(), pose, grids=grids)  # asserts that no map grew
    dev, off = R.BLURS["hk2"]
    drawn = R.oracle_stack(scans, poses, chains, dev, off, size=(L.SIZE, L.SIZE), map_offset=map_offset,
                           default=L.BACKGROUND)
    for g, d in zip(grids, drawn):
        differ = np.argwhere(g.view(np.uint32) != d.view(np.uint32)).tolist()
        assert differ == [[0, 0]], differ[:5]
    # no end point of the query comes near that corner from any pose of the windows
    reach = float(np.max(np.hypot(scans[L.QUERY][:, 0], scans[L.QUERY][:, 1]))) + np.hypot(*L.DELTA[:2]) + 1.0
    assert reach < 0.5 * L.SIZE * R.RES
    best = sorted(t["best0"] for t in want)
    assert all(a < b for a, b in zip(best, best[1:]))
    assert all(t["best0"] > 0.5 for t in want)  # accepted at the default threshold
    assert all(0.0 < t["map_penalty"] < 1.0 and 0.0 < t["score"] < 1.0 for t in want)
    rejected = L.truth(L.levels(threshold=2.0), pose)
    assert all(L.bits(a["pose"]) != L.bits(b["pose"]) for a, b in zip(want, rejected))
