"""csm_scan_matchers_batch_grids_seeded: the 3-level driver from
ScanMatchers::ScanMatch's state after its Gauss-Newton step
(scan_matchers.h:205-281). Six ray-cast scans of two 600 x 600 worlds over a
2-grid stack, on the level-by-level driver and on the pipelined one (a context
created under CSM_PIPELINE=2):

- first_level 0 without a seed is csm_scan_matchers_batch_grids;
- first_level 1, seeded with failed / (cost + failed), from the Gauss-Newton
  pose equals the oracle's composition of its two matchers (test_optimize.py's
  _oracle_scan_matchers, restated here) bit for bit;
- use_fine = 0 runs the coarse level alone, with and without a seed;
- bad first_level and grid_index values are rejected.
"""
import ctypes as C

import numpy as np
import pytest

import pyoracle as O

pytestmark = pytest.mark.gpu

FAILED = 20.0  # ParamConfig's optimize_failed_cost: every scan's Gauss-Newton cost is below it
GIDX = [0, 1, 0, 1, 1, 0]


@pytest.fixture(scope="module", params=["levels", "pipelined"])
def ctx(request):
    import roborts_csm
    mp = pytest.MonkeyPatch()
    if request.param == "pipelined":
        mp.setenv("CSM_PIPELINE", "2")
    c = roborts_csm.Context(0)
    mp.undo()
    yield c
    c.close()


@pytest.fixture(scope="module")
def case():
    """Scans, the stack, and the oracle's results, computed once."""
    from roborts_csm import worlds
    from roborts_csm.params import SIM_YAML_LEVELS, SIM_YAML_OPTIMIZE
    ws = [worlds.make_world(600, 600, 0.05, seed=s) for s in (21, 23)]
    per = [worlds.make_scan_batch(w, 3, seed=22 + k) for k, w in enumerate(ws)]
    take = [0, 0]
    scans, init = [], []
    for g in GIDX:
        b, k = per[g], take[g]
        take[g] += 1
        scans.append(b.points_cells[b.offsets[k]:b.offsets[k + 1]])
        # set_grid_stack places the stack at offset (0, 0): the worlds' poses move with their offset
        init.append(b.init_poses[k] + [ws[g].offset[0], ws[g].offset[1], 0.0])
    points = np.vstack(scans)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    maps = [O.Map(w.grid, 0.05, (0.0, 0.0)) for w in ws]
    want = {"gn": [], "seeded": [], "plain": [], "coarse": []}
    for k, g in enumerate(GIDX):
        m, pts = maps[g], scans[k]
        cost, proc, _ = O.optimize_scan_match(m, pts, SIM_YAML_OPTIMIZE, init[k])
        want["gn"].append((cost, proc))
        # ScanMatchers::ScanMatch with use_optimize_scan_match, cost <= failed (:205-281)
        score, times, cov = FAILED / (cost + FAILED), 1, np.eye(3)
        for lv in SIM_YAML_LEVELS[1:]:
            r, proc, cov, _, _ = O.scan_match(m, pts, lv, proc, cov)
            score, times = score + r, times + 1
        want["seeded"].append((score / times, proc, cov))
        want["plain"].append(O.scan_matchers(m, pts, SIM_YAML_LEVELS, init[k], np.eye(3), True))
        r, p0, c0, _, _ = O.scan_match(m, pts, SIM_YAML_LEVELS[0], np.array(init[k], dtype=np.float64), np.eye(3))
        want["coarse"].append((r, p0, c0))
    return dict(grids=np.stack([w.grid for w in ws]), points=points, offsets=offsets, init=np.array(init), want=want)


def _fresh(case):
    n = len(GIDX)
    return case["init"].copy(), np.tile(np.eye(3).reshape(-1), (n, 1))


def _batch_grids(ctx, case, poses, covs, use_fine=True):
    """csm_scan_matchers_batch_grids through the C-ABI."""
    import roborts_csm
    from roborts_csm import _abi
    from roborts_csm.params import SIM_YAML_LEVELS
    lv = (_abi.CsmParam * 3)(*[l.to_c() for l in SIM_YAML_LEVELS])
    gi = np.array(GIDX, dtype=np.int32)
    scores = np.zeros(len(GIDX))
    dp = lambda a: a.ctypes.data_as(_abi._dp)
    st = roborts_csm._lib.csm_scan_matchers_batch_grids(
        ctx._h, len(GIDX), dp(case["points"]), case["offsets"].ctypes.data_as(C.POINTER(C.c_int64)),
        gi.ctypes.data_as(_abi._i32p), lv, 1 if use_fine else 0, dp(poses), dp(covs), dp(scores))
    assert st == _abi.CSM_OK
    return scores


def test_level0_unseeded_is_batch_grids(ctx, case):
    from roborts_csm.params import SIM_YAML_LEVELS
    ctx.set_grid_stack(case["grids"], 0.05)
    p0, c0 = _fresh(case)
    s0 = _batch_grids(ctx, case, p0, c0)
    p1, c1 = _fresh(case)
    s1 = ctx.scan_matchers_batch_grids_seeded(case["points"], case["offsets"], GIDX, SIM_YAML_LEVELS, p1, c1)
    assert np.array_equal(s0, s1) and np.array_equal(p0, p1) and np.array_equal(c0, c1)
    for k, (s, p, c) in enumerate(case["want"]["plain"]):
        assert s1[k] == s and np.array_equal(p1[k], p) and np.array_equal(c1[k], np.asarray(c).reshape(-1)), k


def test_level1_seeded_matches_oracle_composition(ctx, case):
    from roborts_csm.params import SIM_YAML_LEVELS, SIM_YAML_OPTIMIZE
    ctx.set_grid_stack(case["grids"], 0.05)
    poses, covs = _fresh(case)
    costs, _ = ctx.optimize_scan_match_batch_grids(case["points"], case["offsets"], GIDX, SIM_YAML_OPTIMIZE, poses)
    for k, (c, p) in enumerate(case["want"]["gn"]):
        assert costs[k] == c and np.array_equal(poses[k], p) and c <= FAILED, k
    seed = FAILED / (costs + FAILED)
    scores = ctx.scan_matchers_batch_grids_seeded(case["points"], case["offsets"], GIDX, SIM_YAML_LEVELS, poses, covs,
                                                  first_level=1, score_seed=seed)
    for k, (s, p, c) in enumerate(case["want"]["seeded"]):
        assert scores[k] == s and np.array_equal(poses[k], p) and np.array_equal(covs[k], np.asarray(c).reshape(-1)), k


def test_coarse_only(ctx, case):
    from roborts_csm.params import SIM_YAML_LEVELS
    ctx.set_grid_stack(case["grids"], 0.05)
    seed = np.linspace(0.2, 0.9, len(GIDX))
    for sd in (None, seed):
        poses, covs = _fresh(case)
        scores = ctx.scan_matchers_batch_grids_seeded(case["points"], case["offsets"], GIDX, SIM_YAML_LEVELS, poses,
                                                      covs, use_fine=False, score_seed=sd)
        for k, (r, p, c) in enumerate(case["want"]["coarse"]):
            assert scores[k] == (r / 1 if sd is None else (sd[k] + r) / 2), k
            assert np.array_equal(poses[k], p) and np.array_equal(covs[k], np.asarray(c).reshape(-1)), k


def test_rejected_arguments(ctx, case):
    import roborts_csm
    from roborts_csm import _abi
    from roborts_csm.params import SIM_YAML_LEVELS
    ctx.set_grid_stack(case["grids"], 0.05)

    def call(**kw):
        poses, covs = _fresh(case)
        gi = kw.pop("grid_index", GIDX)
        with pytest.raises(roborts_csm.CsmError) as e:
            ctx.scan_matchers_batch_grids_seeded(case["points"], case["offsets"], gi, SIM_YAML_LEVELS, poses, covs, **kw)
        assert e.value.status == _abi.CSM_ERR_INVALID_ARG
        assert np.array_equal(poses, case["init"])

    call(first_level=2)
    call(first_level=-1)
    call(first_level=1, use_fine=False)
    call(grid_index=[0, 1, 2, 1, 1, 0])
    call(grid_index=[0, -1, 0, 1, 1, 0])
