"""Shared by the tests of csm_loop_closure_scan_match: the small scene (five
chains over the ray-cast scans of chain_maps_ref.mid_case, 300-cell submaps at
0.08 m), and the truth from the oracle: pyoracle.BackEnd.scan_match with one
job per chain, the Gauss-Newton matcher off, a CountCell PubMap built by the
oracle, and, per level, oracle.scan_match over the map the back end rebuilt
(the job struct carries no per-level response).

The numbers: range_max 10 m and a resolution of 0.08 m give the back end's map
(int)((10 + 2) * 2 / 0.08) = 300 cells a side; MapSizeCheck's box with the
1.2 m coarse window is +-(10 + 1.2) / 0.08 = 140 cells around a pose at most a
few cells from the centre (150), inside the bound (0, 301): no map grows, and
every truth call asserts so on the oracle's map state before and after.

The background: the oracle's back-end maps are never Reset() as a whole. They
are allocated as the reference allocates (new CellType[n]{default}: element 0
takes kMapUnknownCellProb = 0.3, every other cell GridCell's own 0.5), and
ResetScanMatchMapWithRangeVec's speed-up reset rewrites only the cells the last
build touched. So a fresh back end matches over 0.5, and the handle's chain
maps are drawn over default_cell_prob = 0.5 here: the same grids but for cell
(0, 0), 12 m from the centre on both axes, which no beam of a 10 m laser
reaches from a window around the centre (tests/test_lc_interface_scene.py
checks both statements on the CPU)."""
import functools
import math

import numpy as np

import chain_maps_ref as R

SIZE = 300
BACKGROUND = 0.5          # what the oracle's fresh back-end maps hold where no scan was drawn
N_CHAINS = 5
RANGE_MAX = 10.0
MAP_RES = 0.05            # the PubMap's
CHECK = (100, 2.5, 0.015)  # config/simulatin_param.yaml's map check
QUERY = 10                # the kept scan matched: the last of the drive
DELTA = np.array([0.06, -0.04, 0.03])  # pose_world - the current pose


def levels(step=R.RES, threshold=0.5):
    """The ScanMatchParam set: a wide coarse window of 1.2 m / +-pi/8 at `step`, then
    config/simulatin_param.yaml's fine and super-fine levels."""
    from roborts_csm.params import SIM_YAML_LEVELS, CorrelationScanMatchParam
    wide = CorrelationScanMatchParam(1.2, step, math.pi / 8, 0.0349, threshold, 100, 0, False, 0)
    return (wide, SIM_YAML_LEVELS[1], SIM_YAML_LEVELS[2])


@functools.lru_cache(maxsize=None)
def scene():
    scans, poses, chains, map_offset = R.mid_case(n_grids=N_CHAINS, size=SIZE)
    assert all(len(c) > 0 for c in chains)
    return scans, poses, chains, map_offset


def chain_param(size=SIZE):
    from roborts_csm.chain_maps import ChainMapParam
    dev, off = R.BLURS["hk2"]
    return ChainMapParam(R.RES, dev, off, size, size, default_cell_prob=BACKGROUND)


def backend_param(lv, use_map_check=True):
    from roborts_csm.backend import BackEndParam
    dev, off = R.BLURS["hk2"]
    return BackEndParam(range_max=RANGE_MAX, gaussian_blur_offset=off, map_resolution=MAP_RES,
                        coarse_map_resolution=R.RES, coarse_map_deviation=dev, fine_map_resolution=R.RES,
                        fine_map_deviation=dev, use_map_check_feedback=use_map_check, map_check_point_num=CHECK[0],
                        map_check_bound_tolerance=CHECK[1], map_check_penalty_gain=CHECK[2], levels=tuple(lv),
                        use_optimize_scan_match=False)


PUB_SCANS = (0, 5, 10)


def _pub_geometry():
    _, poses, _, _ = scene()
    size = (480, 480)
    cur = poses[-1]
    return size, (-(cur[0] - 0.5 * size[0] * MAP_RES), -(cur[1] - 0.5 * size[1] * MAP_RES))


def oracle_pub_map():
    """A CountCell PubMap of three of the drive's scans, full lines, built by the oracle."""
    import pyoracle as O
    scans, poses, _, _ = scene()
    size, off = _pub_geometry()
    m = O.GridMap(1, MAP_RES, size, off, 0.0, 0.5)
    m.set_options(True, False, 0.72, 0.2)
    for k in PUB_SCANS:
        m.update_by_range(scans[k] * (1 / MAP_RES), poses[k])
    return m


def device_pub_map():
    """The same map on device 0."""
    from roborts_csm.gridmap import OccuGridMap
    scans, poses, _, _ = scene()
    size, off = _pub_geometry()
    m = OccuGridMap(MAP_RES, size, off, 0.0, 0.5, kind=1)
    m.set_options(True, False, 0.72, 0.2)
    for k in PUB_SCANS:
        m.UpdateMapByRange(scans[k] * (1 / MAP_RES), poses[k])
    return m


def bits(v):
    return np.asarray(v, dtype=np.float64).reshape(-1).view(np.uint64).tolist()


def truth(lv, pose_world, use_fine=True, use_map_check=True, chains=None, grids=None):
    """Per chain: dict(pose, cov, score, map_penalty, response (3,), best0: the coarse level's
    unclamped best). pose_world: one pose for every chain, or one per chain. grids: a list that
    receives the fine maps the back end matched on."""
    import pyoracle as O
    from roborts_csm.backend import job_results, make_jobs
    scans, poses, all_chains, _ = scene()
    chains = all_chains if chains is None else chains
    n = len(chains)
    pw = np.asarray(pose_world, dtype=np.float64)
    pw = np.tile(pw, (n, 1)) if pw.ndim == 1 else pw
    be = O.BackEnd(backend_param(lv, use_map_check).to_c())
    for k in range(len(scans)):
        assert be.add_scan(scans[k], poses[k]) == k
    arr = make_jobs([scans[QUERY]] * n, chains, pw, use_fine)
    be.scan_match(arr, n, poses[-1], oracle_pub_map() if use_map_check else None)
    res = job_results(arr, n)
    cells = scans[QUERY] * (1 / R.RES)
    out = []
    if grids is not None:
        grids.extend(be.map(j, 1).cells()[0].copy() for j in range(n))
    for j in range(n):
        for which in (0, 1):  # no map grew: MapSizeCheck left both maps as they were created
            inf = be.map(j, which).info()
            assert (inf["size_x"], inf["size_y"]) == (SIZE, SIZE), inf
        fine = be.map(j, 1)
        inf = fine.info()
        m = O.Map(fine.cells()[0].copy(), R.RES, inf["offset"], inf["map_update_index"])
        pose, cov, resp = pw[j].copy(), np.eye(3).reshape(9), [0.0, 0.0, 0.0]
        for l in range(3 if use_fine else 1):
            resp[l], pose, cov, _, _ = O.scan_match(m, cells, lv[l], pose, cov)
        # the per-level replay is the back end's own call
        assert bits(pose) == bits(res[j].pose) and bits(cov) == bits(res[j].cov), j
        na, ns = _dims(lv[0])
        ctr = np.array([(1 / R.RES) * pw[j][0] + (1 / R.RES) * inf["offset"][0],
                        (1 / R.RES) * pw[j][1] + (1 / R.RES) * inf["offset"][1], pw[j][2]])
        best0 = float(np.max(O.score_window(m, cells, lv[0], ctr, na * ns * ns)))
        out.append({"pose": res[j].pose, "cov": res[j].cov, "score": res[j].score, "map_penalty": res[j].map_penalty,
                    "response": np.array(resp), "best0": best0})
    return out


def _dims(p):
    import roborts_csm
    return roborts_csm.window_dims(p)
