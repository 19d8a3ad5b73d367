"""GPU: loop-closure submaps drawn on the devices from chains of kept scans
(csm_loop_closure_add_scan / _set_scan_pose / _set_submaps_chains), on one
device and on every visible device: match_gated and match_gated_full must
equal, in every field but the times, the same calls after set_submaps with the
oracle-built grids (tests/chain_maps_ref.py oracle_stack) and equal offsets."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import chain_maps_ref as R  # noqa: E402

SIZE = 300
N_CHAINS = 24


def _all_devices():
    n = C.c_int(0)
    C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n))
    return list(range(max(1, min(n.value, 8))))


@pytest.fixture(scope="module")
def case():
    """24 chains over 11 ray-cast scans, the maps centred on the query pose, and the oracle's grids."""
    scans, poses, chains, map_offset = R.mid_case(n_grids=N_CHAINS, size=SIZE)
    dev, off = R.BLURS["hk2"]
    grids = R.oracle_stack(scans, poses, chains, dev, off, size=(SIZE, SIZE), map_offset=map_offset)
    return scans, poses, chains, map_offset, grids


def _param():
    from roborts_csm.chain_maps import ChainMapParam
    dev, off = R.BLURS["hk2"]
    return ChainMapParam(R.RES, dev, off, SIZE, SIZE, default_cell_prob=R.DEFAULT)


def _fields(results, n_pass, worlds, matches, covs):
    """Everything a gated match returns but the times, floats as their bits."""
    def b(v):
        return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()
    out = [n_pass, b(worlds), [(r.global_index, r.submap) for r in results],
           b([[r.score, r.x, r.y, r.angle] for r in results])]
    if matches is not None:
        out.append(b(covs))
        for m in matches:
            # of the search's statistics the ones that describe the answer; how many nodes the
            # concurrent descent happened to visit on the way is, like build_ms, not compared
            s = {k: m["search"][k] for k in ("depth", "exhaustive", "candidates", "top_box")}
            f = m["front"]
            out.append((b([m["response"], m["threshold"], f.score, f.x, f.y, f.angle]), b(m["pose_map"]), m["accepted"],
                        m["window"], f.flat_index, m["count"], m["path"], m["collected"], s))
    return out


def _queries(lc, cells, p, pose, gates):
    out = []
    for T in gates:
        res, n = lc.match_gated(cells, p, pose, T, N_CHAINS)
        out.append(_fields(res, n, lc.last_pose_worlds, None, None))
        covs = np.ascontiguousarray(np.tile(np.eye(3).reshape(9), (N_CHAINS, 1)))
        res, n, matches = lc.match_gated_full(cells, p, pose, T, N_CHAINS, covs)
        out.append(_fields(res, n, lc.last_pose_worlds, matches, covs[:len(res)]))
        assert lc.last_n_devices == lc.n_devices
    return out


@pytest.mark.parametrize("which", ["one_device", "all_devices"])
def test_gated_matches_equal_uploaded_oracle_grids(case, which):
    from roborts_csm.loop_closure import DeviceLoopClosure
    from roborts_csm.params import CorrelationScanMatchParam
    scans, poses, chains, map_offset, grids = case
    devices = [0] if which == "one_device" else _all_devices()
    p = CorrelationScanMatchParam(1.2, R.RES, math.pi / 8, 0.0349, 0.5, 100, 0, False, 0)
    cur = poses[-1]
    cells = scans[-1] * (1 / R.RES)

    up = DeviceLoopClosure(devices)
    try:
        up.set_submaps(grids, R.RES, np.tile(np.asarray(map_offset), (N_CHAINS, 1)), version=1)
        best = sorted(r.score for r in up.match_gated(cells, p, cur, -1.0, N_CHAINS)[0])
        assert len(best) == N_CHAINS
        gates = (0.0, best[N_CHAINS // 2], best[-1])
        want = _queries(up, cells, p, cur, gates)
    finally:
        up.close()
    assert [w[0] for w in want] == [N_CHAINS, N_CHAINS] + [w[0] for w in want[2:]] and want[-1][0] >= 1

    lc = DeviceLoopClosure(devices)
    try:
        # the scans go in at other poses first: what is drawn is what set_scan_pose left
        ids = [lc.add_scan(s, q + np.array([0.5, -0.25, 0.1])) for s, q in zip(scans, poses)]
        assert ids == list(range(len(scans)))
        for i, q in enumerate(poses):
            lc.set_scan_pose(i, q)
        lc.set_submaps_chains(_param(), chains, cur)
        got = _queries(lc, cells, p, cur, gates)
    finally:
        lc.close()
    assert got == want


def test_failed_set_submaps_chains_leaves_no_submaps(case):
    """As the host form (test_capi_failed_set_submaps_leaves_no_submaps): a
    failed call commits nothing, the next match fails with CSM_ERR_NO_GRID,
    and a good call restores service."""
    from roborts_csm import CsmError, _abi
    from roborts_csm.chain_maps import ChainMapParam
    from roborts_csm.loop_closure import DeviceLoopClosure
    from roborts_csm.params import CorrelationScanMatchParam
    scans, poses, chains, map_offset, grids = case
    p = CorrelationScanMatchParam(1.2, R.RES, math.pi / 8, 0.0349, 0.5, 100, 0, False, 0)
    cur = poses[-1]
    cells = scans[-1] * (1 / R.RES)
    lc = DeviceLoopClosure(_all_devices())
    try:
        for s, q in zip(scans, poses):
            lc.add_scan(s, q)
        lc.set_submaps_chains(_param(), chains, cur)
        n_good = lc.match_gated(cells, p, cur, 0.0, N_CHAINS)[1]
        assert n_good == N_CHAINS
        bad_chains = [list(c) for c in chains]
        bad_chains[-1][-1] = len(scans)  # an id of no kept scan, in the last shard
        dev, off = R.BLURS["hk2"]
        for param, ch, status in ((_param(), bad_chains, _abi.CSM_ERR_INVALID_ARG),
                                  (ChainMapParam(R.RES, dev, off, SIZE, SIZE, use_blur=False), chains,
                                   _abi.CSM_ERR_UNSUPPORTED)):
            with pytest.raises(CsmError) as ei:
                lc.set_submaps_chains(param, ch, cur)
            assert ei.value.status == status
            with pytest.raises(CsmError) as ei:
                lc.match_gated(cells, p, cur, 0.0, N_CHAINS)
            assert ei.value.status == _abi.CSM_ERR_NO_GRID
            lc.set_submaps_chains(_param(), chains, cur)  # a good call restores service
            assert lc.match_gated(cells, p, cur, 0.0, N_CHAINS)[1] == n_good
        with pytest.raises(CsmError) as ei:
            lc.set_scan_pose(len(scans), cur)
        assert ei.value.status == _abi.CSM_ERR_INVALID_ARG
    finally:
        lc.close()
