"""GPU: csm_loop_closure_scan_match (include/csm_loop_closure.h), the result of
SlamProcessor::ScanMatchInterface (slam/slam_processor.cpp:250-326) for every
gated submap of the sharded handle. The truth is the oracle's back end
(tests/lc_interface_ref.py: pyoracle.BackEnd.scan_match, one job per chain, the
Gauss-Newton matcher off, a CountCell PubMap built by the oracle); every double
is compared as its bits: pose, covariance, score, the three clamped responses,
the penalty, and the wide level's unclamped best."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import lc_interface_ref as L  # noqa: E402

ALL = -1.0  # a gate below every best


def _all_devices():
    n = C.c_int(0)
    C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n))
    return list(range(max(1, min(n.value, 8))))


def _handle(devices, size=L.SIZE, env=None):
    """env: variables the matcher contexts read when the handle creates them (csm_create's knobs)."""
    from roborts_csm.loop_closure import DeviceLoopClosure
    scans, poses, chains, _ = L.scene()
    mp = pytest.MonkeyPatch()
    for k, v in (env or {}).items():
        mp.setenv(k, v)
    try:
        lc = DeviceLoopClosure(devices)
    finally:
        mp.undo()
    try:
        ids = [lc.add_scan(s, q) for s, q in zip(scans, poses)]
        assert ids == list(range(len(scans)))
        lc.set_submaps_chains(L.chain_param(size), chains, poses[-1])
    except Exception:
        lc.close()
        raise
    return lc


@pytest.fixture(scope="module")
def one():
    """A handle on device 0 with the scene's five chain maps, and the PubMap there."""
    lc = _handle([0])
    pub = L.device_pub_map()
    yield lc, pub
    lc.close()


@pytest.fixture(scope="module")
def want():
    """The oracle's results at the default levels and pose, computed once."""
    _, poses, _, _ = L.scene()
    return L.truth(L.levels(), poses[-1] + L.DELTA)


def _pose():
    return L.scene()[1][-1] + L.DELTA


def _same(got, truth, levels_run=3):
    """One entry against the oracle's job, every double as its bits."""
    assert got["levels_run"] == levels_run
    assert L.bits(got["pose"]) == L.bits(truth["pose"]), (got["submap"], got["pose"], truth["pose"])
    assert L.bits(got["cov"]) == L.bits(truth["cov"]), got["submap"]
    assert L.bits(got["response"]) == L.bits(truth["response"]), (got["submap"], got["response"], truth["response"])
    assert L.bits([got["map_penalty"]]) == L.bits([truth["map_penalty"]]), got["submap"]
    assert L.bits([got["score"]]) == L.bits([truth["score"]]), (got["submap"], got["score"], truth["score"])
    assert L.bits([got["wide"].score]) == L.bits([truth["best0"]]), got["submap"]
    assert got["wide"].submap == got["submap"] and got["wide_match"]["window"] == got["submap"]


# 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one_device", "all_devices"])
def test_every_entry_equals_oracle(want, which):
    """Five chains, one-cell steps, a gate below every best."""
    lc = _handle([0] if which == "one_device" else _all_devices())
    try:
        pub = L.device_pub_map()
        got, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
    finally:
        lc.close()
    assert n == L.N_CHAINS and [g["submap"] for g in got] == list(range(L.N_CHAINS))
    for g, t in zip(got, want):
        _same(g, t)
        assert g["wide_match"]["accepted"] == 1  # (whichever path the finish took: a tie that matters scores the window)
    # the scene is not trivial: the levels moved the pose, the penalty is a real one
    assert all(0.0 < t["map_penalty"] < 1.0 and 0.0 < t["score"] < 1.0 for t in want)
    assert all(np.any(t["pose"] != _pose()) for t in want)


def test_pipelined_refine_equals_oracle(want):
    """The fine levels through the pipelined driver (what 512 passers and more on a device take):
    contexts created under CSM_PIPELINE=2 with two parts and hand-offs split from two windows on;
    the per-level responses, the score, pose and covariance of all five entries."""
    lc = _handle([0], env={"CSM_PIPELINE": "2", "CSM_PIPELINE_PARTS": "2", "CSM_SPLIT_HANDOFF_MIN": "2"})
    try:
        pub = L.device_pub_map()
        ctx = lc.matcher(0)
        ctx.set_profiling(1)
        got, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
        names = {s["name"] for s in ctx.kernel_stats()}
        ctx.set_profiling(0)
        best = sorted(t["best0"] for t in want)
        two, n2 = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), best[-2], L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
    finally:
        lc.close()
    assert n == L.N_CHAINS and n2 == 2
    # the pipelined driver ran: its hand-offs account under this name, the plain loop's levels never do
    assert any(nm.startswith("host:complete+plan<") for nm in names), sorted(names)
    for g, t in zip(got, want):
        _same(g, t)
    for g in two:  # two passers: one scan a part
        _same(g, want[g["submap"]])


# 2 ---------------------------------------------------------------------------------------
def test_gate_between_two_bests(one, want):
    lc, pub = one
    best = sorted(t["best0"] for t in want)
    assert best[1] < best[2]
    for gate in (0.5 * (best[1] + best[2]), best[2]):  # between two bests; on one (inclusive)
        passers = [j for j, t in enumerate(want) if t["best0"] >= gate]
        assert len(passers) == 3
        for cap in (L.N_CHAINS, 2, 0):
            got, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), gate, cap, L.RANGE_MAX, check=L.CHECK)
            assert n == len(passers)
            assert [g["submap"] for g in got] == passers[:cap]
            for g in got:
                _same(g, want[g["submap"]])
    got, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), best[-1] + 1e-9, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
    assert n == 0 and got == []


# 3 ---------------------------------------------------------------------------------------
def test_wide_level_not_accepted_starts_fine_from_pose_world(one, want):
    """levels[0].response_threshold above every best: the fine level starts from pose_world."""
    lc, pub = one
    lv = L.levels(threshold=2.0)
    truth = L.truth(lv, _pose())
    got, n = lc.scan_match(pub, L.QUERY, lv, _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
    assert n == L.N_CHAINS
    for g, t, w in zip(got, truth, want):
        assert g["wide_match"]["accepted"] == 0
        _same(g, t)
        assert L.bits(t["pose"]) != L.bits(w["pose"])  # the start pose matters in this scene


# 4 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_fine,use_check", [(False, True), (True, False), (False, False)])
def test_coarse_only_and_no_map_check(one, use_fine, use_check):
    lc, pub = one
    truth = L.truth(L.levels(), _pose(), use_fine=use_fine, use_map_check=use_check)
    got, n = lc.scan_match(pub if use_check else None, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX,
                           use_fine_scan_match=use_fine, check=L.CHECK if use_check else None)
    assert n == L.N_CHAINS
    for g, t in zip(got, truth):
        _same(g, t, 3 if use_fine else 1)
        if not use_check:
            assert g["map_penalty"] == 1.0
        if not use_fine:
            s = g["response"][0] * g["map_penalty"]
            assert g["score"] == (1.0 if s > 1.0 else s) and g["response"][1] == 0.0 and g["response"][2] == 0.0


# 5 ---------------------------------------------------------------------------------------
def test_second_call_from_the_first_results_pose(one, want):
    """TryCloseLoop's second call (:326-333): the same chain from the pose the first call found."""
    lc, pub = one
    chains = L.scene()[2]
    for j in (0, L.N_CHAINS - 1):
        first = want[j]["pose"]
        truth = L.truth(L.levels(), first, chains=[chains[j]])[0]
        got, n = lc.scan_match(pub, L.QUERY, L.levels(), first, ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
        assert n == L.N_CHAINS
        _same(got[j], truth)


# 6 ---------------------------------------------------------------------------------------
def test_half_cell_step_takes_the_unpooled_path(one):
    from roborts_csm import _abi
    lc, pub = one
    lv = L.levels(step=0.5 * L.R.RES)
    truth = L.truth(lv, _pose())
    got, n = lc.scan_match(pub, L.QUERY, lv, _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
    assert n == L.N_CHAINS
    for g, t in zip(got, truth):
        assert g["wide_match"]["path"] == _abi.MATCH_UNPOOLED
        _same(g, t)


# 7 ---------------------------------------------------------------------------------------
def test_submap_too_small_for_the_box_is_unsupported(want):
    """The box is +-140 cells around a centre 0.75 / -0.5 cells off the middle: its low y corner
    needs size / 2 - 140.5 > 0, so 282 cells hold it and 281 do not. The failed call launches
    nothing and leaves the handle usable."""
    from roborts_csm import CsmError, _abi
    scans, poses, chains, _ = L.scene()
    lc = _handle([0], size=281)
    try:
        pub = L.device_pub_map()
        with pytest.raises(CsmError) as ei:
            lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
        assert ei.value.status == _abi.CSM_ERR_UNSUPPORTED and "282 cells" in str(ei.value), str(ei.value)
        # the submaps are resident still
        assert lc.match_gated(scans[L.QUERY] * (1 / L.R.RES), L.levels()[0], _pose(), ALL, L.N_CHAINS)[1] == L.N_CHAINS
        lc.set_submaps_chains(L.chain_param(282), chains, poses[-1])
        assert lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, 0, L.RANGE_MAX, check=L.CHECK)[1] == L.N_CHAINS
        lc.set_submaps_chains(L.chain_param(), chains, poses[-1])
        got, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
        assert n == L.N_CHAINS
        for g, t in zip(got, want):
            _same(g, t)
    finally:
        lc.close()


def test_uploaded_submaps_equal_chain_built(one, want):
    """csm_loop_closure_set_submaps with the oracle-built grids and the submaps' one offset: the
    call's results are the chain-built handle's (and the oracle's); submaps whose offsets differ
    are refused with the fine levels on, and served coarse only."""
    from roborts_csm import CsmError, _abi
    from roborts_csm.loop_closure import DeviceLoopClosure
    scans, poses, chains, map_offset = L.scene()
    dev, off = L.R.BLURS["hk2"]
    grids = L.R.oracle_stack(scans, poses, chains, dev, off, size=(L.SIZE, L.SIZE), map_offset=map_offset,
                             default=L.BACKGROUND)
    lc = DeviceLoopClosure([0])
    try:
        for s, q in zip(scans, poses):
            lc.add_scan(s, q)
        pub = L.device_pub_map()
        lc.set_submaps(grids, L.R.RES, np.tile(np.asarray(map_offset), (L.N_CHAINS, 1)), version=1)
        got, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
        assert n == L.N_CHAINS
        for g, t in zip(got, want):
            _same(g, t)
        offs = np.tile(np.asarray(map_offset), (L.N_CHAINS, 1))
        offs[3, 0] += L.R.RES  # one submap a cell aside
        lc.set_submaps(grids, L.R.RES, offs, version=2)
        with pytest.raises(CsmError) as ei:
            lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX, check=L.CHECK)
        assert ei.value.status == _abi.CSM_ERR_UNSUPPORTED and "offset" in str(ei.value)
        coarse, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), ALL, L.N_CHAINS, L.RANGE_MAX,
                                  use_fine_scan_match=False, check=L.CHECK)
        assert n == L.N_CHAINS and all(g["levels_run"] == 1 for g in coarse)
        assert L.bits([coarse[0]["response"][0]]) == L.bits([want[0]["response"][0]])  # an unmoved submap
    finally:
        lc.close()


def test_generous_capacity_is_clamped_to_the_submaps(one, want):
    lc, pub = one
    from roborts_csm import _abi
    import ctypes
    prm = _abi.CsmLoopClosureInterfaceParam()
    for k, lv in enumerate(L.levels()):
        prm.levels[k] = lv.to_c()
    prm.use_fine_scan_match, prm.use_map_check, prm.range_max, prm.min_response = 1, 0, L.RANGE_MAX, ALL
    res = (_abi.CsmLoopClosureInterfaceResult * L.N_CHAINS)()
    pose = np.ascontiguousarray(_pose())
    n = ctypes.c_int32(-1)
    st = lc._lib.csm_loop_closure_scan_match(lc._h, None, L.QUERY, ctypes.byref(prm),
                                             pose.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, res,
                                             2 ** 31 - 1, ctypes.byref(n))
    assert st == 0 and n.value == L.N_CHAINS and [r.submap for r in res] == list(range(L.N_CHAINS))


def test_invalid_arguments(one):
    from roborts_csm import CsmError, _abi
    from roborts_csm.params import FAST_PARAM
    lc, pub = one
    lv = L.levels()
    bad = [dict(levels=(lv[0], FAST_PARAM, lv[2])), dict(levels=(lv[0], lv[1], FAST_PARAM)), dict(min_response=math.nan),
           dict(capacity=-1), dict(scan_id=len(L.scene()[0])), dict(scan_id=-1), dict(pub_map=None)]
    for kw in bad:
        a = dict(pub_map=pub, scan_id=L.QUERY, levels=lv, pose_world=_pose(), min_response=ALL, capacity=L.N_CHAINS,
                 range_max=L.RANGE_MAX, check=L.CHECK)
        a.update(kw)
        with pytest.raises(CsmError) as ei:
            lc.scan_match(**a)
        assert ei.value.status == _abi.CSM_ERR_INVALID_ARG, kw
    assert lc.scan_match(pub, L.QUERY, lv, _pose(), ALL, 0, L.RANGE_MAX, check=L.CHECK)[1] == L.N_CHAINS


# 8 ---------------------------------------------------------------------------------------
def _level_launches(ctx):
    """Launch counts of the level kernels and their finishes: everything the context accounts
    but its host spans, the wide level's search (pyramid, lists, gate) and the grid's upkeep."""
    skip = ("host:", "pyr", "search", "list", "gate", "chain_maps", "grid", "pool")
    out = {}
    for s in ctx.kernel_stats():
        if not s["name"].startswith(skip):  # by kernel: its template arguments follow the window count
            out[s["name"].split("<")[0]] = out.get(s["name"].split("<")[0], 0) + s["launches"]
    return out


def test_refine_is_one_batch_whatever_the_passers(one, want):
    """The fine and super-fine levels of one passer and of all five are launched as often:
    the refine's launches are what a call with use_fine_scan_match adds to one without."""
    lc, pub = one
    ctx = lc.matcher(0)
    best = sorted(t["best0"] for t in want)
    added = {}
    for name, gate, n_want in (("one", best[-1], 1), ("five", ALL, L.N_CHAINS)):
        counts = []
        for fine in (False, True):
            lc.scan_match(pub, L.QUERY, L.levels(), _pose(), gate, L.N_CHAINS, L.RANGE_MAX, use_fine_scan_match=fine,
                          check=L.CHECK)  # (the lists and copies a first call builds are there)
            ctx.set_profiling(1)
            _, n = lc.scan_match(pub, L.QUERY, L.levels(), _pose(), gate, L.N_CHAINS, L.RANGE_MAX,
                                 use_fine_scan_match=fine, check=L.CHECK)
            assert n == n_want
            counts.append(_level_launches(ctx))
            ctx.set_profiling(0)
        added[name] = {k: v - counts[0].get(k, 0) for k, v in counts[1].items() if v != counts[0].get(k, 0)}
        print(name, "coarse only:", counts[0], "with the fine levels:", counts[1])
    assert added["one"] and sum(added["one"].values()) > 0
    assert added["one"] == added["five"], added
