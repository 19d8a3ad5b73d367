"""GPU: the matcher's grid stack drawn on the device from chains of kept scans
(csm_scan_store_*, csm_set_grid_stack_chains, csm_grid_download;
csrc/csm_chain_maps.*).

The yardstick is the oracle: per grid a ScanMatchMap that was Reset() and then
ResetScanMatchMapWithRangeVec'd with the chain's scans (tests/chain_maps_ref.py
oracle_stack). The bar is identity of every cell's 32 bits. The small cases and
what they reach on purpose are chain_maps_ref's (tests/test_chain_maps_pyref.py
checks that on the CPU, and counts which cases catch each broken rule)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import chain_maps_ref as R  # noqa: E402

CASES = [(b, n) for b in R.BLURS for n in (1, 5)]
SHAPE = (R.SIZE_Y, R.SIZE_X)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _param(blur, size=(R.SIZE_X, R.SIZE_Y), **kw):
    from roborts_csm.chain_maps import ChainMapParam
    dev, off = R.BLURS[blur] if isinstance(blur, str) else blur
    return ChainMapParam(R.RES, dev, off, size[0], size[1], default_cell_prob=R.DEFAULT, **kw)


def _store(scans, poses, device=0):
    from roborts_csm.chain_maps import ScanStore
    st = ScanStore(device)
    assert [st.add(s, p) for s, p in zip(scans, poses)] == list(range(len(scans)))
    assert st.count() == (len(scans), sum(s.shape[0] for s in scans))
    return st


def _download(ctx, n, shape=SHAPE):
    from roborts_csm.chain_maps import grid_download
    return np.stack([grid_download(ctx, g, shape) for g in range(n)])


def _raw_build(ctx, store, mp, n_grids, offsets, ids, map_offset=R.MAP_OFFSET):
    """csm_set_grid_stack_chains with the arrays as given -> status."""
    from roborts_csm import _lib
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    ids = np.ascontiguousarray(ids if len(ids) else [0], dtype=np.int32)
    mo = np.ascontiguousarray(map_offset, dtype=np.float64)
    i32p = C.POINTER(C.c_int32)
    return _lib.csm_set_grid_stack_chains(ctx._h, store._h, C.byref(mp), int(n_grids), off.ctypes.data_as(i32p),
                                          ids.ctypes.data_as(i32p), mo.ctypes.data_as(C.POINTER(C.c_double)), None)


@pytest.fixture(scope="module")
def small():
    """The small scans and their oracle stacks, computed once."""
    scans, poses = R.small_scans()
    stacks = {}
    for blur, n in CASES:
        dev, off = R.BLURS[blur]
        stacks[(blur, n)] = R.oracle_stack(scans, poses, R.CHAINS1 if n == 1 else R.CHAINS5, dev, off)
    return scans, poses, stacks


@pytest.fixture(scope="module")
def ctx():
    import roborts_csm
    c = roborts_csm.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def store(small):
    st = _store(small[0], small[1])
    yield st
    st.close()


@pytest.fixture(scope="module")
def mid():
    """16 grids of 300 x 300 from 11 scans of 1081 ray-cast beams, with the oracle's stack."""
    scans, poses, chains, map_offset = R.mid_case()
    blur = R.BLURS["hk2"]
    want = R.oracle_stack(scans, poses, chains, blur[0], blur[1], size=(300, 300), map_offset=map_offset)
    return scans, poses, chains, map_offset, blur, want


# ---- 1. the stack equals the oracle's, bit for bit ---------------------------------
@pytest.mark.parametrize("blur,n", CASES)
def test_stack_equals_oracle(small, ctx, store, blur, n):
    from roborts_csm.chain_maps import set_grid_stack_chains
    chains = R.CHAINS1 if n == 1 else R.CHAINS5
    info = set_grid_stack_chains(ctx, store, _param(blur), chains, R.MAP_OFFSET)
    assert (info.size_x, info.size_y, info.resolution, info.offset_x, info.offset_y) == \
           (R.SIZE_X, R.SIZE_Y, R.RES, R.MAP_OFFSET[0], R.MAP_OFFSET[1])
    assert info.update_index == min(len(c) for c in chains) - 1
    got = _download(ctx, n)
    want = small[2][(blur, n)]
    diff = np.nonzero(_u32(got) != _u32(want))
    print(f"{blur} x {n}: {diff[0].size} cells differ")
    assert diff[0].size == 0, [(int(g), int(y), int(x), float(got[g, y, x]), float(want[g, y, x]))
                               for g, y, x in zip(*(d[:8] for d in diff))]


def test_pose_change_between_builds(small, ctx):
    """set_pose (UpdateRangeData after a graph solve) moves the next build, not the points."""
    from roborts_csm.chain_maps import set_grid_stack_chains
    scans, poses, stacks = small
    dev, off = R.BLURS["hk2"]
    st = _store(scans, poses)
    try:
        set_grid_stack_chains(ctx, st, _param("hk2"), R.CHAINS5, R.MAP_OFFSET)
        assert np.array_equal(_u32(_download(ctx, 5)), _u32(stacks[("hk2", 5)]))
        moved = R.moved_poses(poses)
        for i, p in enumerate(moved):
            st.set_pose(i, p)
        set_grid_stack_chains(ctx, st, _param("hk2"), R.CHAINS5, R.MAP_OFFSET)
        want = R.oracle_stack(scans, moved, R.CHAINS5, dev, off)
        assert not np.array_equal(_u32(want), _u32(stacks[("hk2", 5)]))
        assert np.array_equal(_u32(_download(ctx, 5)), _u32(want))
        from roborts_csm import CsmError, _abi
        with pytest.raises(CsmError) as ei:
            st.set_pose(len(scans), poses[0])
        assert ei.value.status == _abi.CSM_ERR_INVALID_ARG
    finally:
        st.close()


def test_fewer_grids_over_a_larger_build(small, ctx, store):
    """A one-grid build over a five-grid one: no cell of the old stack shows, and the stack has one grid."""
    from roborts_csm import CsmError, _abi
    from roborts_csm.chain_maps import grid_download, set_grid_stack_chains
    scans, poses, _ = small
    dev, off = R.BLURS["hk7_over1"]
    set_grid_stack_chains(ctx, store, _param("hk7_over1"), R.CHAINS5, R.MAP_OFFSET)
    chains = [[4, 5]]
    info = set_grid_stack_chains(ctx, store, _param("hk7_over1"), chains, R.MAP_OFFSET)
    assert info.update_index == 1
    assert np.array_equal(_u32(_download(ctx, 1)), _u32(R.oracle_stack(scans, poses, chains, dev, off)))
    with pytest.raises(CsmError) as ei:
        grid_download(ctx, 1, SHAPE)
    assert ei.value.status == _abi.CSM_ERR_INVALID_ARG
    with pytest.raises(CsmError):
        grid_download(ctx, 0, (R.SIZE_Y, R.SIZE_X + 1))


def test_kernel_stats_name_the_build(small, store):
    import roborts_csm
    from roborts_csm.chain_maps import set_grid_stack_chains
    with roborts_csm.Context(0) as c:
        c.set_profiling(True)
        set_grid_stack_chains(c, store, _param("hk2"), R.CHAINS5, R.MAP_OFFSET)
        names = {s["name"]: s for s in c.kernel_stats()}
        assert {"chain_maps:fill", "chain_maps:splat", "chain_maps:plan"} <= set(names), sorted(names)
        assert names["chain_maps:fill"]["algorithmic_bytes"] == 5 * R.SIZE_X * R.SIZE_Y * 4
        n_pts = sum(small[0][i].shape[0] for ch in R.CHAINS5 for i in ch)
        assert names["chain_maps:splat"]["scorings"] == n_pts * 25
        assert np.array_equal(_u32(_download(c, 5)), _u32(small[2][("hk2", 5)]))  # timed or not, the same stack


# ---- 2. sizes -----------------------------------------------------------------------------
def test_mid_size_stack_equals_oracle(mid):
    import roborts_csm
    from roborts_csm.chain_maps import set_grid_stack_chains
    scans, poses, chains, map_offset, blur, want = mid
    st = _store(scans, poses)
    try:
        with roborts_csm.Context(0) as c:
            info = set_grid_stack_chains(c, st, _param(blur, size=(300, 300)), chains, map_offset)
            assert info.update_index == 0
            got = _download(c, len(chains), (300, 300))
    finally:
        st.close()
    assert int((want == np.float32(1.0)).sum()) > 1000  # walls were drawn
    assert np.array_equal(_u32(got), _u32(want)), int((_u32(got) != _u32(want)).sum())


def test_cell_index_past_2_31(small, store):
    """700,000 grids of 64 x 48: the last grid's cells lie past element 2^31 of
    the stack (grid, row and column multiply in 64 bits, or this grid is drawn
    somewhere else)."""
    import roborts_csm
    from roborts_csm.chain_maps import grid_download
    n = 700_000
    assert (n - 1) * R.SIZE_X * R.SIZE_Y > 2**31
    scans, poses, stacks = small
    off = np.zeros(n + 1, dtype=np.int32)  # every chain empty but the first and the last
    off[1:] = len(R.CHAINS1[0])
    off[n] = 2 * len(R.CHAINS1[0])
    ids = R.CHAINS1[0] + R.CHAINS1[0]
    with roborts_csm.Context(0) as c:
        assert _raw_build(c, store, _param("hk2").to_c(), n, off, ids) == 0
        want = stacks[("hk2", 1)][0]
        for g in (0, n - 1):
            assert np.array_equal(_u32(grid_download(c, g, SHAPE)), _u32(want)), g
        for g in (1, n // 2, n - 2):
            assert np.all(grid_download(c, g, SHAPE) == np.float32(R.DEFAULT)), g


# ---- 3. the matcher reads what was built --------------------------------------------------------
def test_matcher_reads_the_built_stack(mid):
    """csm_scan_matchers_batch_grids and csm_search_gated on the built stack
    against the same calls on the oracle's grids uploaded with csm_set_grid_stack."""
    import roborts_csm
    from roborts_csm import _abi, _lib
    from roborts_csm.chain_maps import set_grid_stack_chains
    from roborts_csm.loop_closure import world_to_map
    from roborts_csm.params import SIM_YAML_LEVELS, CorrelationScanMatchParam
    scans, poses, chains, map_offset, blur, want = mid
    n_grids = len(chains)
    st = _store(scans, poses)
    built, uploaded = roborts_csm.Context(0), roborts_csm.Context(0)
    try:
        info = set_grid_stack_chains(built, st, _param(blur, size=(300, 300)), chains, map_offset)
        stack = np.ascontiguousarray(want)
        up_info = _abi.CsmMapInfo(R.RES, map_offset[0], map_offset[1], 300, 300, info.update_index, 0)
        assert _lib.csm_set_grid_stack(uploaded._h, stack.ctypes.data_as(C.c_void_p), n_grids, C.byref(up_info), 1) == 0

        # the 3-level driver: every scan on its own grid, from a pose a little off
        cells = [s * (1 / R.RES) for s in scans]
        pts = np.ascontiguousarray(np.concatenate(cells))
        off = np.zeros(len(cells) + 1, dtype=np.int64)
        off[1:] = np.cumsum([c.shape[0] for c in cells])
        gi = np.ascontiguousarray([(3 * k + 5) % n_grids for k in range(len(cells))], dtype=np.int32)
        lv = (_abi.CsmParam * 3)(*[l.to_c() for l in SIM_YAML_LEVELS])
        out = []
        for c in (built, uploaded):
            p = np.ascontiguousarray(poses + np.array([0.06, -0.04, 0.03]))
            cov = np.ascontiguousarray(np.tile(np.eye(3).reshape(9), (len(cells), 1)))
            sc = np.zeros(len(cells))
            dp = C.POINTER(C.c_double)
            stt = _lib.csm_scan_matchers_batch_grids(c._h, len(cells), pts.ctypes.data_as(dp),
                                                     off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     gi.ctypes.data_as(C.POINTER(C.c_int32)), lv, 1,
                                                     p.ctypes.data_as(dp), cov.ctypes.data_as(dp), sc.ctypes.data_as(dp))
            assert stt == 0, _lib.csm_last_error(c._h)
            out.append((p.view(np.uint64).tolist(), cov.view(np.uint64).tolist(), sc.view(np.uint64).tolist()))
        assert out[0] == out[1]
        assert np.all(np.frombuffer(np.array(out[0][2], dtype=np.uint64).tobytes(), dtype=np.float64) > 0.3)

        # the gated search: one query against every grid
        p = CorrelationScanMatchParam(1.2, R.RES, math.pi / 8, 0.0349, 0.5, 100, 0, False, 0)
        centers = np.stack([world_to_map(poses[-1], R.RES, map_offset)] * n_grids)
        ref = uploaded.best_windows(cells[-1], p, np.arange(n_grids), centers)[0]
        for T in (0.0, float(np.median(ref)), float(ref.max())):
            got = [c.search_gated(cells[-1], p, np.arange(n_grids), centers, T) for c in (built, uploaded)]
            a, b = ([w.tolist()] + [np.asarray(v, dtype=np.float64).view(np.uint64).tolist() for v in (s, x, y, an)] +
                    [f.tolist(), npass] for w, s, f, x, y, an, npass, _ in got)
            assert a == b, T
            assert a[-1] == int((ref >= T).sum()) and a[-1] >= 1
    finally:
        built.close()
        uploaded.close()
        st.close()


# ---- 4. what is refused -----------------------------------------------------------------------------
def test_unsupported_modes_say_which(small, ctx, store):
    from roborts_csm import CsmError, _abi
    from roborts_csm.chain_maps import set_grid_stack_chains
    for param, word in ((_param("hk2", use_blur=False), "use_blur"),
                        (_param((0.5 * R.RES, 0.72)), "deviation"), (_param((10 * R.RES, 0.72)), "deviation"),
                        (_param((0.0, 0.72)), "deviation")):
        with pytest.raises(CsmError) as ei:
            set_grid_stack_chains(ctx, store, param, R.CHAINS5, R.MAP_OFFSET)
        assert ei.value.status == _abi.CSM_ERR_UNSUPPORTED
        assert word in str(ei.value), str(ei.value)


def test_rejected_calls_leave_the_previous_grid(small, store):
    import roborts_csm
    from roborts_csm import _abi, _lib
    from roborts_csm.chain_maps import ScanStore, set_grid_stack_chains
    from roborts_csm.loop_closure import world_to_map
    from roborts_csm.params import CorrelationScanMatchParam
    scans, poses, stacks = small
    chains = R.CHAINS5[1:]  # no empty chain: the stack answers matches
    p = CorrelationScanMatchParam(0.4, R.RES, 0.2, 0.0349, 0.5, 100, 0, False, 0)
    centers = np.stack([world_to_map(poses[1], R.RES, R.MAP_OFFSET)] * 4)
    cells = scans[1] * (1 / R.RES)
    with roborts_csm.Context(0) as c:
        info = set_grid_stack_chains(c, store, _param("hk2"), chains, R.MAP_OFFSET)
        assert info.update_index == 0
        before = _download(c, 4)
        assert np.array_equal(_u32(before), _u32(stacks[("hk2", 5)][1:]))
        answer = [np.asarray(v).tolist() for v in c.best_windows(cells, p, np.arange(4), centers)]
        good = _param("hk2").to_c()
        off, ids = [0, 1, 5, 8, 12], [i for ch in chains for i in ch]
        INV, UNS = _abi.CSM_ERR_INVALID_ARG, _abi.CSM_ERR_UNSUPPORTED
        assert _raw_build(c, store, good, 4, off, ids[:-1] + [len(scans)]) == INV   # an id of no kept scan
        assert b"kept scan" in _lib.csm_last_error(c._h)
        assert _raw_build(c, store, good, 4, off, [-1] + ids[1:]) == INV
        assert _raw_build(c, store, good, 4, [0, 5, 1, 8, 12], ids) == INV          # offsets decrease
        assert _raw_build(c, store, good, 4, [1, 1, 5, 8, 12], ids) == INV          # ... or start late
        assert _raw_build(c, store, good, 0, off, ids) == INV
        assert _raw_build(c, store, good, -3, off, ids) == INV
        for field, value in (("size_x", 0), ("size_y", -1), ("resolution", 0.0), ("resolution", -0.08),
                             ("resolution", float("nan"))):
            bad = _param("hk2").to_c()
            setattr(bad, field, value)
            assert _raw_build(c, store, bad, 4, off, ids) == INV, field
        huge = _param("hk2").to_c()
        huge.size_x, huge.size_y = 65536, 32768  # 2^31 cells
        assert _raw_build(c, store, huge, 4, off, ids) == INV
        blurless = _param("hk2", use_blur=False).to_c()
        assert _raw_build(c, store, blurless, 4, off, ids) == UNS
        # the HIP runtime's count, not torch's: importing torch here loads its own librccl, which the
        # loop-closure handles of later tests in this process would then pick up (ncclCommInitAll fails)
        n_dev = C.c_int(0)
        C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n_dev))
        if n_dev.value > 1:  # a store on another device
            other = ScanStore(1)
            try:
                other.add(scans[0], poses[0])
                assert _raw_build(c, other, good, 1, [0, 1], [0]) == INV
                assert b"another device" in _lib.csm_last_error(c._h)
            finally:
                other.close()
        assert np.array_equal(_u32(_download(c, 4)), _u32(before))
        assert [np.asarray(v).tolist() for v in c.best_windows(cells, p, np.arange(4), centers)] == answer


# ---- 5. lifetime ----------------------------------------------------------------------------------------
def test_cycles_with_a_build_enqueued_at_destroy(small, ctx):
    """Eight create / add / build / destroy cycles; the store is destroyed
    right after the build was enqueued (destroy waits for it)."""
    from roborts_csm.chain_maps import set_grid_stack_chains
    scans, poses, stacks = small
    first = None
    for k in range(8):
        st = _store(scans, poses)
        set_grid_stack_chains(ctx, st, _param("hk7_over1"), R.CHAINS5, R.MAP_OFFSET)
        st.close()
        got = _download(ctx, 5)
        if first is None:
            first = got
            assert np.array_equal(_u32(got), _u32(stacks[("hk7_over1", 5)]))
        assert np.array_equal(_u32(got), _u32(first)), k
