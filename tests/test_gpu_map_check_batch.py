"""GPU: the batched map check (include/csm_map_check.h;
SlamProcessor::MapCheckPenalize, slam_processor.cpp:573-595, over
OccuGridMap::MapFeedbackResponsePenalty, map/occu_grid_map.h:331-392) for many
poses in one launch. Every penalty is compared for equality of every bit, per
pose, with the oracle (pyoracle.GridMap.feedback_penalty, then the logistic in
Python) and with csm_gridmap_feedback_penalty on the same device map; the
counts with the count the coefficient stands for, and on the hand-made maps
with a restatement over the list of occupied cells.

tests/test_map_check_scenario.py shows, without a GPU, that the 24 poses used
here are not trivial on the count_lines map."""
import math

import numpy as np
import pytest

import map_check_cases as K
import map_scenarios as S
from map_engines import DeviceEngine, OracleEngine
from map_pyref import bresenham

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


# ---- references, computed once per map -------------------------------------------
class Built:
    """A scenario's final map on the oracle and on the device, the scans kept
    in a store on the device, and per parameter set the reference penalties."""

    def __init__(self, name, use_blur):
        from roborts_csm.chain_maps import ScanStore
        self.scans_m, self.scans_c, self.poses = K.scans()
        sc = S.scenarios()[name]
        self.oracle, _ = S.run(OracleEngine, sc, self.scans_c, self.poses)
        self.dev, _ = S.run(DeviceEngine, sc, self.scans_c, self.poses)
        self.use_blur = use_blur
        self.check, self.idx = K.check_poses(self.poses)
        self.store = ScanStore(0)
        for k in range(K.N_SCANS):
            assert self.store.add(self.scans_m[k], self.poses[k]) == k
        self.want = {}
        for prm in K.PARAMS:
            o = [self.oracle.penalty(self.scans_c[i], p, *prm, use_blur) for p, i in zip(self.check, self.idx)]
            d = [self.dev.penalty(self.scans_c[i], p, *prm, use_blur) for p, i in zip(self.check, self.idx)]
            assert _bits(o) == _bits(d), (name, prm)  # the single call is the oracle's already
            self.want[prm] = o


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name, use_blur):
        if (name, use_blur) not in cache:
            cache[(name, use_blur)] = Built(name, use_blur)
        return cache[(name, use_blur)]
    return get


def _expect(want, prm, logistic):
    """(penalties, counts) a batch call must return for the reference coefficients."""
    cpn, _, gain = prm
    pens = [K.logistic(c) if logistic else c for c in want]
    counts = [-1 if c == 0.0 else (K.count_of(c, gain, 2 * cpn) if c > 0.1 else None) for c in want]
    return pens, counts


def _assert_same(got, pens, counts, what):
    coeff, cnt = got
    assert _bits(coeff) == _bits(pens), (what, coeff.tolist(), pens)
    for k, c in enumerate(counts):
        if c is not None:  # at the floor the coefficient no longer names one count
            assert cnt[k] == c, (what, k, int(cnt[k]), c)
        else:
            assert cnt[k] >= 0, (what, k)


# the three maps that carry a penalty op: CountCell states, ProbabilityCell
# through the blur offset, ProbabilityCell states
MAPS = [("count_lines", False), ("prob_reset_speedup", True), ("prob_reset_speedup", False)]


@pytest.mark.parametrize("name,use_blur", MAPS)
@pytest.mark.parametrize("logistic", [False, True])
def test_scenario_maps_host_and_store_form(built, name, use_blur, logistic):
    b = built(name, use_blur)
    m = b.dev.m
    n0 = m.map_check_launches()
    seen = set()
    for prm in K.PARAMS:
        pens, counts = _expect(b.want[prm], prm, logistic)
        seen |= {c for c in counts if c is not None}
        host = m.feedback_penalty_batch(b.scans_m, b.check, *prm, use_blur=use_blur, use_logistic=logistic,
                                        scan_index=b.idx)
        _assert_same(host, pens, counts, (name, prm, "host"))
        store = m.feedback_penalty_store(b.store, b.idx, b.check, *prm, use_blur=use_blur, use_logistic=logistic)
        _assert_same(store, pens, counts, (name, prm, "store"))
    assert m.map_check_launches() == n0 + 2 * len(K.PARAMS)  # one launch a call
    if name == "count_lines":
        assert 0 in seen and 1 in seen and max(seen) >= 10, seen


def test_host_form_without_scan_index(built):
    """scan_index NULL: pose k checks scan k."""
    b = built("count_lines", False)
    prm = K.PARAMS[0]
    pens, counts = _expect(b.want[prm][:K.N_SCANS], prm, True)
    got = b.dev.m.feedback_penalty_batch(b.scans_m, b.check[:K.N_SCANS], *prm, use_logistic=True)
    _assert_same(got, pens, counts, "no scan_index")
    from roborts_csm.gridmap import GridMapError
    with pytest.raises(GridMapError):  # n_poses != n_scans without an index
        b.dev.m.feedback_penalty_batch(b.scans_m, b.check[:3], *prm)


def _reference(b, scans_m, poses, idx, prm, use_blur):
    """Oracle and single-call coefficients of (pose k, scan idx[k]), agreed."""
    cells = [np.asarray(s, dtype=np.float64).reshape(-1, 2) * (1 / 0.05) for s in scans_m]
    o = [b.oracle.penalty(cells[i], p, *prm, use_blur) for p, i in zip(poses, idx)]
    d = [b.dev.penalty(cells[i], p, *prm, use_blur) for p, i in zip(poses, idx)]
    assert _bits(o) == _bits(d)
    return o


def test_ray_counts_scan_lengths_and_awkward_points(built):
    """One call with scans of 0 rays (every point in the start cell), 1, 4, 5
    and 53 points, an empty scan, lengths 2 cpn - 1, 2 cpn and 2 cpn + 1, and a
    scan holding a NaN, an infinity and a point no int holds; step 1 and
    step > 1 records side by side."""
    b = built("count_lines", False)
    m = b.dev.m
    full = b.scans_m[1]
    bad = full[:40].copy()
    bad[3] = (math.nan, 1.0)
    bad[7] = (math.inf, -math.inf)
    bad[11] = (1e12, -3e11)
    bad[15] = (2.0, math.nan)
    scans_m = [np.zeros((3, 2)), full[:1], full[100:104], full[60:65], full[:53],
               np.zeros((0, 2)), full[:99], full[:100], full[:101], bad, full]
    for cpn, tol, gain in [(50, 2.5, 0.015), (200, 1.0, 0.05)]:
        poses, idx = [], []
        for i in range(len(scans_m)):
            for p in (b.check[1], b.check[5], b.check[9]):
                poses.append(p)
                idx.append(i)
        want = _reference(b, scans_m, poses, idx, (cpn, tol, gain), False)
        assert want[0] == 1.0 + 2 * gain  # no rays: the count is 0
        for logistic in (False, True):
            pens, counts = _expect(want, (cpn, tol, gain), logistic)
            got = m.feedback_penalty_batch(scans_m, poses, cpn, tol, gain, use_logistic=logistic, scan_index=idx)
            _assert_same(got, pens, counts, ("mixed", cpn, logistic))
    # the same scans from a store: the scan's own step, points read in place
    from roborts_csm.chain_maps import ScanStore
    with ScanStore(0) as st:
        for i, s in enumerate(scans_m):
            assert st.add(s, (0.0, 0.0, 0.0)) == i
        got = m.feedback_penalty_store(st, idx, poses, 200, 1.0, 0.05)
        _assert_same(got, *_expect(want, (200, 1.0, 0.05), False), "mixed store")
        with pytest.raises(Exception):  # an id of no kept scan
            m.feedback_penalty_store(st, [len(scans_m)], [poses[0]], 200, 1.0, 0.05)


def test_300_poses_on_3_scans(built):
    b = built("count_lines", False)
    rng = np.random.default_rng(17)
    idx = rng.integers(0, 3, 300).astype(np.int32)
    poses = np.array([b.poses[i] for i in idx]) + rng.uniform(-1.0, 1.0, (300, 3)) * [0.6, 0.6, 1.0]
    prm = K.PARAMS[0]
    want = _reference(b, b.scans_m[:3], poses, idx, prm, False)
    assert len({c for c in want}) >= 10  # many different answers
    pens, counts = _expect(want, prm, True)
    _assert_same(b.dev.m.feedback_penalty_batch(b.scans_m[:3], poses, *prm, use_logistic=True, scan_index=idx),
                 pens, counts, "300 on 3")
    _assert_same(b.dev.m.feedback_penalty_store(b.store, idx, poses, *prm, use_logistic=True), pens, counts,
                 "300 on 3, store")


def test_kernel_timer_is_apart_from_the_counted_calls(built):
    """The diagnostic times the kernel of a store call without counting a
    launch, leaves the next call's answers alone and refuses guarded arguments."""
    from roborts_csm.gridmap import GridMapError
    b = built("count_lines", False)
    m, prm = b.dev.m, K.PARAMS[0]
    n0 = m.map_check_launches()
    ms = m.feedback_penalty_store_kernel_ms(b.store, b.idx, b.check, *prm, repeats=3)
    assert 0.0 < ms < 50.0 and m.map_check_launches() == n0
    _assert_same(m.feedback_penalty_store(b.store, b.idx, b.check, *prm), *_expect(b.want[prm], prm, False), "after timer")
    with pytest.raises(GridMapError):
        m.feedback_penalty_store_kernel_ms(b.store, b.idx, b.check, 0, 2.5, 0.015)


def test_pose_outside_between_two_inside(built):
    b = built("count_lines", False)
    prm = K.PARAMS[0]
    poses = np.array([b.check[2], [100.0, -100.0, 0.3], b.check[3]])
    for logistic in (False, True):
        out = K.logistic(0.0) if logistic else 0.0
        for got in (b.dev.m.feedback_penalty_batch(b.scans_m, poses, *prm, use_logistic=logistic, scan_index=[2, 2, 3]),
                    b.dev.m.feedback_penalty_store(b.store, [2, 2, 3], poses, *prm, use_logistic=logistic)):
            pens, counts = _expect([b.want[prm][2], 0.0, b.want[prm][3]], prm, logistic)
            assert pens[1] == out and counts == [1, -1, 0]
            _assert_same(got, pens, counts, "outside")
    assert b.oracle.penalty(b.scans_c[2], poses[1], *prm, False) == 0.0


def test_guard_and_rejected_arguments(built):
    from roborts_csm import _abi
    from roborts_csm.gridmap import GridMapError
    b = built("count_lines", False)
    m = b.dev.m
    n0 = m.map_check_launches()
    for cpn, tol, gain in [(0, 2.5, 0.015), (-4, 2.5, 0.015), (50, -0.5, 0.015), (50, 2.5, 0.0), (50, 2.5, 1.0),
                           (50, 2.5, -0.2), (1, -1.0, 0.5)]:
        assert b.oracle.penalty(b.scans_c[0], b.check[0], cpn, tol, gain, False) == 1.0
        for logistic in (False, True):
            one = K.logistic(1.0) if logistic else 1.0
            for coeff, cnt in (m.feedback_penalty_batch(b.scans_m, b.check, cpn, tol, gain, use_logistic=logistic,
                                                        scan_index=b.idx),
                               m.feedback_penalty_store(b.store, b.idx, b.check, cpn, tol, gain, use_logistic=logistic)):
                assert _bits(coeff) == _bits([one] * 24) and cnt.tolist() == [0] * 24
    assert m.map_check_launches() == n0  # the guard launches nothing
    # check_point_num == 1: a one-point scan is checked, two points are the reference's division by zero
    one_pt = [b.scans_m[0][:1]]
    want = _reference(b, one_pt, [b.check[0]], [0], (1, 2.5, 0.5), False)
    _assert_same(m.feedback_penalty_batch(one_pt, [b.check[0]], 1, 2.5, 0.5), *_expect(want, (1, 2.5, 0.5), False), "1/1")
    for call in (lambda: m.feedback_penalty_batch([b.scans_m[0][:2]], [b.check[0]], 1, 2.5, 0.5),
                 lambda: m.feedback_penalty_store(b.store, [0], [b.check[0]], 1, 2.5, 0.5),
                 lambda: m.feedback_penalty_batch(b.scans_m, b.check, 50, 2.5, 0.015, scan_index=[4] * 24)):
        with pytest.raises(GridMapError) as e:
            call()
        assert e.value.status == _abi.CSM_ERR_INVALID_ARG
    # no poses: nothing to do
    coeff, cnt = m.feedback_penalty_batch([], np.zeros((0, 3)), 50, 2.5, 0.015)
    assert coeff.size == 0 and cnt.size == 0


# ---- hand-made CountCell maps with single occupied cells ------------------------
def _hand_maps(size, occ, res=0.5):
    """A size x size CountCell map of `res` m cells at offset 0 whose occupied
    cells are exactly `occ` (one once-per-scan occupied update each, min_pass
    1), on the oracle and on the device."""
    out = []
    for eng in (OracleEngine, DeviceEngine):
        m = eng(1, res, (size, size), (0.0, 0.0), 0.0, 0.5)
        m.set_options(False, True, 0.72, 1.0)
        m.set_cell_params(0.0, 0.0, 0.5, 1.0)
        m.update(np.array(sorted(occ), dtype=np.float64), (0.0, 0.0, 0.0), False)
        out.append(m)
    return out


def _hand_count(size, occ, start, ends, min_d2):
    """The rule restated over the occupied list: rays to ends strictly inside
    the map, not the start cell, that cross an occupied cell at d2 >= min_d2."""
    n = 0
    for ex, ey in ends:
        if (ex, ey) == start or not (0 < ex < size and 0 < ey < size):
            continue
        n += any((x, y) in occ and (ex - x) ** 2 + (ey - y) ** 2 >= min_d2 for x, y in bresenham(*start, ex, ey))
    return n


def _hand_check(size, occ, start, groups, tols):
    """groups: lists of end cells, one scan and one pose (at `start`, angle 0)
    each. Batch, store, single call and oracle against the restated counts."""
    from roborts_csm.chain_maps import ScanStore
    oracle, dev = _hand_maps(size, occ)
    pose = (start[0] * 0.5, start[1] * 0.5, 0.0)  # cell = 2 * metres, exactly
    scans_m = [np.array([((ex - start[0]) * 0.5, (ey - start[1]) * 0.5) for ex, ey in g]).reshape(-1, 2) for g in groups]
    poses = [pose] * len(groups)
    gain, cpn = 0.004, 200  # 1 + 2 gain - count gain stays above the floor: the count is readable
    with ScanStore(0) as st:
        ids = [st.add(s, pose) for s in scans_m]
        for tol, min_d2 in tols:
            want_counts = [_hand_count(size, occ, start, g, min_d2) for g in groups]
            want = [max(1.0 + 2 * gain - float(c) * gain, 0.1) for c in want_counts]
            for g, s, w in zip(groups, scans_m, want):
                cells = s * (1 / 0.5)
                assert oracle.penalty(cells, pose, cpn, tol, gain, False) == w, (tol, g)
                assert dev.penalty(cells, pose, cpn, tol, gain, False) == w, (tol, g)
            coeff, cnt = dev.m.feedback_penalty_batch(scans_m, poses, cpn, tol, gain)
            assert cnt.tolist() == want_counts and _bits(coeff) == _bits(want), (tol, cnt.tolist(), want_counts)
            coeff, cnt = dev.m.feedback_penalty_store(st, ids, poses, cpn, tol, gain)
            assert cnt.tolist() == want_counts and _bits(coeff) == _bits(want), (tol, "store")
    return want_counts


def test_hand_made_map_octants_tolerance_and_borders():
    size, start = 96, (48, 48)
    sx, sy = start
    octants = [(40, 13), (13, 40), (-13, 40), (-40, 13), (-40, -13), (-13, -40), (13, -40), (40, -13)]
    occ = set()
    for k, (dx, dy) in enumerate(octants):  # a cell in the middle of every second octant's ray
        if k % 2 == 0:
            occ.add(bresenham(sx, sy, sx + dx, sy + dy)[20])
    occ |= {(75, 48)}            # d2 = 9 from the end (78, 48)
    occ |= {(57, 75)}            # d2 = 10 from the end (58, 78), on its ray
    assert (57, 75) in bresenham(sx, sy, 58, 78)
    occ |= {(30, 48), (40, 48)}  # two occupied cells on the ray to (18, 48)
    occ |= {(48, 20), (20, 48)}  # on the rays to row 0 / row 1 and column 0 / column 1
    assert start not in occ
    groups = [
        [(sx + dx, sy + dy) for dx, dy in octants],
        [(sx + 1, sy), (sx, sy + 1), (sx - 1, sy), (sx, sy - 1), (sx + 1, sy + 1), (sx - 1, sy - 1)],  # distance 1
        [(78, 48)],                      # occupied at d2 = 9: no hit at tolerance 3.0, a hit at 2.5
        [(58, 78)],                      # occupied at d2 = 10: a hit at tolerance 3.0
        [(18, 48)],                      # two occupied cells: one ray, one hit
        [(108, 48), (48, -3)],           # ends outside the map, past occupied cells
        [(48, 0), (0, 48)],              # ends on row 0 and column 0: PointInMap is strict
        [(48, 1), (1, 48)],              # ends just inside
        [start, start],                  # every point in the start cell: no rays
    ]
    got = _hand_check(size, occ, start, groups, [(3.0, 10), (2.5, 7), (0.0, 1)])
    # at tolerance 0 (the last): four octant rays hit their own cell and the ray to (61, 88) crosses (57, 75),
    # nothing at distance 1, and the designed rays as designed
    assert got == [5, 0, 1, 1, 1, 0, 0, 2, 0]
    assert [_hand_count(size, occ, start, g, 10) for g in groups][2:5] == [0, 1, 1]
    assert [_hand_count(size, occ, start, g, 7) for g in groups][2:5] == [1, 1, 1]


def test_hand_made_map_wave_iteration_boundaries():
    """Ends at distance 63, 64, 65 and 129 cells: one, two and three rounds of
    64 lanes. 129 cells do not fit the 96-cell map, so these rays cross a 192 x
    192 map made the same way. Each ray's only occupied cell is the one next to
    its end, which the lanes reach in their last (or, walking from the end, in
    their first) round."""
    size = 192
    for start, sign in (((31, 31), 1), ((160, 160), -1)):
        groups, occ = [], set()
        for d in (63, 64, 65, 129):
            for dx, dy in ((d, 20), (20, d), (d, d), (d, 0)):  # shallow, steep, diagonal, straight
                end = (start[0] + sign * dx, start[1] + sign * dy)
                line = bresenham(*start, *end)
                assert len(line) == d + 1
                near = line[-2] if line[-1] == end else line[1]
                assert abs(near[0] - end[0]) <= 1 and abs(near[1] - end[1]) <= 1 and near != end
                occ.add(near)
                groups.append([end])
        groups.append([g[0] for g in groups])  # all of them as one pose's scan
        got = _hand_check(size, occ, start, groups, [(0.0, 1), (3.0, 10)])
        assert len(got) == 17


# (x, y) of one point in metres, the pose's angle and x: found by a search on the host so that the end
# cell's column depends on where 1 / resolution is applied (see the test below)
ROUNDING_CASES = [
    ("0x1.d2c2393cca056p+1", "-0x1.32357de331dcfp+1", "0x1.294abc2072d82p-1", "0x1.9d20b1b787ff3p+0"),
    ("0x1.a11a8232c11e8p+1", "-0x1.e5389e6a4fad5p+1", "0x1.b8e771be90748p-1", "0x1.f3c74e615972dp-1"),
    ("0x1.a418d91e7383bp+1", "-0x1.f965f3f188932p+1", "0x1.c11fbfcc05dd6p-1", "0x1.ae68aa71b2000p-1"),
    ("0x1.1f6f6c37e94d4p+2", "-0x1.25b658e17cf67p+1", "0x1.e3cb25b858135p-2", "0x1.dcf98246f215ap-1"),
]


def test_scale_before_rotation_decides_an_end_cell():
    """CreateFrom scales the raw point first (one rounding, sensor_data_manager.h:99-115), then the pose is
    applied. For these four points (raw * f) rotated and (raw rotated) * f differ in the last bit, and the
    pose's x is chosen so that the bit decides between columns 119 and 120 of row 128. The only occupied
    cell is (119, 128): a ray that ends in column 120 passes it at distance 1 (a hit at tolerance 0), a
    ray that ends in it does not count it."""
    from libm import sincos
    from roborts_csm.chain_maps import ScanStore
    res, f, posey = 0.05, 1 / 0.05, 6.4
    oracle, dev = _hand_maps(256, {(119, 128)}, res)
    scans_m, poses, want_counts = [], [], []
    for xs, ys, ths, pxs in ROUNDING_CASES:
        x, y, th, posex = (float.fromhex(v) for v in (xs, ys, ths, pxs))
        c, s = sincos(th)
        tx, ty = f * posex + f * 0.0, f * posey + f * 0.0
        first = int(((c * (x * f) + (-s) * (y * f)) + tx) + 0.5), int(((s * (x * f) + c * (y * f)) + ty) + 0.5)
        after = int(((c * x + (-s) * y) * f + tx) + 0.5), int(((s * x + c * y) * f + ty) + 0.5)
        assert {first, after} == {(119, 128), (120, 128)} and int(ty + 0.5) == 128, (first, after)
        scans_m.append(np.array([[x, y]]))
        poses.append((posex, posey, th))
        want_counts.append(1 if first == (120, 128) else 0)
    assert sorted(want_counts) == [0, 0, 1, 1]
    cpn, tol, gain = 10, 0.0, 0.25
    want = [max(1.0 + 2 * gain - float(k) * gain, 0.1) for k in want_counts]
    for s_m, p, w in zip(scans_m, poses, want):
        assert oracle.penalty(s_m * f, p, cpn, tol, gain, False) == w
        assert dev.penalty(s_m * f, p, cpn, tol, gain, False) == w
    coeff, cnt = dev.m.feedback_penalty_batch(scans_m, poses, cpn, tol, gain)
    assert cnt.tolist() == want_counts and _bits(coeff) == _bits(want)
    with ScanStore(0) as st:
        ids = [st.add(s_m, p) for s_m, p in zip(scans_m, poses)]
        coeff, cnt = dev.m.feedback_penalty_store(st, ids, poses, cpn, tol, gain)
        assert cnt.tolist() == want_counts and _bits(coeff) == _bits(want)


# ---- pending updates, growth -----------------------------------------------------
def test_batch_flushes_pending_updates_and_follows_growth():
    """prob_blur_grow keeps blur endpoints pending until something reads the
    map, and grows from 40 x 40 at its first scan and again at a scan drawn
    from farther away: a batch call straight after each update must see that
    update, also after the map grew."""
    scans_m, scans_c, poses = K.scans()
    sc = S.scenarios()["prob_blur_grow"]
    off = S.map_offset(sc, sc["size"], sc["res"], poses[0])
    maps = []
    for eng in (OracleEngine, DeviceEngine):
        m = eng(sc["kind"], sc["res"], sc["size"], off, sc["dev"], sc["default"])
        m.set_options(*sc["opts"])
        maps.append(m)
    oracle, dev = maps
    check, idx = K.check_poses(poses)
    prm = (30, 2.0, 0.05)
    sizes, answers = [dev.state()["size_x"]], []
    far = np.array([4.0, 3.0, 0.5])  # scans drawn from here make the grown map grow again
    for k, at in [(k, poses[k]) for k in range(K.N_SCANS)] + [(0, poses[0] + far), (1, poses[1] + far)]:
        assert oracle.update(scans_c[k], at, True) == dev.update(scans_c[k], at, True)
        got = dev.m.feedback_penalty_batch(scans_m, check, *prm, use_blur=True, scan_index=idx)  # first: it flushes
        want = [oracle.penalty(scans_c[i], p, *prm, True) for p, i in zip(check, idx)]
        _assert_same(got, *_expect(want, prm, False), ("pending", k))
        assert _bits([dev.penalty(scans_c[i], p, *prm, True) for p, i in zip(check, idx)]) == _bits(want)
        sizes.append(dev.state()["size_x"])
        answers.append(tuple(want))
    assert len(set(sizes)) >= 3 and len(set(answers)) > 2, (sizes, len(set(answers)))  # it grew twice, the answers moved


# ---- loop closure and back end ---------------------------------------------------
def test_loop_closure_map_check_is_the_store_form(built):
    from roborts_csm.loop_closure import DeviceLoopClosure
    b = built("count_lines", False)
    lc = DeviceLoopClosure([0])
    try:
        for k in range(K.N_SCANS):
            assert lc.add_scan(b.scans_m[k], b.poses[k]) == k
        for prm in K.PARAMS[:2]:
            for sid in (2, 3):
                want, _ = b.dev.m.feedback_penalty_store(b.store, [sid] * 24, b.check, *prm, use_logistic=True)
                got = lc.map_check(b.dev.m, sid, b.check, *prm)
                assert _bits(got) == _bits(want), (prm, sid)
        ref = [K.logistic(c) for c in b.want[K.PARAMS[0]][2:3]]
        assert _bits(lc.map_check(b.dev.m, 2, b.check[2:3], *K.PARAMS[0])) == _bits(ref)
        assert lc.map_check(b.dev.m, 2, np.zeros((0, 3)), *K.PARAMS[0]).size == 0
        with pytest.raises(Exception):
            lc.map_check(b.dev.m, 99, b.check, *K.PARAMS[0])
    finally:
        lc.close()


def test_backend_checks_all_jobs_in_one_launch():
    """csm_backend_scan_match over 8 jobs: one map-check launch on the pub map
    (the map's own counter: csm_backend_matcher's contexts are the matchers',
    not the map's), and every job's map_penalty is the single call's at the
    job's final pose, through the logistic."""
    import test_backend as B
    from roborts_csm import worlds
    from roborts_csm.backend import ScanMatchService
    w = worlds.make_world(400, 400, 0.05, seed=8)
    st = worlds.make_scan_stream(w, B.N_SCANS, seed=9)
    kept = B._kept_poses(st)
    jobs = B._jobs(st)
    jobs = jobs + [(q, c, p + np.array([0.02, 0.01, -0.01])) for q, c, p in jobs]
    assert len(jobs) == 8
    prm = B._param("opt")
    svc = ScanMatchService(prm)
    for k in range(B.N_SCANS):
        assert svc.AddRangeData(st.points_m[k], kept[k]) == k
    pub = B._device_pub(w, st, kept)
    n0 = pub.map_check_launches()
    got = svc.scan_match_jobs([st.points_m[q] for q, _, _ in jobs], [c for _, c, _ in jobs], [p for _, _, p in jobs],
                              st.true_poses[-1], pub, True)
    assert pub.map_check_launches() == n0 + 1
    pens = []
    for (q, _, _), r in zip(jobs, got):
        c = pub.MapFeedbackResponsePenalty(st.points_m[q] * (1 / prm.map_resolution), r.pose, prm.map_check_point_num,
                                           prm.map_check_bound_tolerance, prm.map_check_penalty_gain)
        assert r.map_penalty == K.logistic(c), (q, r.map_penalty, c)
        pens.append(r.map_penalty)
    assert len(set(pens)) > 1
    svc.close()
