"""GPU parity for batches whose scans differ in length: the kernels and the
3-level driver choose their form from beam counts (the pair kernel's run-free
form and the phase kernel's short form up to 128 beams, the fused finish up to
512, the fixed-point kernels inside a range of the map), and a real sensor
hands over scans on both sides of each threshold in one batch. Homogeneous
batches exactly at 128 | 129 and 512 | 513 beams, heterogeneous batches in one
launch and in spans (level_begin_split, the split hand-off), and short, mixed
and long batches alternating in one context: each against the CPU oracle bit
for bit (scores, poses, covariances), on the float map and on the map
quantised to three values, where every level's exact pass has windows.

A level sent out in spans must reach one decision (csm_level_decision.hpp);
tests/test_level_decision.py checks the decision itself on the host, the span
cases here check what the device then computes.

The 2000 x 2000 world at 5 cm, 96 scans, the headline levels (every beam:
U = 1081, so a scan shortened to n points sums n beams) unless stated."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

N_SCANS = 96
SPANS = {"CSM_PIPELINE": "16", "CSM_PIPELINE_PARTS": "2", "CSM_FIRST_WINDOWS": "5", "CSM_SPLIT_HANDOFF_MIN": "8"}
ONE = {"CSM_PIPELINE": "16", "CSM_PIPELINE_PARTS": "2", "CSM_FIRST_WINDOWS": "0"}
FULL = 1 << 20  # a beam count: the scan as it is


# ---- the driver's split and window order, restated (csm_pipeline.cpp job_setup, window_order;
# csm_level.cpp level_begin_split, level_end_begin) -----------------------------------------

def _parts(n, permille=550):
    """job_setup, two parts: part 0 takes permille of the scans (550; 500 for submitted batches)."""
    n0 = n * permille // 1000
    return [(0, n0), (n0, n)]


def _spread(v):
    v &= 0xFFFF
    v = (v | (v << 8)) & 0x00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F
    v = (v | (v << 2)) & 0x33333333
    v = (v | (v << 1)) & 0x55555555
    return v


def _window_order(m, poses):
    """window_order: a part's scans ranked by the Morton code of their initial
    map cell's 64-cell tile (stable: ties in scan order), rank r at launch
    position (r % 8) * n / 8 + r / 8."""
    keys = []
    for p in poses:
        c = O.world_to_map(m, p)
        q = [int(max(-32768.0, min(32767.0, np.floor(c[k] / 64.0)))) + 32768 for k in (0, 1)]
        keys.append(_spread(q[0]) | (_spread(q[1]) << 1))
    rank = np.argsort(np.array(keys, dtype=np.uint64), kind="stable")
    return [int(rank[r]) for x in range(8) for r in range(x, len(poses), 8)]


def _windows(m, init_poses, counts, permille=550):
    """Each part's windows as global scan numbers, in launch order (empty scans have none)."""
    out = []
    for lo, hi in _parts(len(counts), permille):
        out.append([lo + s for s in _window_order(m, init_poses[lo:hi]) if counts[lo + s] > 0])
    return out


def _spans(nw, first=5, growth=4):
    """level_begin_split's scoring spans (it sends one launch when nw < 2 * first)."""
    if first <= 0 or nw < 2 * first:
        return [(0, nw)]
    out, w0, sz = [], 0, first
    while w0 < nw:
        w1 = nw if nw - w0 <= 2 * sz else w0 + sz
        out.append((w0, w1))
        w0, sz = w1, sz * max(2, growth)
    return out


def test_restated_spans():
    assert _spans(52) == [(0, 5), (5, 25), (25, 52)]
    assert _spans(9) == [(0, 9)] and _spans(10) == [(0, 10)] and _spans(16) == [(0, 5), (5, 16)]
    assert _parts(96) == [(0, 52), (52, 96)] and _parts(96, 500) == [(0, 48), (48, 96)]


# ---- inputs -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def world():
    from roborts_csm import worlds
    w = worlds.make_world(2000, 2000, 0.05)
    b = worlds.make_scan_batch(w, N_SCANS, seed=99)
    grid = np.asarray(w.grid, dtype=np.float32)
    grids = {"float": grid, "quantised": np.round(grid * 2.0).astype(np.float32) / np.float32(2.0)}
    O.set_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    yield w, b, grids
    O.set_threads(1)


def _take(p, n):
    """n of a scan's points, spread over the scan (pts[::k][:n]); FULL: all of them."""
    if n >= FULL:
        return p
    if n == 0:
        return p[:0]
    assert n <= p.shape[0], (n, p.shape[0])
    q = p[::p.shape[0] // n][:n]
    assert q.shape[0] == n
    return q


def _batch(b, counts):
    """The batch with scan k shortened to counts[k] points: (points, offsets, sizes)."""
    scans = [_take(b.points_cells[b.offsets[k]:b.offsets[k + 1]], counts[k]) for k in range(N_SCANS)]
    off = np.zeros(N_SCANS + 1, dtype=np.int64)
    off[1:] = np.cumsum([s.shape[0] for s in scans])
    return np.ascontiguousarray(np.concatenate(scans, axis=0)), off, np.diff(off)


_oracle_cache = {}


def _oracle(world, kind, key, pts, off, levels, init):
    """The oracle's answer for a batch, computed once per module and left unchanged."""
    w, _, grids = world
    k = (kind, key)
    if k not in _oracle_cache:
        m = O.Map(grids[kind], w.resolution, w.offset)
        eye = np.tile(np.eye(3).reshape(1, 9), (N_SCANS, 1))
        r = O.scan_matchers_batch(m, pts, off, levels, init, eye)
        for a in r:
            a.setflags(write=False)
        _oracle_cache[k] = r
    return _oracle_cache[k]


def _context(world, kind, env):
    import roborts_csm
    w, _, grids = world
    assert not any(k.startswith("CSM_") for k in os.environ)
    os.environ.update(env)
    try:
        c = roborts_csm.Context(0)
    finally:
        for k in env:
            del os.environ[k]
    c.set_grid(roborts_csm.ScanMatchMap(grids[kind], float(w.resolution), tuple(w.offset), 0, 1))
    return c


def _run(c, pts, off, levels, init, stats=False):
    poses = np.ascontiguousarray(init.copy())
    covs = np.tile(np.eye(3).reshape(1, 9), (N_SCANS, 1))
    if stats:
        c.set_profiling(True)
    s = c.scan_matchers_batch(pts, off, levels, poses, covs)
    st = None
    if stats:
        st = {k["name"]: k for k in c.kernel_stats()}
        c.set_profiling(False)
    return (s, poses, covs), st


def _same(got, want, what):
    for a, e, nm in zip(got, want, ("scores", "poses", "covariances")):
        bad = np.flatnonzero(np.any(np.atleast_2d(a.T != e.T), axis=0))
        assert np.array_equal(a, e), (what, nm, bad[:8].tolist(), len(bad))


def _finishes(st):
    """How the levels' fast finishes ran: (fused, separate) launches, from kernel_stats()."""
    fused = sum(k["launches"] for n, k in st.items() if n.startswith("finish:fused<"))
    sep = sum(k["launches"] for n, k in st.items() if n.startswith("finish:separate<"))
    fast = {n: round(k["total_ms"], 4) for n, k in st.items() if n.startswith("finish:fast<")}
    print("finish: fused", fused, "separate", sep, "fast pass ms", fast)
    return fused, sep


def _levels(which="headline"):
    from roborts_csm.params import SIM_YAML_LEVELS, headline_levels
    return headline_levels() if which == "headline" else SIM_YAML_LEVELS


# ---- a. homogeneous batches at each edge ---------------------------------------------------

@pytest.mark.parametrize("kind", ["float", "quantised"])
@pytest.mark.parametrize("mode", ["one", "spans"])
@pytest.mark.parametrize("beams", [128, 129, 512, 513])
def test_homogeneous_batch_at_threshold(world, beams, mode, kind):
    """Every scan sums exactly `beams` beams: the last count of the short
    kernel forms and the first of the long ones (128 | 129), the last level
    that finishes its windows inside the scoring launches and the first that
    keeps the separate fast pass (512 | 513), one launch per level and in
    spans. 2 parts x 3 levels: six finishes, all fused or all separate."""
    _, b, _ = world
    pts, off, sizes = _batch(b, [beams] * N_SCANS)
    assert np.all(sizes == beams)
    want = _oracle(world, kind, ("homog", beams), pts, off, _levels(), b.init_poses)
    c = _context(world, kind, ONE if mode == "one" else SPANS)
    try:
        got, st = _run(c, pts, off, _levels(), b.init_poses, stats=True)
        _same(got, want, (beams, mode, kind))
        assert _finishes(st) == ((6, 0) if beams <= 512 else (0, 6))
        got, _ = _run(c, pts, off, _levels(), b.init_poses)  # once more, unprofiled
        _same(got, want, (beams, mode, kind, "again"))
    finally:
        c.close()


# ---- b. heterogeneous batches in one launch ------------------------------------------------

MIXED = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, FULL]
SHORT = [1, 2, 3, 31, 63, 64, 65, 100, 127, 128]
SIM_EDGE = [150, 199, 200, 255, 256, 257, FULL]  # U = 100: the beam rule's own edge at 2U


def _cycle(vals, shift=0):
    return [vals[(k + shift) % len(vals)] for k in range(N_SCANS)]


@pytest.mark.parametrize("kind", ["float", "quantised"])
@pytest.mark.parametrize("parts", [False, True])
@pytest.mark.parametrize("mix", ["mixed", "short", "sim_edge"])
def test_heterogeneous_batch_one_launch(world, mix, parts, kind):
    """Scans on both sides of every threshold in one launch per level
    (CSM_FIRST_WINDOWS=0; all 96 windows, or two parts): beam counts 1 ...
    full; at most 128 beams with 1- and 2-beam scans (the short forms at their
    lower edge); the sim YAML's U = 100 with point counts around 2U."""
    _, b, _ = world
    counts = _cycle({"mixed": MIXED, "short": SHORT, "sim_edge": SIM_EDGE}[mix])
    levels = _levels("sim" if mix == "sim_edge" else "headline")
    pts, off, sizes = _batch(b, counts)
    assert set(c for c in counts if c < FULL) <= set(sizes.tolist())
    want = _oracle(world, kind, ("cycle", mix), pts, off, levels, b.init_poses)
    env = dict(ONE) if parts else {"CSM_FIRST_WINDOWS": "0"}
    c = _context(world, kind, env)
    try:
        got, st = _run(c, pts, off, levels, b.init_poses, stats=True)
        _same(got, want, (mix, parts, kind))
        n = 6 if parts else 3
        # sim_edge: 199 points under 2U sum 199 beams, all others at most 150
        assert _finishes(st) == ((0, n) if mix == "mixed" else (n, 0))
    finally:
        c.close()


# ---- c. heterogeneous batches in spans -----------------------------------------------------

def _far_pose(world, kind, pose):
    """A pose whose windows are out of the fixed-point range on any grid of
    this width: int_mode_window_ok needs (|points| + reach + 2) * 4 * pitch <
    2^30 with pitch >= 2000 cells and reach >= |x0| (x0: the window's start,
    half the 0.6 m search size before the pose's map cell). Checked through
    the oracle's world -> map arithmetic."""
    w, _, grids = world
    m = O.Map(grids[kind], w.resolution, w.offset)
    far = np.array(pose, dtype=np.float64)
    far[0] += 7000.0  # metres: 140000 cells at 5 cm
    x0 = O.world_to_map(m, far)[0] - (0.6 / w.resolution) * 0.5
    assert (abs(x0) + 2.0) * 4.0 * 2000.0 >= 2.0 ** 30 and grids[kind].shape[1] == 2000
    return far


def _arrangement(world, kind, name):
    """(counts, init_poses) with scans of chosen lengths at chosen windows, and
    the precondition asserted from the restated order."""
    w, b, grids = world
    m = O.Map(grids[kind], w.resolution, w.offset)
    init = b.init_poses.copy()
    counts = [128] * N_SCANS
    far = []
    if name == "out_of_range":  # the far scans change the order: placed first
        order = _windows(m, init, counts)
        far = [order[0][9], order[1][30]]
        for s in far:
            init[s] = _far_pose(world, kind, init[s])
    W = _windows(m, init, counts)
    assert [len(x) for x in W] == [52, 44]
    sp0, half1 = _spans(len(W[0])), len(W[1]) // 2
    assert sp0[0] == (0, 5) and len(sp0) == 3 and half1 >= 8 // 2
    if name == "short_first":  # part 0's first span short, a later window long
        counts[W[0][7]] = FULL
        counts[W[0][30]] = 513
        for k, s in enumerate(W[1]):
            counts[s] = (512, 300, 128)[k % 3]
        assert all(counts[s] <= 512 for s in W[0][:5]) and max(counts[s] for s in W[0][5:]) > 512
    elif name == "short_first_handoff":  # the last part's first half short, its second half long
        counts[W[1][30]] = FULL
        counts[W[1][3]] = 512
        assert all(counts[s] <= 512 for s in W[1][:half1]) and max(counts[s] for s in W[1][half1:]) > 512
        assert all(counts[s] <= 512 for s in W[0])
    elif name == "long_first":  # a long scan in the first span, the rest short
        counts[W[0][2]] = FULL
        assert max(counts[s] for s in W[0][:5]) > 512 and all(counts[s] <= 128 for s in W[0][5:] + W[1])
    elif name == "straddle_128":  # the first span at most 128 beams, later windows 129-512
        for k, n in enumerate((128, 64, 127, 2, 128)):
            counts[W[0][k]] = n
        counts[W[0][6]], counts[W[0][20]], counts[W[0][40]] = 129, 512, 300
        counts[W[1][1]], counts[W[1][25]] = 128, 129
        assert all(counts[s] <= 128 for s in W[0][:5]) and all(counts[s] <= 128 for s in W[1][:half1])
        assert 128 < max(counts[s] for s in W[0][5:]) <= 512 and 128 < max(counts[s] for s in W[1][half1:]) <= 512
    elif name == "out_of_range":  # in range first, a later scan far outside the map (both parts)
        assert W[0].index(far[0]) >= 5 and W[1].index(far[1]) >= half1
        counts[W[0][12]] = 512
    elif name == "empty_tiny":  # one empty scan and one 1-point scan among full ones
        counts = [FULL] * N_SCANS
        counts[W[0][1]] = 1
        counts[W[0][3]] = 0
        W = _windows(m, init, counts)
        assert len(W[0]) == 51 and counts[W[0][1]] == 1 and _spans(51)[0] == (0, 5)
    else:
        raise KeyError(name)
    return counts, init


@pytest.fixture(scope="module")
def one_launch_ctx(world):
    """One context per map with one launch per level, for every arrangement."""
    cs = {}

    def get(kind):
        if kind not in cs:
            cs[kind] = _context(world, kind, ONE)
        return cs[kind]

    yield get
    for c in cs.values():
        c.close()


@pytest.mark.parametrize("kind", ["float", "quantised"])
@pytest.mark.parametrize("name", ["short_first", "short_first_handoff", "long_first", "straddle_128", "out_of_range",
                                  "empty_tiny"])
def test_heterogeneous_batch_in_spans(world, one_launch_ctx, name, kind):
    """The first part's coarse level in spans of 5, 20 and 27 windows and the
    last part's hand-off to the super-fine level in two halves, with the scans
    that decide the level's kernels and its finish placed before or after the
    first span: the result is the oracle's and the one-launch level's, three
    times over, and a fused-finish batch (128 beams) and a full-length batch
    that follow in the same context are right too: no counter was left
    part-counted, no window listed twice."""
    _, b, _ = world
    counts, init = _arrangement(world, kind, name)
    pts, off, sizes = _batch(b, counts)
    want = _oracle(world, kind, ("arr", name), pts, off, _levels(), init)
    one, st1 = _run(one_launch_ctx(kind), pts, off, _levels(), init, stats=True)
    _same(one, want, (name, kind, "one launch"))
    p128, o128, _ = _batch(b, [128] * N_SCANS)
    w128 = _oracle(world, kind, ("homog", 128), p128, o128, _levels(), b.init_poses)
    pful, oful, _ = _batch(b, [FULL] * N_SCANS)
    wful = _oracle(world, kind, ("homog", FULL), pful, oful, _levels(), b.init_poses)
    c = _context(world, kind, SPANS)
    try:
        for it in range(3):
            got, st = _run(c, pts, off, _levels(), init, stats=(it == 0))
            _same(got, want, (name, kind, "spans", it))
            if it == 0:  # every level finished as the one-launch level's did
                assert _finishes(st) == _finishes(st1)
        got, st = _run(c, p128, o128, _levels(), b.init_poses, stats=True)
        _same(got, w128, (name, kind, "then 128 beams"))
        assert _finishes(st) == (6, 0)
        got, st = _run(c, pful, oful, _levels(), b.init_poses, stats=True)
        _same(got, wful, (name, kind, "then full scans"))
        assert _finishes(st) == (0, 6)
    finally:
        c.close()


# ---- d. alternation in one context ---------------------------------------------------------

@pytest.mark.parametrize("kind", ["float", "quantised"])
@pytest.mark.parametrize("settings", ["defaults", "spans"])
def test_alternating_batches_in_one_context(world, settings, kind):
    """Six batches queued (csm_load_scans_async) and submitted back to back:
    all short (at most 128 beams), mixed, all long, twice over, so fused-finish
    and fast-pass levels alternate in one context's buffers and counters; each
    batch against its own oracle answer."""
    import roborts_csm
    _, b, _ = world
    batches = []
    for mix, counts in (("short", _cycle(SHORT)), ("mixed", _cycle(MIXED)), ("long", [FULL] * N_SCANS)):
        pts, off, _ = _batch(b, counts)
        key = ("homog", FULL) if mix == "long" else ("cycle", mix)
        batches.append((pts, off, _oracle(world, kind, key, pts, off, _levels(), b.init_poses)))
    seq = [0, 1, 2, 0, 1, 2]
    c = _context(world, kind, SPANS if settings == "spans" else {})
    pins = []
    try:
        for pts, _, _ in batches:
            pins.append(roborts_csm.PinnedArray(pts.shape))
            np.copyto(pins[-1].array, pts)
        eye = np.tile(np.eye(3).reshape(1, 9), (N_SCANS, 1))
        got = [(np.zeros(N_SCANS), np.ascontiguousarray(b.init_poses.copy()), eye.copy()) for _ in seq]
        c.load_scans_async(pins[seq[0]].array, batches[seq[0]][1])
        for k, which in enumerate(seq):
            if k + 1 < len(seq):
                c.load_scans_async(pins[seq[k + 1]].array, batches[seq[k + 1]][1])
            c.scan_matchers_submit(_levels(), got[k][1], got[k][2], got[k][0])
        c.scan_matchers_wait()
        for k, which in enumerate(seq):
            _same(got[k], batches[which][2], (settings, kind, k))
    finally:
        c.close()
        for p in pins:
            p.close()
