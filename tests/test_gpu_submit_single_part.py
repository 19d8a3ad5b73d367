"""Submitted batches in one part (csrc/csm_submit_order.hpp,
csm_scan_matchers_submit): the new batch's coarse level, the pending batch's
deferred last launch, the new batch's coarse -> fine hand-off, then the pending
batch's completion: one scoring launch and one fast pass per level over every
window of the batch, where two parts take two.

96 scans of the 2000 x 2000 world at 5 cm with CSM_PIPELINE=16 (as
tests/test_gpu_mixed_batches.py), CSM_SUBMIT_PARTS=1, the coarse level in one
launch (CSM_FIRST_WINDOWS=0) and in spans of 5, 20 and 71 windows (5). Each
case against scan_matchers_loaded (the synchronous two-part driver) and
against the CPU oracle, bit for bit: scores, poses, covariances.

  a  one batch, then wait
  b  four batches back to back, different scans and initial poses, queued
     with load_scans_async (the pending batch's last launch runs on its own,
     parked, points)
  c  single-part (headline levels), two-part (the sim YAML's B = 109 levels,
     by the rule) and synchronous-fallback (10 scans) batches alternating in
     one context
  d  a wait, and a scan_matchers_loaded, between two submits
  e  beam counts 512 | 513 in one batch
  f  the quantised map: every level has windows in the exact pass

kernel_stats() of a profiled run shows one scoring launch per level and batch
plus the coarse level's spans (three launches of the coarse kernel a batch at
CSM_FIRST_WINDOWS=5, listed again under "span2:") and finish:separate<n> once
per level and batch over all 96 windows. A context destroyed with a single-part
batch pending leaves no error behind."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402

N_SCANS = 96
SMALL = 10  # scans of the synchronous-fallback batch (under CSM_PIPELINE=16)
SINGLE = {"CSM_PIPELINE": "16", "CSM_SUBMIT_PARTS": "1"}
RULE = {"CSM_PIPELINE": "16"}  # CSM_SUBMIT_PARTS unset, by the rule: headline one part, B = 109 two
SYNC = {"CSM_PIPELINE": "16", "CSM_FIRST_WINDOWS": "0"}  # scan_matchers_loaded: the two-part synchronous driver
FACTORS = (1.0, 0.995, 1.005, 0.99)


def _levels(which):
    from roborts_csm.params import SIM_YAML_LEVELS, headline_levels
    return headline_levels() if which == "headline" else SIM_YAML_LEVELS


@pytest.fixture(scope="module")
def world():
    from roborts_csm import worlds
    w = worlds.make_world(2000, 2000, 0.05)
    b = worlds.make_scan_batch(w, N_SCANS, seed=99)
    grid = np.asarray(w.grid, dtype=np.float32)
    grids = {"float": grid, "quantised": np.round(grid * 2.0).astype(np.float32) / np.float32(2.0)}
    rng = np.random.default_rng(5)
    # four batches: the scans scaled, the initial poses moved (0: as generated)
    batches = []
    for k, f in enumerate(FACTORS):
        init = b.init_poses + (rng.uniform(-1, 1, size=(N_SCANS, 3)) * [0.03, 0.03, 0.01] if k else 0.0)
        batches.append((np.ascontiguousarray(b.points_cells * f), b.offsets.copy(), np.ascontiguousarray(init)))
    # 512 | 513 beams alternating (the headline levels sum every beam)
    scans = []
    for k in range(N_SCANS):
        p = b.points_cells[b.offsets[k]:b.offsets[k + 1]]
        n = 512 + (k & 1)
        q = p[::p.shape[0] // n][:n]
        assert q.shape[0] == n
        scans.append(q)
    off = np.zeros(N_SCANS + 1, dtype=np.int64)
    off[1:] = np.cumsum([s.shape[0] for s in scans])
    edge = (np.ascontiguousarray(np.concatenate(scans, axis=0)), off, np.ascontiguousarray(b.init_poses.copy()))
    O.set_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    yield {"w": w, "grids": grids, "batches": batches, "edge": edge, "oracle": {}, "loaded": {}}
    O.set_threads(1)


def _input(world, which):
    return world["edge"] if which == "edge" else world["batches"][which]


def _oracle(world, kind, which, levels):
    """The oracle's answer for a batch on a map, computed once and left unchanged."""
    key = (kind, which, levels)
    if key not in world["oracle"]:
        w = world["w"]
        pts, off, init = _input(world, which)
        m = O.Map(world["grids"][kind], w.resolution, w.offset)
        r = O.scan_matchers_batch(m, pts, off, _levels(levels), init, np.tile(np.eye(3).reshape(1, 9), (N_SCANS, 1)))
        for a in r:
            a.setflags(write=False)
        world["oracle"][key] = r
    return world["oracle"][key]


def _context(world, kind, env):
    import roborts_csm
    w = world["w"]
    assert not any(k.startswith("CSM_") for k in os.environ)
    os.environ.update(env)
    try:
        c = roborts_csm.Context(0)
    finally:
        for k in env:
            del os.environ[k]
    c.set_grid(roborts_csm.ScanMatchMap(world["grids"][kind], float(w.resolution), tuple(w.offset), 0, 1))
    return c


def _fresh(init, n=N_SCANS):
    return np.zeros(n), np.ascontiguousarray(init[:n].copy()), np.tile(np.eye(3).reshape(1, 9), (n, 1))


def _loaded(world, kind, which, levels):
    """scan_matchers_loaded's answer (the synchronous driver), once per batch, checked against the oracle."""
    key = (kind, which, levels)
    if key not in world["loaded"]:
        pts, off, init = _input(world, which)
        c = _context(world, kind, SYNC)
        try:
            _, poses, covs = _fresh(init)
            c.load_scans(pts, off)
            s = c.scan_matchers_loaded(_levels(levels), poses, covs)
        finally:
            c.close()
        _same((s, poses, covs), _oracle(world, kind, which, levels), ("loaded", key))
        world["loaded"][key] = (s, poses, covs)
    return world["loaded"][key]


def _same(got, want, what, n=None):
    for a, e, nm in zip(got, want, ("scores", "poses", "covariances")):
        e = e if n is None else e[:n]
        bad = np.flatnonzero(np.any(np.atleast_2d(a.T != e.T), axis=0))
        assert np.array_equal(a, e), (what, nm, bad[:8].tolist(), len(bad))


def _check(world, kind, which, levels, got, what, n=None):
    _same(got, _loaded(world, kind, which, levels), (what, "against scan_matchers_loaded"), n)
    _same(got, _oracle(world, kind, which, levels), (what, "against the oracle"), n)


def _single_part_stats(st, batches, fw):
    """One scoring launch and one separate fast pass per level and batch, over all 96 windows."""
    score = {n: k for n, k in st.items() if n.startswith("score_")}
    sep = {n: k for n, k in st.items() if n.startswith("finish:separate<")}
    fused = [n for n in st if n.startswith("finish:fused<")]
    print({n: (k["launches"], k["scorings"]) for n, k in {**score, **sep}.items()},
          {n: k["launches"] for n, k in st.items() if n.startswith("span2:")})
    assert len(score) == 3 and len(sep) == 3 and not fused, (sorted(score), sorted(sep), fused)
    # the coarse level of 96 windows in spans of 5, 20 and 71 (level_begin_split: first 5, growth 4, the
    # last span takes the rest): three scoring launches, listed again as a multi-dispatch level
    spans = 3 if fw else 1
    for n, k in score.items():
        want = batches * (spans if n.startswith("score_box_pair_kernel<13,") else 1)
        assert k["launches"] == want, (n, k["launches"], want)
    for n, k in sep.items():
        assert k["launches"] == batches and k["scorings"] == batches * N_SCANS, (n, k)
    span2 = {n: k["launches"] for n, k in st.items() if n.startswith("span2:")}
    assert span2 == ({"span2:score_box_pair_kernel<13,all>": batches * 3} if fw else {}), (span2, batches, fw)
    # part 0 only: no wait of a second part
    assert not any(n.startswith("host:wait<") and n.endswith(",p1>") for n in st), sorted(st)
    assert sum(k["launches"] for n, k in st.items() if n.startswith("host:wait<")) == 3 * batches


def _env(base, fw):
    return dict(base, CSM_FIRST_WINDOWS=str(fw))


@pytest.mark.parametrize("fw", [0, 5])
def test_one_batch_then_wait(world, fw):
    """(a), and (d)'s wait: a single-part batch completed by wait, profiled, then another after it."""
    c = _context(world, "float", _env(SINGLE, fw))
    try:
        c.set_profiling(True)
        for which in (0, 1):
            pts, off, init = _input(world, which)
            got = _fresh(init)
            c.load_scans(pts, off)
            c.scan_matchers_submit(_levels("headline"), got[1], got[2], got[0])
            c.scan_matchers_wait()
            _check(world, "float", which, "headline", got, ("one batch", fw, which))
        st = {k["name"]: k for k in c.kernel_stats()}
        c.set_profiling(False)
        _single_part_stats(st, 2, fw)
    finally:
        c.close()


def _back_to_back(world, kind, env, seq, profile=False):
    """Batches seq = [(which, levels, n_scans)] queued from pinned memory and
    submitted back to back; returns the outputs and the stats."""
    import roborts_csm
    c = _context(world, kind, env)
    pins = {}
    try:
        for which, _, n in seq:
            if (which, n) not in pins:
                pts, off, _ = _input(world, which)
                pin = roborts_csm.PinnedArray((int(off[n]), 2))
                np.copyto(pin.array, pts[:off[n]])
                pins[(which, n)] = (pin, off[:n + 1].copy())
        got = [_fresh(_input(world, which)[2], n) for which, _, n in seq]
        if profile:
            c.set_profiling(True)

        def queue(k):
            pin, off = pins[(seq[k][0], seq[k][2])]
            c.load_scans_async(pin.array, off)

        queue(0)
        for k, (which, levels, n) in enumerate(seq):
            if k + 1 < len(seq):
                queue(k + 1)
            c.scan_matchers_submit(_levels(levels), got[k][1], got[k][2], got[k][0])
        c.scan_matchers_wait()
        st = {k["name"]: k for k in c.kernel_stats()} if profile else None
        return got, st
    finally:
        c.close()
        for pin, _ in pins.values():
            pin.close()


@pytest.mark.parametrize("fw", [0, 5])
def test_four_batches_back_to_back(world, fw):
    """(b): each batch's deferred last launch goes out inside the next submit,
    after that batch's points were parked: it must still read its own."""
    seq = [(k, "headline", N_SCANS) for k in range(4)]
    got, st = _back_to_back(world, "float", _env(SINGLE, fw), seq, profile=True)
    for k, (which, levels, n) in enumerate(seq):
        _check(world, "float", which, levels, got[k], ("back to back", fw, k))
    _single_part_stats(st, 4, fw)


@pytest.mark.parametrize("fw", [0, 5])
def test_single_two_part_and_synchronous_batches_alternate(world, fw):
    """(c): by the rule the headline batches take one part and the B = 109
    batches two; the 10-scan batches complete inside their submit. Every
    neighbour pair occurs: one part after two and two after one, the fallback
    after and before each."""
    seq = [(0, "headline", N_SCANS), (1, "sim", N_SCANS), (2, "headline", N_SCANS), (3, "headline", SMALL),
           (1, "sim", N_SCANS), (0, "sim", SMALL), (3, "headline", N_SCANS), (2, "headline", N_SCANS),
           (0, "sim", N_SCANS)]
    got, st = _back_to_back(world, "float", _env(RULE, fw), seq, profile=True)
    for k, (which, levels, n) in enumerate(seq):
        _check(world, "float", which, levels, got[k], ("alternating", fw, k, levels, n), n if n < N_SCANS else None)
    # the driver's waits by (level, part): 4 single-part and 3 two-part batches went through it
    # (the 10-scan batches' levels run one after the other, outside it)
    waits = {n: k["launches"] for n, k in st.items() if n.startswith("host:wait<")}
    print(waits)
    assert waits == {f"host:wait<l{l},p{p}>": (7, 3)[p] for l in range(3) for p in range(2)}, waits
    # headline levels keep the separate fast pass, one per level of each single-part batch;
    # the B = 109 levels finish inside their scoring launches, once per part
    sep = {n: k["launches"] for n, k in st.items() if n.startswith("finish:separate<")}
    fused = {n: k["launches"] for n, k in st.items() if n.startswith("finish:fused<")}
    print(sep, fused)
    assert len(sep) == 3 and all(v == 4 for v in sep.values()), sep
    assert len(fused) == 3 and all(v == 3 * 2 for v in fused.values()), fused


def test_wait_and_loaded_between_submits(world):
    """(d): a synchronous call between two single-part submits completes the
    pending batch first and leaves the next submit nothing to finish."""
    c = _context(world, "float", _env(SINGLE, 5))
    try:
        lv = _levels("headline")
        p0, o0, i0 = _input(world, 0)
        p1, o1, i1 = _input(world, 1)
        p2, o2, i2 = _input(world, 2)
        a, b, d, e = _fresh(i0), _fresh(i1), _fresh(i2), _fresh(i0)
        c.load_scans(p0, o0)
        c.scan_matchers_submit(lv, a[1], a[2], a[0])
        c.load_scans(p1, o1)  # completes the pending batch
        _check(world, "float", 0, "headline", a, "submit, then load_scans")
        s = c.scan_matchers_loaded(lv, b[1], b[2])
        _check(world, "float", 1, "headline", (s, b[1], b[2]), "scan_matchers_loaded in between")
        c.load_scans(p2, o2)
        c.scan_matchers_submit(lv, d[1], d[2], d[0])
        c.scan_matchers_wait()
        _check(world, "float", 2, "headline", d, "submit after scan_matchers_loaded")
        c.load_scans(p0, o0)
        c.scan_matchers_submit(lv, e[1], e[2], e[0])
        c.scan_matchers_wait()
        _check(world, "float", 0, "headline", e, "submit after wait")
    finally:
        c.close()


@pytest.mark.parametrize("fw", [0, 5])
def test_beam_counts_512_and_513_in_one_batch(world, fw):
    """(e): scans on both sides of the fused finish's threshold in one
    single-part level: the level decides once, for all 96 windows (513 beams:
    the separate fast pass)."""
    seq = [("edge", "headline", N_SCANS), (1, "headline", N_SCANS), ("edge", "headline", N_SCANS)]
    got, st = _back_to_back(world, "float", _env(SINGLE, fw), seq, profile=True)
    for k, (which, levels, n) in enumerate(seq):
        _check(world, "float", which, levels, got[k], ("512 | 513", fw, k))
    _single_part_stats(st, 3, fw)


def test_quantised_map_exact_pass_every_level(world):
    """(f): on the three-valued map ties send windows of every level to the
    exact pass on its own stream, which now runs beside the other batch's next
    scoring launch."""
    seq = [(0, "headline", N_SCANS), (1, "headline", N_SCANS), (2, "headline", N_SCANS)]
    got, st = _back_to_back(world, "quantised", _env(SINGLE, 5), seq, profile=True)
    for k, (which, levels, n) in enumerate(seq):
        _check(world, "quantised", which, levels, got[k], ("quantised", k))
    _single_part_stats(st, 3, 5)
    ex = [k for n, k in st.items() if n.startswith("finish:exact_windows<")]
    assert len(ex) == 3 and all(k["scorings"] > 0 for k in ex), ex


def test_destroy_with_single_part_batch_pending(world):
    """A context closed with a single-part batch pending: the batch is
    completed (its outputs are final and right), nothing is left in error, and
    the next context works."""
    pts, off, init = _input(world, 0)
    got = _fresh(init)
    c = _context(world, "float", _env(SINGLE, 5))
    try:
        c.load_scans(pts, off)
        c.scan_matchers_submit(_levels("headline"), got[1], got[2], got[0])
    finally:
        c.close()
    _check(world, "float", 0, "headline", got, "destroyed while pending")
    c = _context(world, "float", _env(SINGLE, 5))
    try:
        again = _fresh(init)
        c.load_scans(pts, off)
        c.scan_matchers_submit(_levels("headline"), again[1], again[2], again[0])
        c.scan_matchers_wait()
        _check(world, "float", 0, "headline", again, "the next context")
    finally:
        c.close()
