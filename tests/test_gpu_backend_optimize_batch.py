"""The batched back end with the Gauss-Newton matcher on (ParamConfig's default
use_optimize_scan_match): csm_backend_scan_match runs the matcher of all jobs
in one launch over a stack of the coarse maps, splits the jobs by the
reference's test (!use_fine || cost > optimize_failed_cost, scan_matchers.h:224)
and runs each group's correlative levels as one batch over a stack of the
fine maps. test_backend.py's drive; every job's pose, covariance, score,
penalty and optimiser cost equal the oracle's bit for bit.

optimize_failed_cost is the median of the oracle's own Gauss-Newton costs of
the jobs, so both groups are non-empty (asserted on the oracle's numbers).
Also use_fine_scan_match = 0 (every job in the first group), and a call whose
maps differ in geometry (the pairs grown by different amounts, as in
test_device_backend_map_growth), which stays on the job-by-job path.
"""
import dataclasses

import numpy as np
import pytest

import test_backend as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drive():
    from roborts_csm import worlds
    w = worlds.make_world(400, 400, 0.05, seed=8)
    st = worlds.make_scan_stream(w, B.N_SCANS, seed=9)
    kept = B._kept_poses(st)
    return w, st, kept, B._jobs(st)


@pytest.fixture(scope="module")
def split_param(drive):
    """Gauss-Newton on, optimize_failed_cost between the jobs' oracle costs."""
    w, st, kept, jobs = drive
    _, probe = B._oracle_run(B._param("opt"), st, kept, jobs, st.true_poses[-1], None)
    costs = np.array([r.optimize_cost for r in probe])
    failed = float(np.median(costs))
    assert (costs > failed).any() and (costs <= failed).any(), costs  # both groups, on the oracle's numbers
    return dataclasses.replace(B._param("opt"), optimize_failed_cost=failed), costs


def _service(prm, st, kept):
    from roborts_csm.backend import ScanMatchService
    svc = ScanMatchService(prm)
    for k in range(B.N_SCANS):
        assert svc.AddRangeData(st.points_m[k], kept[k]) == k
    return svc


def _run(svc, st, jobs, cur, pub, use_fine=True):
    return svc.scan_match_jobs([st.points_m[q] for q, _, _ in jobs], [c for _, c, _ in jobs],
                               [p for _, _, p in jobs], cur, pub, use_fine)


def _same(want, got, what):
    for j, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a.pose, b.pose) and np.array_equal(a.cov, b.cov), (what, j)
        assert (a.score, a.map_penalty, a.optimize_cost) == (b.score, b.map_penalty, b.optimize_cost), (what, j)


def _launches(c, name):
    s = next((s for s in c.kernel_stats() if s["name"] == name), None)
    return None if s is None else s["launches"]


def test_both_groups_match_oracle(drive, split_param):
    w, st, kept, jobs = drive
    prm, costs = split_param
    cur = st.true_poses[-1]
    _, want = B._oracle_run(prm, st, kept, jobs, cur, B._pub_maps(w, st, kept))
    assert [r.optimize_cost for r in want] == costs.tolist()
    svc = _service(prm, st, kept)
    coarse = svc.matcher(svc.COARSE_MATCHER)
    assert coarse is not None and svc.matcher(svc.FINE_MATCHER) is not None
    coarse.set_profiling(True)
    pub = B._device_pub(w, st, kept)
    _same(want, _run(svc, st, jobs, cur, pub), "split")
    assert _launches(coarse, "optimize_solve_kernel") == 1  # every job's Gauss-Newton solve in one launch
    assert _launches(coarse, "optimize_cost_kernel") is None
    # a second call reuses the stacks' contexts
    _same(want, _run(svc, st, jobs, cur, pub), "again")
    assert _launches(coarse, "optimize_solve_kernel") == 2
    svc.close()


def test_coarse_only_all_in_first_group(drive, split_param):
    w, st, kept, jobs = drive
    prm, _ = split_param
    cur = st.true_poses[-1]
    _, want = B._oracle_run(prm, st, kept, jobs, cur, None, use_fine=False)
    svc = _service(prm, st, kept)
    coarse = svc.matcher(svc.COARSE_MATCHER)
    coarse.set_profiling(True)
    _same(want, _run(svc, st, jobs, cur, None, use_fine=False), "coarse only")
    assert _launches(coarse, "optimize_solve_kernel") == 1
    svc.close()


def test_mixed_geometry_stays_job_by_job(drive, split_param):
    """The current pose far from the queries: MapSizeCheck grows every pair by a
    different amount, so the call runs job by job (the host-loop Gauss-Newton)."""
    w, st, kept, jobs = drive
    prm, _ = split_param
    cur = st.true_poses[30] + np.array([1.8, -1.7, 0.0])
    _, want = B._oracle_run(prm, st, kept, jobs, cur, None)
    svc = _service(prm, st, kept)
    coarse = svc.matcher(svc.COARSE_MATCHER)
    coarse.set_profiling(True)
    _same(want, _run(svc, st, jobs, cur, None), "grown")
    assert len({svc.map(j, 1).state().size_x for j in range(len(jobs))}) > 1
    assert _launches(coarse, "optimize_solve_kernel") is None and _launches(coarse, "optimize_cost_kernel") >= len(jobs)
    svc.close()


def test_matcher_without_optimizer():
    """csm_backend_matcher: no coarse context when the Gauss-Newton matcher is off."""
    from roborts_csm.backend import ScanMatchService
    svc = ScanMatchService(B._param("sim"))
    assert svc.matcher(svc.COARSE_MATCHER) is None and svc.matcher(svc.FINE_MATCHER) is not None
    with pytest.raises(RuntimeError):
        svc.matcher(2)
    svc.close()
