"""The Gauss-Newton matcher's step rules (csrc/csm_optimize_step.hpp), without a
GPU. The host loop (csm_optimize_scan_match*) and the one-launch solve
(optimize_solve_kernel, csm_optimize_scan_match_batch_grids) both take their
steps from that header: the cost's normalisation, Eigen's 3x3 LDLT solve
restated, the NaN test, the two stop tests and UpdatePose with its clamps.

tests/cpp/optimize_step_check.cpp, compiled here against the header alone,
runs csm::opt::step and csm::opt::ldlt_solve3 over seeded cases; every result
is compared bit for bit (NaN payloads included) with the pure-Python
restatement (tests/opt_pyref.py) and the solve also with the oracle's
(O.ldlt_solve). The cases: random Gauss-Newton sums, an all-zero H, a zero
pivot, indefinite H, equal diagonal entries (the pivot tie), pivots at or
below DBL_MIN, NaN and infinite sums, steps beyond both clamps, and both stop
tests at iterations 0 and 1. The same program once more under ASan + UBSan,
stand-alone. Then the new entry points: exported, and CSM_ERR_INVALID_ARG for
a null context.
"""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import opt_pyref as R
import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "optimize_step_check.cpp")
INC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

K_SKIP, K_RUN, K_DONE, K_NAN = 0, 1, 2, 3
DBL_MIN = sys.float_info.min
DENORM = 5e-324


def _case(v, valid=100, last=0.0, est=(10.0, 20.0, 0.3), it=1, cdt=0.1, cmt=0.5, cells=6.25, ang=0.5):
    assert len(v) == 10
    return [float(x) for x in v] + [float(valid), float(last), *map(float, est), float(it), cdt, cmt, cells, ang]


def _sums(cost, H, b):
    """v = {cost, H00, H10, H11, H20, H21, H22, b0, b1, b2}"""
    return [cost, H[0][0], H[1][0], H[1][1], H[2][0], H[2][1], H[2][2], b[0], b[1], b[2]]


def _cases():
    rng = np.random.default_rng(20240607)
    out = []
    # what UpdateCost sums: J^T J and -J^T e over a few hundred points
    for k in range(1600):
        n = int(rng.integers(1, 400))
        J = rng.normal(size=(n, 3)) * rng.choice([1e-3, 1.0, 30.0])
        e = rng.uniform(0, 1, size=n)
        H, b, cost = J.T @ J, -(J.T @ e), float(e @ e)
        last = cost * 1000.0 / (1 + n) + rng.choice([-1.0, 0.0, 0.05, 0.2, 50.0])
        out.append(_case(_sums(cost, H, b), valid=n, last=last, est=rng.normal(size=3) * [100, 100, 3],
                         it=int(rng.integers(0, 10)), cdt=float(rng.choice([0.0, 0.1, 1.0])),
                         cmt=float(rng.choice([0.0, 0.5, 5.0])), cells=float(rng.choice([0.5, 6.25, 1e9])),
                         ang=float(rng.choice([0.05, 0.5, -0.5, 1e9]))))
    b = [1.0, 2.0, 3.0]
    Z = [[0.0] * 3 for _ in range(3)]
    out.append(_case(_sums(3.0, Z, b)))                                   # all-zero H: Eigen stops at k = 0
    out.append(_case(_sums(3.0, Z, b), valid=0, it=0))
    out.append(_case(_sums(3.0, np.diag([2.0, 0.0, 4.0]), [2.0, 5.0, 8.0])))   # a zero pivot
    out.append(_case(_sums(3.0, np.diag([0.0, 0.0, 4.0]), [2.0, 5.0, 8.0])))
    out.append(_case(_sums(3.0, [[1, 0, 0], [1, 1, 0], [1, 1, 1]], b)))        # rank 1: zero pivots after the first
    for _ in range(100):                                                    # indefinite H
        A = rng.normal(size=(3, 3))
        H = A + A.T
        H[int(rng.integers(0, 3))][int(rng.integers(0, 3))] *= -3.0
        H = np.tril(H) + np.tril(H, -1).T
        out.append(_case(_sums(2.0, H, rng.normal(size=3)), it=int(rng.integers(0, 3))))
    for _ in range(100):                                                    # the pivot tie: equal diagonal entries
        d = float(rng.choice([1.0, 3.0, -2.0, 1e-200]))
        lo = rng.normal(size=3) * abs(d) * 0.4
        H = [[d, lo[0], lo[1]], [lo[0], d, lo[2]], [lo[1], lo[2], d if rng.random() < 0.5 else d / 2]]
        out.append(_case(_sums(2.0, H, rng.normal(size=3))))
    for d in ([DBL_MIN, DBL_MIN, DBL_MIN], [DBL_MIN, DBL_MIN / 2, DENORM], [2 * DBL_MIN, DBL_MIN, DENORM],
              [1.0, DBL_MIN, DENORM], [1.0, np.nextafter(DBL_MIN, 1.0), DBL_MIN], [-DBL_MIN, DENORM, -DENORM],
              [DENORM, DENORM, DENORM], [1.0, 1.0, DBL_MIN]):               # pivots at or below DBL_MIN
        out.append(_case(_sums(1.0, np.diag(d), b)))
        out.append(_case(_sums(1.0, np.diag(d), [DBL_MIN, DENORM, 1e-300])))
    for _ in range(60):                                                     # ... reached by elimination
        A = rng.normal(size=(3, 3))
        H = (A @ A.T) * float(rng.choice([1e-308, 1e-310, 1e-320, 1e-154]))
        out.append(_case(_sums(1.0, H, rng.normal(size=3) * float(rng.choice([1.0, 1e-300])))))
    for bad in (math.nan, math.inf, -math.inf):                             # NaN and infinite sums
        for slot in range(10):
            A = rng.normal(size=(3, 3))
            v = _sums(2.0, A @ A.T, rng.normal(size=3))
            v[slot] = bad
            out.append(_case(v, it=slot % 2))
    out.append(_case([math.inf] * 10))
    out.append(_case([math.nan] * 10, it=0))
    for _ in range(60):                                                     # steps beyond both clamps, either sign
        H = np.diag(rng.uniform(1e-6, 1e-3, size=3))
        out.append(_case(_sums(1.0, H, rng.normal(size=3) * 100), it=0, cells=float(rng.choice([0.5, -0.5])),
                         ang=float(rng.choice([0.05, -0.05]))))
    out.append(_case(_sums(1.0, np.eye(3), [0.5, -0.5, 0.05]), it=0, cells=0.5, ang=0.05))  # exactly at the clamps
    I, c100 = np.eye(3), 101 / 1000.0 * 7.0                                 # normalized cost 7.0 at valid = 100
    for it in (0, 1):                                                       # both stop tests at iter 0 and 1
        out.append(_case(_sums(c100, I, b), last=7.05, it=it, cdt=0.1, cmt=0.0))    # decrease below the threshold
        out.append(_case(_sums(c100, I, b), last=7.2, it=it, cdt=0.1, cmt=0.0))     # ... above it: goes on
        out.append(_case(_sums(c100, I, b), last=5.0, it=it, cdt=0.1, cmt=0.0))     # the cost rose
        out.append(_case(_sums(c100, I, b), last=100.0, it=it, cdt=0.1, cmt=7.5))   # cost below cost_min_threshold
        out.append(_case(_sums(c100, I, b), last=100.0, it=it, cdt=0.1, cmt=7.0))   # ... equal: goes on
        out.append(_case(_sums(c100, I, b), last=7.0 + 0.1, it=it, cdt=0.1, cmt=0.0))
    while len(out) < 2000:
        out.append(_case(rng.normal(size=10) * float(rng.choice([1e-300, 1.0, 1e300])), it=int(rng.integers(0, 3))))
    return np.array(out, dtype=np.float64)


def _ref(c):
    """csm::opt::step and ldlt_solve3 on one case, from tests/opt_pyref.py."""
    v = [float(x) for x in c[:10]]
    valid, last, est, it = int(c[10]), float(c[11]), [float(x) for x in c[12:15]], int(c[15])
    cdt, cmt, cells, ang = (float(x) for x in c[16:20])
    cost = v[0] * (R.K_COST_POINT_SIZE / (1 + valid))
    H = [[v[1], v[2], v[4]], [v[2], v[3], v[5]], [v[4], v[5], v[6]]]
    det = R.ldlt_solve(H, v[7:10])
    if any(math.isnan(d) for d in det):
        state = K_NAN
    elif it > 0 and (last - cost < cdt or cost < cmt):
        state = K_DONE
    else:
        state = K_RUN
        est = [est[0] + R._limit(det[0], cells), est[1] + R._limit(det[1], cells), est[2] + R._limit(det[2], ang)]
    return [float(state), cost, *est, *det]


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", INC,
                        *extra, SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def expected(cases):
    return np.array([_ref(c) for c in cases], dtype=np.float64)


def _run(exe, cases, tmp_path, env=None):
    fin, fout = tmp_path / "cases.bin", tmp_path / "results.bin"
    cases.tofile(fin)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert f"optimize_step_check ok cases={len(cases)}" in r.stdout
    return np.fromfile(fout, dtype=np.float64).reshape(len(cases), 8)


def _same_bits(got, expected):
    bad = np.flatnonzero((got.view(np.uint64) != expected.view(np.uint64)).any(axis=1))
    assert bad.size == 0, (bad[:10], got[bad[:3]], expected[bad[:3]])


def test_cases_cover_every_branch(cases, expected):
    assert len(cases) >= 2000
    states = expected[:, 0]
    for it in (0, 1):
        at = cases[:, 15] == it
        assert (states[at] == K_RUN).any() and (states[at] == K_NAN).any()
    assert not (states[cases[:, 15] == 0] == K_DONE).any()  # no stop test before the second iteration
    assert (states[cases[:, 15] == 1] == K_DONE).any()
    moved = expected[:, 2:5] - cases[:, 12:15]
    run = states == K_RUN
    assert (np.abs(moved[run, 0]) == np.abs(cases[run, 18])).any()  # the distance clamp ...
    assert (np.abs(moved[run, 2]) == np.abs(cases[run, 19])).any()  # ... and the angle clamp took effect


@needs_gxx
def test_step_rules_match_restatement(tmp_path, cases, expected):
    exe, b = _build(tmp_path, "optimize_step_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    got = _run(exe, cases, tmp_path)
    _same_bits(got, expected)
    for c, g in zip(cases[::7], got[::7]):  # the solve also against the oracle's restatement
        H = [[c[1], c[2], c[4]], [c[2], c[3], c[5]], [c[4], c[5], c[6]]]
        assert np.array_equal(O.ldlt_solve(H, c[7:10]).view(np.uint64), g[5:8].view(np.uint64)), c


@needs_gxx
def test_step_rules_clean_under_asan_ubsan(tmp_path, cases, expected):
    exe, b = _build(tmp_path, "optimize_step_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    _same_bits(_run(exe, cases, tmp_path, env), expected)


NEW_SYMBOLS = ("csm_optimize_scan_match_batch_grids", "csm_scan_matchers_batch_grids_seeded", "csm_backend_matcher")


def test_new_entry_points_exported_and_reject_null():
    from roborts_csm import _abi
    lib = C.CDLL(_abi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    lib = _abi.load_library()
    null, n = C.c_void_p(None), None
    assert lib.csm_optimize_scan_match_batch_grids(null, 0, n, n, n, n, n, n, n) == _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_scan_matchers_batch_grids_seeded(null, 0, n, n, n, n, 0, 1, n, n, n, n) == _abi.CSM_ERR_INVALID_ARG
    out = C.c_void_p()
    assert lib.csm_backend_matcher(null, 0, C.byref(out)) == _abi.CSM_ERR_INVALID_ARG
