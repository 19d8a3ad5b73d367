"""The reduced finish (csrc/csm_search_match.hpp: reduced_finish), host only:
tests/cpp/list_reduce_check.cpp, compiled with csm_search_match.cpp alone,
feeds list_finish the subset R = A u B that two selections cut out of the
collected set H (the selection restated on the host: a sort plus the
definition) and compares tie_matters, FinishOut, CovSums, response, pose and
cov bit for bit with list_finish over all of H -- on random windows
(5 x 21^2, 3 x 33^2, 9 x 13^2; COARSE / FINE / SUPER) and the planted classes
the check's header lists, each of which must show up in at least a tenth of
the trials. Once plain, once under ASan + UBSan, stand-alone; and the
mutation K = 20, which must fail on a tie at ranks 20 / 21. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "cpp", "list_reduce_check.cpp"), os.path.join(CSRC, "csm_search_match.cpp")]
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # csm_internal.hpp: hip_runtime_api.h
CLASSES = ("tie2021", "tie2122", "tie_across", "band_long", "near_lt", "near_eq", "near_gt_tie", "a_below_b",
           "small_h", "dup_ab", "signed_zero")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-isystem", HIP_INC,
                        *extra, *SRCS, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out, trials):
    assert "list_reduce_check ok" in out, out[-2000:]
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[-2])}
    assert f["trials"] == trials and f["equal"] + f["ties"] == f["variants"] and f["variants"] >= 8 * trials, f
    assert f["equal"] >= 4 * trials and f["ties"] >= trials // 2 and f["overflow"] >= trials, f
    for t in ("coarse", "fine", "super"):
        assert f[t] >= trials // 3 - 1, f
    for k in CLASSES:  # every planted class occurred
        assert f[k] >= (trials + 9) // 10, (k, f)


def test_reduced_finish_equals_the_whole_list_finish(tmp_path):
    exe, b = _build(tmp_path, "list_reduce_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), "180"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout, 180)
    for seed in ("1", "77"):  # other seeds: the properties hold, whatever the windows drawn
        r = subprocess.run([str(exe), "90", seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        _check(r.stdout, 90)


def test_reduced_finish_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "list_reduce_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "180"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout, 180)


def test_mutation_k20_misses_the_tie_at_ranks_20_21(tmp_path):
    """K = 20 selects ranks 0..19: the run that starts at rank 20 is not in A,
    so a tie at ranks 20 / 21 that matters on H goes unseen on R. (K = 21 does
    pass: the selection is closed under ties with its K-th, so rank 20 brings
    a tied rank 21 along; K = 22 is the margin the header's argument states.)"""
    exe, b = _build(tmp_path, "list_reduce_check_k20", ["-DCSM_REDUCE_K=20"])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), "180"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "variant tie2021: a tie that matters on H is missed on R" in r.stdout, r.stdout[-2000:]
