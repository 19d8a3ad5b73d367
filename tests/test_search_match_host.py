"""The finish over a collected list (csrc/csm_search_match.cpp: list_finish,
finish_complete), host only: tests/cpp/search_match_check.cpp, compiled with
that one source file, compares it with a plain std::sort finish over full
score arrays -- random windows (5 x 21^2, 3 x 33^2, 9 x 13^2) with distinct
scores for COARSE / FINE / SUPER bit for bit; planted ties that must give "a
tie matters" (inside FindBest's band, at ranks 19 and 20 of the positional
list, among the near-best angular candidates) and ones that must not (far
below rank 20, outside the near-best set); the early returns (best < 1e-6, a
norm of 1e-6, an empty near-best set). Once plain, once under ASan + UBSan,
stand-alone. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "cpp", "search_match_check.cpp"), os.path.join(CSRC, "csm_search_match.cpp")]
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # csm_internal.hpp: hip_runtime_api.h

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-isystem", HIP_INC,
                        *extra, *SRCS, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out, trials):
    assert "search_match_check ok" in out, out[-2000:]
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[-2])}
    assert f["windows"] == trials and f["equal"] == trials
    for t in ("coarse", "fine", "super"):
        assert f[t] >= trials // 3 - 1, f
    # every planted class occurred
    for k in ("tie_band", "tie_pos19", "tie_pos20", "tie_ang", "tie_harmless", "rank20_exercised"):
        assert f[k] >= trials // 10, (k, f)
    assert f["early_best"] == 3 and f["early_norm"] == 3 and f["early_near_empty"] == 3, f


def test_list_finish_equals_a_plain_sort_finish(tmp_path):
    exe, b = _build(tmp_path, "search_match_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), "180"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout, 180)
    for seed in ("1", "77"):  # other seeds: the properties hold, whatever the windows drawn
        r = subprocess.run([str(exe), "90", seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "search_match_check ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_list_finish_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "search_match_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "180"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout, 180)
