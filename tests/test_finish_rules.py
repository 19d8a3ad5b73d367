"""The finish's decision rules (csrc/csm_finish_rules.hpp) as pure host
functions: tests/cpp/finish_rules_check.cpp, compiled against the header and
csm_internal.hpp alone, drives them serially over one window the way the fast
finish does (max, level counts, selected set, ranks and ties, find_best,
near-best set, ranks and ties) with both cap sets (128, 512) and all four
skip_lists values, over seeded windows of the three sim shapes and one
candidate: distinct scores, a planted duplicate at rank 0, 19, 20, 21 and at
either edge of FindBest's band, one at ranks 19, 20, 21 of the near-best set,
3-5 value palettes, hundreds of scores inside level 0, a NaN, best below and above 0.6. A window the rules do not flag gives
the FinishOut of a plain std::sort finish bit for bit; a window is flagged
exactly when a reason the program finds on its own holds; level_of equals
eight explicit comparisons and select_level a direct count. The same program
once more under ASan + UBSan, stand-alone. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "finish_rules_check.cpp")
INC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # csm_internal.hpp: hip_runtime_api.h

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-D__HIP_PLATFORM_AMD__", "-I", INC, "-isystem", HIP_INC, *extra, SRC, "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out):
    assert "finish_rules_check ok" in out, out[-2000:]
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[-2])}
    assert f["windows"] >= 400 and f["runs"] == 8 * f["windows"]
    # every class occurred: flagged for each reason, unflagged for each skip_lists
    for why in ("nan", "set_cap", "tie_band", "tie_rank", "near_cap", "tie_ang"):
        assert f[why] > 0, (why, f)
    for skip in range(4):
        assert f[f"unflagged_skip{skip}"] > 0, (skip, f)
    # the tie test includes rank 20, the list stores ranks below 20
    assert f["plant20_flagged"] > 0 and f["plant21_unflagged"] > 0, f
    assert f["near20_flagged"] > 0 and f["near21_unflagged"] > 0, f  # likewise inside the near-best set
    # the equality check is not starved
    assert 2 * f["flagged"] <= f["runs"] and f["flagged_pct"] <= 50, f
    assert f["level_checks"] >= 2000 * 30 and f["select_checks"] > 0


def test_rules_equal_a_plain_sort_finish(tmp_path):
    exe, b = _build(tmp_path, "finish_rules_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout)
    # other seeds: the properties hold, whatever the windows drawn
    for seed in ("1", "77"):
        r = subprocess.run([str(exe), "200", seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "finish_rules_check ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_rules_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "finish_rules_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), "400"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout)
