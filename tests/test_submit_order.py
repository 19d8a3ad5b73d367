"""The order csm_scan_matchers_submit takes its steps in
(csrc/csm_submit_order.hpp) as a pure host function:
tests/cpp/submit_order_check.cpp, compiled against the header alone, lists the
steps for every combination of 1 or 2 parts of the new batch, none, 1 or 2
parts of the pending batch, 1 or 3 levels and deferral on or off, and checks
that every hand-off follows the launch of the level it completes, that the
pending batch's last launch precedes its completion and both are inside the
call, that a single part's hand-off precedes the pending batch's completion,
and that no step appears twice. It then hands its own checker two wrong orders
(the completion back in front of the single part's hand-off; a hand-off in
front of its part's begin), which must be refused, and checks the rule for the
number of parts (submit_parts). The same program once more under ASan + UBSan,
stand-alone. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "submit_order_check.cpp")
INC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", INC, *extra, SRC,
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out):
    assert "submit_order_check ok" in out and "FAIL" not in out, out[-3000:]
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[-2])}
    # 2 x 3 x 2 x 2 combinations; the single-part orders with a batch pending
    # and a hand-off (2 x 2) refuse the finish-first mutant, every 3-level
    # order (12) the hand-off-first one
    assert f == {"combos": 24, "refused_finish_first": 4, "refused_handoff_first": 12, "rules": 36}, f
    lines = out.splitlines()
    assert "parts=1 pending=1 levels=3 defer=1: begin(p0) prior_last handoff(l0,p0) prior_finish " in lines
    assert "parts=1 pending=2 levels=3 defer=0: begin(p0) prior_last handoff(l0,p0) prior_finish handoff(l1,p0) " in lines
    assert ("parts=2 pending=1 levels=3 defer=1: begin(p0) prior_last begin(p1) prior_finish handoff(l0,p0) "
            "handoff(l0,p1) handoff(l1,p0) ") in lines
    assert "parts=1 pending=0 levels=1 defer=1: begin(p0) " in lines


def test_submit_order(tmp_path):
    exe, b = _build(tmp_path, "submit_order_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout)


def test_submit_order_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "submit_order_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout)
