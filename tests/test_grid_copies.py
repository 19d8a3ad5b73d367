"""The grid's derived copies (csrc/csm_grid_copies.hpp) as pure host code:
tests/cpp/grid_copies_check.cpp, compiled against that header (and the buffer
template of csm_resources.hpp without HIP), evaluates every rule on both sides
of its thresholds (palette sizes 0, 1, 16, 17 and 257; strips of 2^24 - 1 and
2^24 bytes; maps of 2^28 - 1 and 2^28 bytes; 65535 and 65536 grids; a share
just under and at kBgMinShare; CSM_BG_RUNS 0 to 3; the phase kernel's wish
for the palette over all eight combinations of its inputs), the key's test
(stale after a generation step with the same grid and after another grid at
the same generation, current otherwise), and moves and swaps of the record
over a counting allocator: every buffer freed once, keys and outcomes
travelling with the buffers. The same program once more under ASan + UBSan,
stand-alone. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "grid_copies_check.cpp")
INC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I", INC,
                        *extra, SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out):
    assert "grid_copies_check ok" in out, out[-2000:]
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[-2])}
    # three records of eight buffers each, every one freed exactly once
    assert f["allocs"] == 24 and f["frees"] == 24 and f["bad_frees"] == 0 and f["live"] == 0
    assert f["failed"] == 0 and f["checks"] >= 130


def test_header_includes_neither_hip_nor_the_context():
    text = open(os.path.join(INC, "csm_grid_copies.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text) == ["cstdint"]


def test_rules_key_and_record(tmp_path):
    exe, b = _build(tmp_path, "grid_copies_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout)


def test_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "grid_copies_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout)
