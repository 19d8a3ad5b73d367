"""Ownership of the host side's buffer type (csrc/csm_resources.hpp) as a pure
host check: tests/cpp/resources_check.cpp, compiled against the header alone
with a counting malloc / free policy in place of the HIP ones, checks that
ensure below capacity allocates nothing, that ensure above it asks for exactly
grow_bytes(bytes, cap) and ensure_exact for exactly the bytes, that a failed
allocation leaves {nullptr, 0}, and that move construction, move assignment,
std::swap and the eviction pattern (an empty value assigned over a slot that
holds buffers; a struct of buffers and scalars standing in for GridState,
swapped whole) end with every allocation freed exactly once and none live.
A move assignment that does not free its target fails it (tried: moves(),
eviction() and the final balance report it). submit_sequence() runs
csm_scan_matchers_submit's exchanges on a stand-in for ScanBatch: a loaded
batch whose job reads its offsets through a pointer, a queued batch taken (one
whole swap), the parked batch borrowed back and returned, the next batch
queued into the slot that holds the parked one, and that one taken; the
pointer addresses the first batch's offsets, unchanged, until its slot is
queued into, every field travels with its batch, the cache flag is false after
every swap and each allocation is freed once. The same program once more under
ASan + UBSan, stand-alone. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "resources_check.cpp")
INC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", INC, *extra, SRC,
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out):
    assert "resources_check ok" in out, out[-2000:]
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out.splitlines()[-2])}
    assert f["failed"] == 0 and f["live"] == 0 and f["bad_frees"] == 0
    # 7 in sizes(), 1 in failures(), 3 in moves(), 16 in eviction(), 3 in submit_sequence()
    assert f["allocs"] == f["frees"] == 30


def test_buffer_owns_what_it_allocates(tmp_path):
    exe, b = _build(tmp_path, "resources_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout)


def test_buffer_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "resources_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout)
