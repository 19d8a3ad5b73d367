"""The layouts' geometry (csrc/csm_grid_copies.hpp: gridi_pitch, strip_geom,
istrip_geom, bg_geom) against the scoring kernels' documented read patterns, as
pure host code: tests/cpp/grid_geom_check.cpp walks every size_x, size_y in
1..80, 399..403, 1999..2003 and 2047..2049 (93 per axis) and the GPU tests'
shapes (tests/grid_shapes.py), and checks that the furthest cell of each
pattern (a 16 x 16 box from an on-grid corner in gridi, the tiny kernel's
2 x 2 block, a box row piece in every strip copy with 16 rows below the grid,
the phase kernel's 8-cell strip reads at phase <= 3, the corner bits of the
maps of uniform boxes) lies inside the buffer the geometry sizes. The tight
pitch is named: gridi_pitch(sx) == sx + kGridiPadCols exactly when
sx % 4 == 1. The same program once more under ASan + UBSan, stand-alone.
No GPU."""
import os
import re
import shutil
import subprocess

import pytest

from grid_shapes import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "grid_geom_check.cpp")
INC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

PER_AXIS = 80 + 5 + 5 + 3
ARGS = [str(v) for shape in SHAPES for v in shape]


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", INC, *extra, SRC,
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _check(out):
    assert "grid_geom_check ok" in out, out[-3000:]
    lines = out.splitlines()
    f = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", lines[-2])}
    assert f["per_axis"] == PER_AXIS and f["sizes"] == PER_AXIS * PER_AXIS and f["failed"] == 0
    # the tight pitch: the sizes 1 (mod 4) of the axis (20 in 1..80, 401, 2001, 2049) and of the shapes
    assert f["tight_pitch"] == 23 + sum(sx % 4 == 1 for _, sx in SHAPES)
    # every padded column of every size was walked: the smallest grid has 17 of them in each strip layout
    # (five checks a column in the phase strips, four in the pair strips) and in the maps
    assert f["checks"] > (5 + 4 + 1) * 17 * f["sizes"]
    shapes = [{k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)} for ln in lines if ln.startswith("shape ")]
    assert [(s["size_y"], s["size_x"]) for s in shapes] == SHAPES
    for s in shapes:
        sx = s["size_x"]
        assert s["pitch"] == (sx + 15 + 3) // 4 * 4 and s["slack"] == (1 - sx) % 4
    by = {(s["size_y"], s["size_x"]): s for s in shapes}
    # what the shapes are for
    assert [by[k]["slack"] for k in ((29, 33), (33, 45), (40, 49), (12, 13), (1, 37), (37, 1), (1, 1))] == [0] * 7
    assert by[(31, 47)]["slack"] == 2 and by[(17, 16)]["slack"] == 1 and by[(5, 3)]["slack"] == 2


def test_shapes_have_the_residues_they_are_for():
    assert len(SHAPES) == len(set(SHAPES)) == 10
    assert {sx % 16 for _, sx in SHAPES} >= {1, 13, 15, 0, 3, 5}
    assert {sx % 8 for _, sx in SHAPES} >= {1, 5, 7, 0, 3}
    assert min(sx for _, sx in SHAPES) == 1 and min(sy for sy, _ in SHAPES) == 1


def test_read_patterns_stay_inside_the_buffers(tmp_path):
    exe, b = _build(tmp_path, "grid_geom_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe), *ARGS], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    _check(r.stdout)


def test_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "grid_geom_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), *ARGS], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    _check(r.stdout)
