"""csm_occupancy_grid_info (include/csm_gridmap.h) against its ctypes mirror
(roborts_csm._abi.CsmOccupancyGridInfo): size and every field's offset from a
small C program gcc compiles against the header, as tests/test_abi_layout.py
does for the other structs; and the map publisher's entry points are bound
with the pointer types the headers declare. No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc")
def test_occupancy_grid_info_layout(tmp_path):
    from roborts_csm import _abi
    cls = _abi.CsmOccupancyGridInfo
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "csm_gridmap.h"', '#include "csm_frontend.h"',
             "int main(void) {", '  printf("size %zu\\n", sizeof(csm_occupancy_grid_info));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(csm_occupancy_grid_info, {fname}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) == 3 * 8 + 6 * 4
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def test_publisher_entry_points_are_bound():
    from roborts_csm import _abi
    lib = _abi.load_library()
    info_p = C.POINTER(_abi.CsmOccupancyGridInfo)
    assert lib.csm_gridmap_states.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    for name in ("csm_gridmap_occupancy_grid_info", "csm_gridmap_occupancy_grid_begin"):
        assert getattr(lib, name).argtypes == [C.c_void_p, C.c_int32, info_p]
    assert lib.csm_gridmap_occupancy_grid.argtypes == [C.c_void_p, C.c_int32, info_p, C.c_void_p, C.c_int64]
    assert lib.csm_frontend_publish_map.argtypes == [C.c_void_p, C.c_int32, info_p, C.POINTER(C.c_void_p)]
    # null handles are refused before anything touches a device
    info = _abi.CsmOccupancyGridInfo()
    p = C.c_void_p()
    assert lib.csm_gridmap_states(None, 0, 0, 1, 1, None) == _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_gridmap_occupancy_grid_begin(None, 0, C.byref(info)) == _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_gridmap_occupancy_grid_end(None, C.byref(p)) == _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_frontend_publish_map(None, -1, C.byref(info), C.byref(p)) == _abi.CSM_ERR_INVALID_ARG
