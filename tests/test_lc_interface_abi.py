"""csm_loop_closure_interface_param and csm_loop_closure_interface_result
(include/csm_loop_closure.h, csm_loop_closure_scan_match) against their ctypes
mirrors: sizes and field offsets from a small C program gcc compiles against
the header (the manner of tests/test_search_gated_abi.py), the symbols the
library exports, and the argument rejections that need no handle. No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc")
def test_interface_structs_layout_matches_header(tmp_path):
    from roborts_csm import _abi
    structs = [("csm_loop_closure_interface_param", _abi.CsmLoopClosureInterfaceParam),
               ("csm_loop_closure_interface_result", _abi.CsmLoopClosureInterfaceResult)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "csm_loop_closure.h"', "int main(void) {"]
    for cname, cls in structs:
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout_lc_interface.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout_lc_interface"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, key, val = line.split()
        got[(cname, key)] = int(val)
    for cname, cls in structs:
        assert got[(cname, "size")] == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    # the nested structs are the ones the gated calls fill
    assert dict(_abi.CsmLoopClosureInterfaceResult._fields_)["wide"] is _abi.CsmLoopClosureResult
    assert dict(_abi.CsmLoopClosureInterfaceResult._fields_)["wide_match"] is _abi.CsmMatchResult
    assert dict(_abi.CsmLoopClosureInterfaceParam._fields_)["check"] is _abi.CsmMapCheckParam


def test_symbols_exist_and_are_bound():
    from roborts_csm import _abi
    lib = _abi.load_library()
    for name in ("csm_loop_closure_scan_match", "csm_loop_closure_matcher"):
        assert name in _abi.EXPORTED, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert lib.csm_abi_version() == 1
    # the header's gate through the library: 3 T - 2 lowered by 8 ulps of 1, T itself with one level
    assert "csm_loop_closure_wide_gate" in _abi.EXPORTED and lib.csm_loop_closure_wide_gate.restype is C.c_double
    for T in (0.0, 0.6, 0.75, 1.0 / 3):
        assert lib.csm_loop_closure_wide_gate(T, 3) == 3.0 * T - 2.0 - 8.0 * 2.0 ** -52
        assert lib.csm_loop_closure_wide_gate(T, 1) == T


def test_calls_without_a_handle_are_rejected():
    from roborts_csm import _abi
    lib = _abi.load_library()
    prm = _abi.CsmLoopClosureInterfaceParam()
    pose = (C.c_double * 3)(0.0, 0.0, 0.0)
    n = C.c_int32(-7)
    assert lib.csm_loop_closure_scan_match(None, None, 0, C.byref(prm), pose, None, None, 0,
                                           C.byref(n)) == _abi.CSM_ERR_INVALID_ARG
    h = C.c_void_p()
    assert lib.csm_loop_closure_matcher(None, 0, C.byref(h)) == _abi.CSM_ERR_INVALID_ARG
    assert n.value == -7 and not h.value
