"""csm_gate_options and csm_gate_stats (include/csm.h, csm_search_gated)
against their ctypes mirrors: sizes and field offsets from a small C program
gcc compiles against the header (the manner of tests/test_abi_layout_match.py),
the enum's numbers, and the argument rejections that need no context. No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc")
def test_gate_structs_layout_matches_header(tmp_path):
    from roborts_csm import _abi
    structs = [("csm_gate_options", _abi.CsmGateOptions), ("csm_gate_stats", _abi.CsmGateStats)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "csm_loop_closure.h"', "int main(void) {"]
    for cname, cls in structs:
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout_gate.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout_gate"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, key, val = line.split()
        got[(cname, key)] = int(val)
    for cname, cls in structs:
        assert got[(cname, "size")] == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)


def test_gate_path_values_and_abi_version():
    from roborts_csm import _abi
    txt = open(os.path.join(ROOT, "include", "csm.h")).read()
    for name, val in (("CSM_GATE_PRUNED", _abi.GATE_PRUNED), ("CSM_GATE_OVERFLOW", _abi.GATE_OVERFLOW),
                      ("CSM_GATE_UNPOOLED", _abi.GATE_UNPOOLED)):
        assert f"{name} = {val}," in txt or f"{name} = {val} " in txt, name
    assert _abi.load_library().csm_abi_version() == 1


def test_calls_without_a_handle_are_rejected():
    """A null context or handle is CSM_ERR_INVALID_ARG before anything else is
    read (everything else needs a device and lives in test_gpu_search_gated.py)."""
    from roborts_csm import _abi
    lib = _abi.load_library()
    n = C.c_int32(-7)
    p = _abi.CsmParam(1.0, 0.05, 0.2, 0.0349, 0.5, 100, 0, 0, 0)
    pts = (C.c_double * 4)(0.0, 0.0, 1.0, 1.0)
    ctr = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.csm_search_gated(None, pts, 2, C.byref(p), 1, None, ctr, 0.5, None, None, None, 0, C.byref(n),
                                None) == _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_loop_closure_match_gated(None, pts, 2, C.byref(p), ctr, 0.5, None, 0,
                                            C.byref(n)) == _abi.CSM_ERR_INVALID_ARG
    assert lib.csm_loop_closure_match_gated_full(None, pts, 2, C.byref(p), ctr, 0.5, None, 0, C.byref(n), None,
                                                 None) == _abi.CSM_ERR_INVALID_ARG
    assert n.value == -7
