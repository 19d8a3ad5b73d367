"""csm_match_options and csm_match_result (include/csm.h, csm_search_match /
csm_loop_closure_match_full) against their ctypes mirrors: every struct's size
and every field's offset, from a small C program gcc compiles against the
header, in the manner of tests/test_abi_layout.py. No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "roborts-edu-slam_amd"))


def _structs():
    from roborts_csm import _abi
    return [("csm_match_options", _abi.CsmMatchOptions), ("csm_match_result", _abi.CsmMatchResult)]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc")
def test_match_structs_layout_matches_header(tmp_path):
    structs = _structs()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "csm_loop_closure.h"', "int main(void) {"]
    for cname, cls in structs:
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout_match.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout_match"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, key, val = line.split()
        got[(cname, key)] = int(val)
    for cname, cls in structs:
        assert got[(cname, "size")] == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)


def test_match_path_values():
    """The path numbers the header's enum and the binding agree on."""
    from roborts_csm import _abi
    txt = open(os.path.join(ROOT, "include", "csm.h")).read()
    for name, val in (("CSM_MATCH_PRUNED", _abi.MATCH_PRUNED), ("CSM_MATCH_TIE", _abi.MATCH_TIE),
                      ("CSM_MATCH_OVERFLOW", _abi.MATCH_OVERFLOW), ("CSM_MATCH_UNPOOLED", _abi.MATCH_UNPOOLED),
                      ("CSM_MATCH_LOW_RESPONSE", _abi.MATCH_LOW_RESPONSE),
                      ("CSM_MATCH_NO_RESPONSE", _abi.MATCH_NO_RESPONSE)):
        assert f"{name} = {val}," in txt or f"{name} = {val} " in txt, name
