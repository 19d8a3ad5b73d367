"""The gated search's host half (csrc/csm_search_gate.hpp: key -> score, the
pass test, ascending order, the capacity rule, and what follows an overflowed
list) against a Python restatement, through tests/cpp/search_gate_check.cpp: a
stand-alone host program over the header alone, run plain and once more under
ASan + UBSan. The arrays are what the device would leave per window: wkey (the
order-preserving image of the best score) and wflat (the lowest global flat of
the best candidates; INT64_MAX: the window does not pass). No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roborts-edu-slam_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "search_gate_check.cpp")
HIP_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # csm_internal.hpp: hip_runtime_api.h

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

I64_MAX = 2**63 - 1
DONE, REDESCEND, GROW, FALLBACK = 0, 1, 2, 3


# ---- the restatement ---------------------------------------------------------
def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def select_key(x):
    """csm_search_match.hpp: the key of x + 0.0; negatives flip every bit, the
    others the sign bit."""
    u = bits(x + 0.0)
    return (~u) & (2**64 - 1) if u >> 63 else u | (1 << 63)


def key_score_bits(key):
    return key & ~(1 << 63) if key >> 63 else (~key) & (2**64 - 1)


def gate_results(wkey, wflat, n_cand, capacity):
    rows = [(w, key_score_bits(k), f - w * n_cand) for w, (k, f) in enumerate(zip(wkey, wflat)) if f != I64_MAX]
    return len(rows), rows[:capacity]


def gate_after(descents, listed, capacity, fixed):
    if listed <= capacity:
        return DONE, capacity
    if descents <= 1:
        return REDESCEND, capacity
    if descents == 2 and not fixed and listed <= 2**26:
        return GROW, listed
    return FALLBACK, capacity


# ---- the program ---------------------------------------------------------------
def _build(tmp_path, name, extra):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                        "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-isystem", HIP_INC,
                        *extra, SRC, "-o", str(exe)], capture_output=True, text=True, timeout=300)
    return exe, b


def _run(exe, mode, text, env):
    r = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return r.stdout.split()


def _scores():
    """Scores of both signs, both zeros, subnormals, values above 1, ties."""
    rng = np.random.default_rng(31)
    s = [0.0, -0.0, 5e-324, -5e-324, 1.0, 1.1414, -0.45, 2.0 ** -1022, 0.5, 0.5]
    s += rng.uniform(-1.0, 1.5, 200).tolist()
    s += (rng.uniform(-1.0, 1.0, 50) * 1e-300).tolist()
    return s


def _cases():
    """(n_windows, n_cand, capacity, wkey, wflat), seeded: windows that never
    pass, none passing, all passing, capacity below the count, capacity 0."""
    rng = np.random.default_rng(32)
    sc = _scores()
    cases = []
    for k in range(60):
        nw = int(rng.integers(1, 40))
        n_cand = int(rng.integers(1, 5000))
        p_pass = (0.0, 1.0, 0.5, 0.1)[k % 4]
        wkey, wflat = [], []
        for w in range(nw):
            passes = rng.random() < p_pass
            # a key is raised even in a window whose list entries were lost; a
            # window nothing reached keeps the lowest key
            wkey.append(select_key(sc[int(rng.integers(len(sc)))]) if passes or rng.random() < 0.5 else 0)
            wflat.append(w * n_cand + int(rng.integers(n_cand)) if passes else I64_MAX)
        n_pass = sum(f != I64_MAX for f in wflat)
        capacity = (0, n_pass, max(n_pass - 1, 0), n_pass + 3, 1)[k % 5]
        cases.append((nw, n_cand, capacity, wkey, wflat))
    # the last candidate of the last window, a large n_cand (flat beyond 2^31)
    cases.append((3, 2**31 + 7, 3, [select_key(-0.25), 0, select_key(1.25)],
                  [2**31 + 6, I64_MAX, 3 * (2**31 + 7) - 1]))
    return cases


def _check(exe, env=None):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "search_gate_check ok" in r.stdout, (r.stdout + r.stderr)[-3000:]

    # key -> score: the bits of x + 0.0 come back, and the keys order as the scores
    sc = _scores()
    out = _run(exe, "--keys", "".join(f"{bits(x):016x}\n" for x in sc), env)
    assert len(out) == 2 * len(sc)
    for i, x in enumerate(sc):
        key, back = int(out[2 * i], 16), int(out[2 * i + 1], 16)
        assert key == select_key(x), x
        assert back == key_score_bits(key) == bits(x + 0.0), x
    assert select_key(-0.0) == select_key(0.0) and bits(from_bits(key_score_bits(select_key(-0.0)))) == 0
    ordered = sorted(sc)
    for a, b in zip(ordered, ordered[1:]):
        assert select_key(a) <= select_key(b) and (select_key(a) < select_key(b)) == (a < b), (a, b)

    # the pass test, ascending order and the capacity rule
    cases = _cases()
    text = ""
    for nw, n_cand, capacity, wkey, wflat in cases:
        text += f"{nw} {n_cand} {capacity}\n" + "".join(f"{k:016x} {f}\n" for k, f in zip(wkey, wflat))
    tok = _run(exe, "--results", text, env)
    pos = 0
    seen_short = seen_none = seen_all = 0
    for nw, n_cand, capacity, wkey, wflat in cases:
        n_pass, rows = gate_results(wkey, wflat, n_cand, capacity)
        assert int(tok[pos]) == n_pass
        pos += 1
        got = []
        for _ in range(min(n_pass, capacity)):
            got.append((int(tok[pos]), int(tok[pos + 1], 16), int(tok[pos + 2])))
            pos += 3
        assert got == rows
        assert [g[0] for g in got] == sorted(g[0] for g in got)
        seen_short += capacity < n_pass
        seen_none += n_pass == 0
        seen_all += n_pass == nw
    assert pos == len(tok)
    assert seen_short >= 5 and seen_none >= 5 and seen_all >= 5  # every kind was exercised

    # the decision after a descent, both modes
    table = []
    for descents in (1, 2, 3):
        for fixed in (0, 1):
            for listed, cap in ((0, 10240), (10240, 10240), (10241, 10240), (5, 4), (765000, 10240),
                                (2**26, 10240), (2**26 + 1, 10240), (2**26 + 1, 2**26 + 1), (65, 64)):
                table.append((descents, listed, cap, fixed))
    tok = _run(exe, "--after", "".join("%d %d %d %d\n" % t for t in table), env)
    assert len(tok) == 2 * len(table)
    for i, t in enumerate(table):
        assert (int(tok[2 * i]), int(tok[2 * i + 1])) == gate_after(*t), t
    # spelled out: the ladder of an automatic list, and a fixed one
    assert gate_after(1, 765000, 10240, False) == (REDESCEND, 10240)
    assert gate_after(2, 20000, 10240, False) == (GROW, 20000)
    assert gate_after(3, 20001, 20000, False) == (FALLBACK, 20000)
    assert gate_after(2, 65, 64, True) == (FALLBACK, 64)
    assert gate_after(2, 2**26 + 1, 10240, False) == (FALLBACK, 10240)

    first = [(0, 0), (0, 10240), (0, 10241), (0, 1 << 20), (4, 1 << 20), (64, 0), (-1, 500)]
    tok = _run(exe, "--first", "".join("%d %d\n" % t for t in first), env)
    assert [int(v) for v in tok] == [a if a > 0 else max(10240, h) for a, h in first]


def test_header_matches_restatement(tmp_path):
    exe, b = _build(tmp_path, "search_gate_check", [])
    assert b.returncode == 0, b.stderr[-3000:]
    _check(exe)


def test_header_clean_under_asan_ubsan(tmp_path):
    exe, b = _build(tmp_path, "search_gate_check_san",
                    ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    _check(exe, env)
