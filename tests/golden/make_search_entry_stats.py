"""Record tests/golden/search_entry_stats.json: the csm_kernel_stats rows that
tests/test_gpu_search_entry.py's four profiled calls leave (launches,
algorithmic bytes, scorings; no times), from the library CSM_LIB names -- the
build of the commit before the search entry points moved into their own unit.
Needs an MI355X.

  CSM_LIB=<that commit's libroborts_csm.so> python3 tests/golden/make_search_entry_stats.py record OUT.json
  python3 tests/golden/make_search_entry_stats.py merge A.json B.json

record: the rows of one run, with the library's build digest. merge: two
recordings -> the golden file; a field whose value differs between them is
left out of its row and named under "unstable".
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "roborts-edu-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def record(out):
    import roborts_csm
    import test_gpu_search_entry as T
    rows = T.profiled_rows()
    with open(out, "w") as fh:
        json.dump({"library": roborts_csm.build_digest(), "rows": rows}, fh, indent=1)
    print(out, len(rows), "rows")


def merge(a, b):
    with open(a) as fa, open(b) as fb:
        A, B = json.load(fa), json.load(fb)
    assert A["library"] == B["library"] and sorted(A["rows"]) == sorted(B["rows"])
    rows, unstable = {}, []
    for name, ra in A["rows"].items():
        rows[name] = {f: v for f, v in ra.items() if B["rows"][name][f] == v}
        unstable += [f"{name}.{f}" for f in ra if f not in rows[name]]
    with open(os.path.join(HERE, "search_entry_stats.json"), "w") as fh:
        json.dump({"library": A["library"], "unstable": unstable, "rows": rows}, fh, indent=1)
        fh.write("\n")
    print(len(rows), "rows; unstable:", unstable)


if __name__ == "__main__":
    {"record": record, "merge": merge}[sys.argv[1]](*sys.argv[2:])
