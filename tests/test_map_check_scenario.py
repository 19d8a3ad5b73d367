"""A condition on the batched map check's GPU test, checked with the Python
restatement alone (tests/map_pyref.py): on the count_lines PubMap of
map_scenarios (CountCell, grown to 160 x 239, rays up to 100 cells), the 24
poses that tests/test_gpu_map_check_batch.py compares must not be trivial.
At (50, 2.5, 0.015) their counts include a 0, a 1 and a value >= 10; at
(100, 1.0, 0.05) at least one pose reaches the coefficient's floor of 0.1.
With default_rng(5) the counts at (50, 2.5, 0.015) were
0, 1, 1, 0, 23, 15, 6, 17, 6, 28, ... and 13 of 24 poses reached the floor at
(100, 1.0, 0.05). No GPU."""
import map_check_cases as K
import map_scenarios as S
from map_engines import PyrefEngine


def test_checked_poses_are_not_trivial():
    scans_m, scans_c, poses = K.scans()
    sc = S.scenarios()["count_lines"]
    m, pens = S.run(PyrefEngine, sc, scans_c, poses)
    st = m.state()
    assert (st["size_x"], st["size_y"]) == (160, 239)
    check, idx = K.check_poses(poses)
    assert check.shape == (24, 3)
    # the scenario's own penalty ops are the first four poses' answers
    assert pens[0] == m.penalty(scans_c[2], check[2], 50, 2.5, 0.015, False)
    assert pens[1] == m.penalty(scans_c[3], check[3], 100, 1.0, 0.05, False)

    cpn, tol, gain = K.PARAMS[0]
    coeffs = [m.penalty(scans_c[i], p, cpn, tol, gain, False) for p, i in zip(check, idx)]
    assert all(c > 0.1 for c in coeffs if c != 0.0)  # above the floor: the count can be read back
    counts = [-1 if c == 0.0 else K.count_of(c, gain, 2 * cpn) for c in coeffs]
    print("counts at", K.PARAMS[0], counts)
    assert 0 in counts and 1 in counts and max(counts) >= 10, counts

    cpn, tol, gain = K.PARAMS[1]
    floored = sum(m.penalty(scans_c[i], p, cpn, tol, gain, False) == 0.1 for p, i in zip(check, idx))
    print("poses at the floor at", K.PARAMS[1], floored)
    assert floored >= 1, floored
