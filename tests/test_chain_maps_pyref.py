"""CPU: the splat rule of csrc/csm_chain_maps.hip, restated in NumPy
(tests/chain_maps_ref.py), against the oracle on the small cases the GPU test
uses; that those cases reach every branch on purpose; and that each way of
breaking the rule shows against the oracle on them. The GPU test compares the
device's stacks with the same oracle stacks: a kernel with one of these
mistakes fails there on the cases counted here. No GPU."""
import numpy as np
import pytest

import chain_maps_ref as R

CASES = [(b, n) for b in R.BLURS for n in (1, 5)]


@pytest.fixture(scope="module")
def small():
    scans, poses = R.small_scans()
    stacks = {}
    for blur, n in CASES:
        dev, off = R.BLURS[blur]
        stacks[(blur, n)] = R.oracle_stack(scans, poses, R.CHAINS1 if n == 1 else R.CHAINS5, dev, off)
    return scans, poses, stacks


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("blur,n", CASES)
def test_restated_rule_equals_oracle(small, blur, n):
    scans, poses, stacks = small
    dev, off = R.BLURS[blur]
    chains = R.CHAINS1 if n == 1 else R.CHAINS5
    st = {}
    assert _same(R.pyref_stack(scans, poses, chains, dev, off, stats=st), stacks[(blur, n)])
    # the cases reach what they were built for: both sides of the band's edge
    # on all four sides, the start cell, an exact .5, NaN and infinity
    for k in ("edge_x_lo", "edge_x_hi", "edge_y_lo", "edge_y_hi", "in_x_lo", "in_x_hi", "in_y_lo", "in_y_hi", "start",
              "half", "nonfinite"):
        assert st[k] >= 1, (k, st)
    moved = R.moved_poses(poses)
    assert _same(R.pyref_stack(scans, moved, chains, dev, off), R.oracle_stack(scans, moved, chains, dev, off))
    assert not _same(R.oracle_stack(scans, moved, chains, dev, off), stacks[(blur, n)])  # the move shows


def test_untouched_cells_and_empty_chain(small):
    _, _, stacks = small
    s = stacks[("hk2", 5)]
    assert np.all(s[0] == np.float32(R.DEFAULT))  # the empty chain
    assert np.all(s[1:].max(axis=(1, 2)) == np.float32(1.0))
    assert all(np.any(g == np.float32(R.DEFAULT)) for g in s)


@pytest.mark.parametrize("mutate", ["band_hk", "no_centre", "no_le1", "no_start_skip"])
def test_each_broken_rule_shows_on_the_small_cases(small, mutate):
    scans, poses, stacks = small
    caught = []
    for blur, n in CASES:
        dev, off = R.BLURS[blur]
        got = R.pyref_stack(scans, poses, R.CHAINS1 if n == 1 else R.CHAINS5, dev, off, mutate=mutate)
        if not _same(got, stacks[(blur, n)]):
            caught.append((blur, n))
    print(f"{mutate}: {len(caught)} of {len(CASES)} small cases differ from the oracle: {caught}")
    assert caught
