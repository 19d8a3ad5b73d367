"""GPU: the finish kernel's sort (csrc/csm_introsort.hpp) against libstdc++'s
std::sort(greater) at the sizes where it changes path, for every key family
of tests/sort_path_cases.py: 16/17 is the leaf threshold, 64/65 the boundary
between sort_small and partition_lds, 256/257 kCoopMin (partition_block); the
killer sequences reach heap_sort at depth 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pyoracle as O  # noqa: E402
from sort_path_cases import FAMILIES, SIZES  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import roborts_csm
    c = roborts_csm.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_device_sort_at_path_boundaries(ctx, family):
    for n in SIZES:
        k = FAMILIES[family](n)
        assert np.array_equal(ctx.sort_order(k), O.std_sort_order(k)), n
