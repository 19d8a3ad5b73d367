"""Keys at the sizes where the device sort (csrc/csm_introsort.hpp) changes
path, shared by tests/test_sort_model.py (the Python models) and
tests/test_gpu_sort_paths.py (the kernel): 16/17 is the leaf threshold, 64/65
the boundary between sort_small and partition_lds, 256/257 kCoopMin
(partition_block); the killer sequences reach heap_sort at depth 0."""
import numpy as np

SIZES = (1, 2, 15, 16, 17, 18, 63, 64, 65, 66, 255, 256, 257, 258, 1023, 1024, 1025)


def killer(n):
    """Median-of-3 killer-ish sequences that drive introsort to its depth limit."""
    k = np.zeros(n)
    half = n // 2
    for i in range(half):
        k[2 * i] = i + 1
        k[2 * i + 1] = half + i + 1
    return k[::-1].copy()


def _rng(n):
    return np.random.default_rng(7000 + n)


FAMILIES = {
    "all_equal": lambda n: np.zeros(n),
    "two_values": lambda n: (np.arange(n) % 2).astype(float),
    "killer": killer,
    "int3": lambda n: _rng(n).integers(0, 3, size=n).astype(float),
    "int50": lambda n: _rng(n).integers(0, 50, size=n).astype(float),
    "uniform": lambda n: _rng(n).random(n),
    "ascending": lambda n: np.arange(n, dtype=float),
}
