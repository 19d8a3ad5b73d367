"""Python restatement of the step from a LaserScan's ranges to the matcher's
scan endpoints: SlamNode::BuildRangeDataContainer (roborts_slam_node.cpp:290-311)
followed by RangeDataContainer::CreateFrom (sensor_data_manager.h:99-115), with
LaserRangeFinder::set_range_threshold_scale's threshold (:43-49).

Independent of the library: Python floats (binary64, one rounding per
operation) for the running beam angle and the products, tests/libm.sincos for
the (cos, sin) pair GCC makes of :303, and the message's float32 fields widened
with float(). It pins csm_ranges_to_points (the C++ restatement), which in
turn pins the device path (tests/test_gpu_ranges.py).

Also the hand-made scans both test files use (edge_batch).
"""
from dataclasses import dataclass

import numpy as np

from libm import sincos


@dataclass(frozen=True)
class Laser:
    """A LaserScan's float32 fields and ParamConfig's range_threshold_scale."""

    angle_min: np.float32
    angle_increment: np.float32
    range_min: np.float32
    range_max: np.float32
    range_threshold_scale: float
    n_beams: int

    def to_c(self):
        from roborts_csm._abi import CsmLaser
        return CsmLaser(float(self.angle_min), float(self.angle_increment), float(self.range_min),
                        float(self.range_max), float(self.range_threshold_scale), int(self.n_beams), 0)

    def with_beams(self, n: int) -> "Laser":
        return Laser(self.angle_min, self.angle_increment, self.range_min, self.range_max,
                     self.range_threshold_scale, n)


def hokuyo(n_beams: int = 1081) -> Laser:
    """worlds/willow-pr2-5cm.world:7-13 (270.25 deg, 0.1-10 m), threshold scale 0.95
    (config/simulatin_param.yaml:36); its threshold is no float32."""
    fov = np.radians(270.25)
    return Laser(np.float32(-fov / 2), np.float32(fov / 1080), np.float32(0.1), np.float32(10.0), 0.95, n_beams)


def exact_threshold(n_beams: int = 1081) -> Laser:
    """0.5 + 0.5 * (8.5 - 0.5) = 4.5: the threshold is itself a float32."""
    return Laser(np.float32(-2.0), np.float32(0.00390625), np.float32(0.5), np.float32(8.5), 0.5, n_beams)


def backwards(n_beams: int = 1081) -> Laser:
    """A sensor mounted upside down: beams sweep from +angle downwards."""
    fov = np.radians(240.0)
    return Laser(np.float32(fov / 2), np.float32(-fov / 682), np.float32(0.06), np.float32(5.6), 0.9, n_beams)


def threshold(L: Laser) -> float:
    lo, hi = float(L.range_min), float(L.range_max)  # sensor_data_manager.h:47
    return lo + L.range_threshold_scale * (hi - lo)


def ranges_to_points(L: Laser, ranges, factor: float):
    """-> (points [N, 2] float64, offsets [n_scans + 1] int64)."""
    r = np.asarray(ranges)
    assert r.dtype == np.float32
    r = r.reshape(-1, L.n_beams)
    thr, lo = threshold(L), float(L.range_min)
    a, inc = float(L.angle_min), float(L.angle_increment)
    cs = []
    for _ in range(L.n_beams):  # roborts_slam_node.cpp:294,306
        cs.append(sincos(a))
        a = a + inc
    factor = float(factor)
    pts, off = [], [0]
    for scan in r:
        for i in range(L.n_beams):
            d = float(scan[i])
            if d > lo and d < thr:  # :300
                c, s = cs[i]
                x, y = c * d, s * d  # :303
                pts.append((x * factor, y * factor))  # sensor_data_manager.h:111
        off.append(len(pts))
    return np.array(pts, dtype=np.float64).reshape(-1, 2), np.array(off, dtype=np.int64)


def edge_values(L: Laser) -> np.ndarray:
    """The float32 ranges at which the keep test can go wrong."""
    f = np.float32
    lo, hi = L.range_min, L.range_max
    t = threshold(L)
    t32 = f(t)  # the float32 nearest the threshold (the threshold itself where it is one)
    inf = f(np.inf)
    return np.array([
        f(np.nan), inf, -inf, f(0.0), f(-0.0), f(-1.0), -lo,
        lo, np.nextafter(lo, inf), np.nextafter(lo, -inf),
        t32, np.nextafter(t32, -inf), np.nextafter(t32, inf),
        hi, np.nextafter(hi, -inf), f(np.finfo(np.float32).tiny), f(np.finfo(np.float32).max),
        f(1e-45),  # the smallest denormal
    ], dtype=np.float32)


def edge_batch(L: Laser, seed: int = 0) -> np.ndarray:
    """Scans [S, n_beams] of edge values and ordinary ranges in a seeded
    shuffle (every edge value appears at least twice), with scans whose every
    beam is dropped first, in the middle and last."""
    rng = np.random.default_rng(seed)
    ev = edge_values(L)
    n = L.n_beams
    k = max(4, -(-3 * ev.size // n))
    k += k % 2
    flat = rng.uniform(float(L.range_min), threshold(L), size=k * n).astype(np.float32)
    where = rng.permutation(k * n)[:2 * ev.size] if k * n >= 2 * ev.size else np.arange(k * n)
    flat[where] = np.resize(ev, where.size)
    body = flat.reshape(k, n)
    dead = np.resize(np.array([np.nan, np.inf, 0.0, -1.0, float(L.range_min), float(L.range_max)], dtype=np.float32),
                     n).reshape(1, n)
    return np.ascontiguousarray(np.concatenate([dead, body[:k // 2], dead, dead, body[k // 2:], dead]))
