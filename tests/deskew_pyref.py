"""Python restatement of the reference's motion de-skew of a LaserScan:
LaserDataProcessor::Process (laser_data_processor.cpp:43-120), DataCorrect
(:154-226) and BeamsUpdate (:231-314) with Transform2d (util/transform.h:52-103).

Independent of the library: Python floats (binary64, one rounding per
operation), numpy float32 for the two float steps of the beam angle (:58) and
the float32 the message stores (:115), tests/libm.sincos for every cos/sin
pair GCC merges, math.atan2 and math.sqrt. Written the way the reference is:
the ranges and angles vectors are rewritten in place segment by segment, so
an interior closing beam goes through BeamsUpdate twice. It pins
csm_deskew_ranges (the C++ restatement), which pins the device path
(tests/test_gpu_deskew.py).

Eigen as read here: AngleAxisd(a, z).toRotationMatrix() is [[c, 0 - s],
[0 + s, c]] with (c, s) from one sincos(a); a 3-vector product row is
(r0*p0 + r1*p1) + r2*p2 with r2*p2 a zero; Pose2d == compares per coefficient.

Also what both test files build their scans from (scans(), odometry(), batch()
...), and per scan the figure the device path's guard looks at (info["guard"]).
"""
import math

import numpy as np

from libm import sincos

PI = math.pi


def plan(n_beams, start_sec, end_sec, odom_interpolation_time):
    """DataCorrect's loop (:167-225) -> (closing beams, lookup times in s)."""
    if not start_sec < end_sec:  # Process :104
        return [], []
    T = int(odom_interpolation_time * 1e6)
    start_time = start_sec * 1e6
    end_time = end_sec * 1e6
    time_inc = (end_time - start_time) / n_beams
    start_index = 0
    close, look = [], []
    for i in range(n_beams):
        mid_time = start_time + time_inc * (i - start_index)
        if mid_time - start_time > T or i == n_beams - 1:
            close.append(i)
            look.append(mid_time / 1e6)
            start_time = mid_time
            start_index = i
    return close, look


class Transform2d:
    """transform.h:52-103, the x / y part."""

    def __init__(self, p1, p2):
        if p1[0] == p2[0] and p1[1] == p2[1] and p1[2] == p2[2]:  # :72-77
            self.R = ((1.0, 0.0), (0.0, 1.0))
            self.t = (0.0, 0.0)
            return
        c, s = sincos(p2[2] - p1[2])
        self.R = ((c, 0.0 - s), (0.0 + s, c))
        if p1[0] != 0.0 or p1[1] != 0.0:  # :85-88
            self.t = (p2[0] - ((self.R[0][0] * p1[0] + self.R[0][1] * p1[1]) + 0.0),
                      p2[1] - ((self.R[1][0] * p1[0] + self.R[1][1] * p1[1]) + 0.0))
        else:
            self.t = (p2[0], p2[1])

    def transform(self, x, y):  # :58-62
        R, t = self.R, self.t
        return (t[0] + ((R[0][0] * x + R[0][1] * y) + 0.0), t[1] + ((R[1][0] * x + R[1][1] * y) + 0.0))


def beams_update(base, start, end, ranges, angles, start_index, beam_number):
    """BeamsUpdate (:231-314); poses are (x, y, tf yaw)."""
    ya, yb = -start[2], -end[2]
    diff = yb - ya
    if diff > PI:
        ya += 2 * PI
    elif diff < -PI:
        yb += 2 * PI
    det_yaw = (yb - ya) / (beam_number - 1)
    det_x = (end[0] - start[0]) / (beam_number - 1)
    det_y = (end[1] - start[1]) / (beam_number - 1)
    base_frame = (base[0], base[1], -base[2])
    for i in range(start_index, start_index + beam_number):
        m = i - start_index
        c, s = sincos(angles[i])
        x, y = ranges[i] * c, ranges[i] * s
        mid = (start[0] + det_x * m, start[1] + det_y * m, ya + det_yaw * m)
        mx, my = Transform2d((0.0, 0.0, 0.0), mid).transform(x, y)
        bx, by = Transform2d(base_frame, (0.0, 0.0, 0.0)).transform(mx, my)
        ranges[i] = math.sqrt(bx * bx + by * by)
        angles[i] = math.atan2(by, bx)


def sanitised(scan, L):
    """Process :56-67 -> (ranges, angles) as Python floats."""
    ranges, angles = [], []
    for i in range(L.n_beams):
        r = float(scan[i])
        a = float(np.float32(L.angle_min + np.float32(L.angle_increment * np.float32(i))))
        if r < 0.05 or math.isnan(r) or math.isinf(r):
            r = 0.0
        ranges.append(r)
        angles.append(a)
    return ranges, angles


def quotient(angle, L):
    return (angle - float(L.angle_min)) / float(L.angle_increment)


def process_scan(L, scan, close, poses):
    """One scan -> (float32 [n_beams], info). close: the plan's closing beams
    (empty: the scan passes through), poses: len(close) + 1 (x, y, yaw).
    info: collisions (beams whose bin a later beam overwrote), dropped_low /
    dropped_high (j < 0, j >= n), guard (the smallest |q - rint(q)| over the
    beams the device bins itself -- every beam but the interior closing ones
    -- with rint(q) != 0; inf if none)."""
    n = L.n_beams
    scan = np.asarray(scan, dtype=np.float32)
    if not close:
        return scan.copy(), dict(collisions=0, dropped_low=0, dropped_high=0, guard=math.inf)
    ranges, angles = sanitised(scan, L)
    base = poses[0]
    start_index = 0
    for k, i in enumerate(close):
        beams_update(base, poses[k], poses[k + 1], ranges, angles, start_index, i - start_index + 1)
        start_index = i
    out = np.zeros(n, dtype=np.float32)
    written = [False] * n
    info = dict(collisions=0, dropped_low=0, dropped_high=0, guard=math.inf)
    interior = set(close[:-1])
    for i in range(n):
        q = quotient(angles[i], L)
        if i not in interior:
            if not math.isfinite(q):
                info["guard"] = 0.0
            elif round(q) != 0:
                info["guard"] = min(info["guard"], abs(q - round(q)))
        if not math.isfinite(q) or abs(q) >= 2147483648.0:  # defined here: dropped
            continue
        j = int(q)  # toward zero
        if j < 0:
            info["dropped_low"] += 1
            continue
        if j >= n:  # defined here: dropped
            info["dropped_high"] += 1
            continue
        if written[j]:
            info["collisions"] += 1
        written[j] = True
        out[j] = np.float32(ranges[i])
    return out, info


def process(L, ranges, seg_offsets, seg_close, poses):
    """The batch form of csm_deskew_ranges -> (float32 [n_scans, n_beams], [info])."""
    r = np.asarray(ranges, dtype=np.float32).reshape(-1, L.n_beams)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    out, infos = [], []
    for s in range(r.shape[0]):
        k0, k1 = int(seg_offsets[s]), int(seg_offsets[s + 1])
        P = [tuple(float(v) for v in poses[k0 + s + k]) for k in range(k1 - k0 + 1)] if k1 > k0 else []
        o, info = process_scan(L, r[s], [int(c) for c in seg_close[k0:k1]], P)
        out.append(o)
        infos.append(info)
    return np.array(out, dtype=np.float32).reshape(-1, L.n_beams), infos


GUARD = 2.0 ** -30  # the device path flags a scan with a beam closer than this to a nonzero integer


# ---- inputs -------------------------------------------------------------------

def even_closes(n_beams, K):
    """K segments of about equal length (K <= n_beams - 1)."""
    K = max(1, min(K, n_beams - 1))
    return [max(k + 1, ((k + 1) * (n_beams - 1)) // K) for k in range(K - 1)] + [n_beams - 1]


def odometry(rng, K, speed=0.5, turn=1.0, dt=0.005, start=None):
    """K + 1 poses (x, y, yaw) of seeded motion: speed m/s, turn rad/s, dt per segment."""
    x, y, yaw = start if start is not None else (rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3.0, 3.0))
    v, w = speed * rng.uniform(0.5, 1.5), turn * rng.uniform(-1.5, 1.5)
    P = [(x, y, yaw)]
    for _ in range(K):
        x += v * dt * math.cos(yaw) + rng.normal(0, 1e-4)
        y += v * dt * math.sin(yaw) + rng.normal(0, 1e-4)
        yaw += w * dt + rng.normal(0, 1e-4)
        P.append((x, y, yaw))
    return P


def scans(L, n_scans, rng, lo=0.3, hi=9.0):
    """Seeded ranges [n_scans, n_beams] float32, smooth along the scan with jumps."""
    n = L.n_beams
    t = np.linspace(0, 1, n)
    out = np.empty((n_scans, n), dtype=np.float32)
    for s in range(n_scans):
        base = rng.uniform(lo + 0.5, hi - 0.5)
        wave = sum(rng.uniform(0, 0.6) * np.sin(2 * PI * (f * t + rng.uniform())) for f in (1, 3, 7))
        step = np.where(t > rng.uniform(), rng.uniform(-0.5, 0.5), 0.0)
        out[s] = np.clip(base + wave + step, lo, hi).astype(np.float32)
    return out


def batch(L, n_scans, K, seed, **motion):
    """(ranges, seg_offsets, seg_close, poses) of n_scans moving scans of K segments each."""
    rng = np.random.default_rng(seed)
    r = scans(L, n_scans, rng)
    close = even_closes(L.n_beams, K)
    off, cl, ps = [0], [], []
    for _ in range(n_scans):
        cl += close
        ps += odometry(rng, len(close), **motion)
        off.append(len(cl))
    return r, np.array(off, dtype=np.int64), np.array(cl, dtype=np.int32), np.array(ps, dtype=np.float64).reshape(-1, 3)


def concat(parts):
    """Batches (ranges, off, close, poses) of one laser, back to back."""
    r = np.concatenate([p[0] for p in parts])
    off, cl, ps = [0], [], []
    for p in parts:
        off += [int(o) + off[-1] for o in p[1][1:]]
        cl.append(p[2])
        ps.append(np.asarray(p[3], dtype=np.float64).reshape(-1, 3))
    off = np.array(off, dtype=np.int64)
    return r, off, np.concatenate(cl).astype(np.int32), np.concatenate(ps)


def at_rest(L, n_scans, K, seed, pose=(1.25, -0.5, 0.75)):
    """Scans whose poses are all equal: every beam lands on a bin boundary up to rounding."""
    rng = np.random.default_rng(seed)
    r = scans(L, n_scans, rng)
    close = even_closes(L.n_beams, K)
    off = np.arange(n_scans + 1, dtype=np.int64) * len(close)
    cl = np.array(close * n_scans, dtype=np.int32)
    ps = np.array([pose] * ((len(close) + 1) * n_scans), dtype=np.float64)
    return r, off, cl, ps


def passthrough(L, n_scans, seed):
    """Scans with no segments (start >= end), with values Process would have sanitised."""
    rng = np.random.default_rng(seed)
    r = scans(L, n_scans, rng)
    r[:, ::5] = np.float32(0.01)
    r[:, 1::7] = np.float32(np.nan)
    r[:, 2::11] = np.float32(np.inf)
    # (a scan without segments still owns one pose slot, unread)
    return r, np.zeros(n_scans + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros((n_scans, 3))
