// csm_deskew_host.hpp — motion de-skew of raw laser scans on the host: the
// arithmetic of LaserDataProcessor::Process (laser_data_processor.cpp:43-120),
// DataCorrect (:154-226) and BeamsUpdate (:231-314) with Transform2d
// (util/transform.h:52-103), operation for operation (build with
// -ffp-contract=off). Pure host code over csm.h and host_math.hpp, so
// tests/cpp/deskew_check.cpp compiles it alone.
//
// tf is the caller's: deskew_plan says which times DataCorrect looks up, the
// caller passes (x, y, tf::getYaw) of each lookup.
//
// Eigen restated (3.3, as the reference uses it):
//   AngleAxisd(a, (0, 0, 1)).toRotationMatrix() has the upper-left block
//   [[c, 0 - s], [0 + s, c]] from one sincos(a) (GCC merges the pair), and
//   r02 = r12 = +0;
//   R * p of a 3-vector is (r0*p0 + r1*p1) + r2*p2 per row; the last term is
//   a zero here, restated as + 0.0;
//   Pose2d == Pose2d compares coefficient-wise (-0 == 0).
//
// Two undefined behaviours of Process get a defined result:
//   j >= n_beams (:115, an out-of-bounds write in the reference): the beam is
//   dropped;
//   a quotient (:113) that is not finite or whose magnitude is >= 2^31 (an
//   undefined double -> int conversion): the beam is dropped.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "csm.h"
#include "host_math.hpp"

#if defined(__HIPCC__)
#define CSM_DESKEW_HD __host__ __device__
#else
#define CSM_DESKEW_HD
#endif

namespace csm {
namespace deskew {

// Transform2d's rotation_ (upper-left block) and transform_ (x, y).
struct T2 {
  double r00, r01, r10, r11, tx, ty;
};

CSM_DESKEW_HD inline T2 identity_t2() { return T2{1.0, 0.0, 0.0, 1.0, 0.0, 0.0}; }

// AngleAxisd(angle, z).toRotationMatrix(), upper-left block, from sincos(angle)
CSM_DESKEW_HD inline void rotation_from_sincos(double s, double c, T2* t) {
  t->r00 = c;
  t->r01 = 0.0 - s;
  t->r10 = 0.0 + s;
  t->r11 = c;
}

// Transform2d(Pose2d(0, 0, 0), mid) with (s, c) = sincos(mid yaw - 0)
// (transform.h:71-95: pose_1 is zero, so transform_ = pose_2).
CSM_DESKEW_HD inline T2 mid_transform(double mx, double my, double myaw, double s, double c) {
  if (mx == 0.0 && my == 0.0 && myaw == 0.0) return identity_t2();  // :72-77
  T2 t;
  rotation_from_sincos(s, c, &t);
  t.tx = mx;
  t.ty = my;
  return t;
}

// Transform2d(base, Pose2d(0, 0, 0)), base = (bx, by, -yaw_base) (:289).
inline T2 base_transform(double bx, double by, double byaw) {
  if (bx == 0.0 && by == 0.0 && byaw == 0.0) return identity_t2();
  double s, c;
  host_sincos(0.0 - byaw, &s, &c);  // pose_2(2) - pose_1(2)
  T2 t;
  rotation_from_sincos(s, c, &t);
  if (bx != 0.0 || by != 0.0) {  // :85-88, new_position = pose_2 - rotation_ * pose_1
    t.tx = 0.0 - ((t.r00 * bx + t.r01 * by) + 0.0);
    t.ty = 0.0 - ((t.r10 * bx + t.r11 * by) + 0.0);
  } else {
    t.tx = 0.0;
    t.ty = 0.0;
  }
  return t;
}

// Transform2d::Transform (:58-62), x and y
CSM_DESKEW_HD inline void apply(const T2& t, double x, double y, double* ox, double* oy) {
  *ox = t.tx + ((t.r00 * x + t.r01 * y) + 0.0);
  *oy = t.ty + ((t.r10 * x + t.r11 * y) + 0.0);
}

// BeamsUpdate's per-segment interpolation (:247-265).
struct Segment {
  double x0, det_x, y0, det_y, ya, det_yaw;
  int32_t first, cnt;  // beams first ... first + cnt - 1
};

inline Segment make_segment(const double* start_pose, const double* end_pose, int32_t first, int32_t cnt) {
  Segment g;
  double ya = -start_pose[2], yb = -end_pose[2];
  const double diff = yb - ya;
  if (diff > M_PI)
    ya += 2 * M_PI;
  else if (diff < -M_PI)
    yb += 2 * M_PI;
  const double div = (double)(size_t)(cnt - 1);  // (beam_number - 1), a size_t
  g.ya = ya;
  g.det_yaw = (yb - ya) / div;
  g.x0 = start_pose[0];
  g.det_x = (end_pose[0] - start_pose[0]) / div;
  g.y0 = start_pose[1];
  g.det_y = (end_pose[1] - start_pose[1]) / div;
  g.first = first;
  g.cnt = cnt;
  return g;
}

// One beam of BeamsUpdate's second loop (:278-298): (r, a) in, (r, a) out.
// (ca, sa) = sincos(a), given by the caller (a table for a beam's first pass).
inline void update_beam(const Segment& g, int32_t m, const T2& base, double ca, double sa, double* r, double* a) {
  const double x = *r * ca, y = *r * sa;  // :281-282
  const double md = (double)m;
  const double myaw = g.ya + g.det_yaw * md, mx = g.x0 + g.det_x * md, my = g.y0 + g.det_y * md;  // :269-271
  double s = 0.0, c = 1.0;
  if (!(mx == 0.0 && my == 0.0 && myaw == 0.0)) host_sincos(myaw, &s, &c);
  const T2 tm = mid_transform(mx, my, myaw, s, c);
  double ox, oy, bx, by;
  apply(tm, x, y, &ox, &oy);
  apply(base, ox, oy, &bx, &by);
  *r = std::sqrt(bx * bx + by * by);  // :295
  *a = std::atan2(by, bx);            // :297
}

// Process :56-63, beam i of a scan
CSM_DESKEW_HD inline double sanitised_range(float r) {
  const double d = (double)r;
  return (d < 0.05 || std::isnan(d) || std::isinf(d)) ? 0.0 : d;
}
CSM_DESKEW_HD inline double beam_angle(const csm_laser& L, int32_t i) {
  const float m = L.angle_increment * (float)i;  // float arithmetic (:58)
  const float a = L.angle_min + m;
  return (double)a;
}

// Process :113-115 with the two undefined cases defined: the bin, or -1 for a
// beam that writes nothing.
inline int32_t beam_bin(double angle, double amin, double inc, int32_t n_beams) {
  const double q = (angle - amin) / inc;
  if (!std::isfinite(q) || std::fabs(q) >= 2147483648.0) return -1;
  const int32_t j = (int32_t)q;
  return (j < 0 || j >= n_beams) ? -1 : j;
}

// DataCorrect's segmentation (:167-225).
inline int plan(int32_t n_beams, double start_sec, double end_sec, double odom_interpolation_time,
                int32_t* seg_close, double* lookup_sec, int32_t capacity, int32_t* n_segments) {
  if (!n_segments || n_beams < 2 || capacity < 0 || (capacity > 0 && (!seg_close || !lookup_sec)))
    return CSM_ERR_INVALID_ARG;
  if (!std::isfinite(start_sec) || !std::isfinite(end_sec)) return CSM_ERR_INVALID_ARG;
  const double t_us = odom_interpolation_time * 1e6;
  if (!(t_us >= 0.0) || t_us >= 2147483648.0) return CSM_ERR_INVALID_ARG;  // negative: beam 0 would close alone
  *n_segments = 0;
  if (!(start_sec < end_sec)) return CSM_OK;  // Process :104
  const int T = (int)t_us;
  double start_time = start_sec * 1e6;
  const double end_time = end_sec * 1e6;
  const double inc = (end_time - start_time) / n_beams;
  int32_t start_index = 0, k = 0;
  for (int32_t i = 0; i < n_beams; ++i) {
    const double mid = start_time + inc * (i - start_index);
    if (mid - start_time > T || i == n_beams - 1) {
      if (k < capacity) {
        seg_close[k] = i;
        lookup_sec[k] = mid / 1e6;
      }
      ++k;
      start_time = mid;
      start_index = i;
    }
  }
  *n_segments = k;
  return k <= capacity ? CSM_OK : CSM_ERR_INVALID_ARG;
}

// The checks csm_deskew_ranges makes of a batch's plan and poses.
inline bool plan_valid(const csm_laser& L, int32_t n_scans, const int64_t* seg_offsets, const int32_t* seg_close,
                       const double* poses) {
  if (L.n_beams < 2 || !std::isfinite(L.angle_min) || !std::isfinite(L.angle_increment) ||
      L.angle_increment == 0.0f || n_scans < 0 || !seg_offsets || seg_offsets[0] != 0)
    return false;
  for (int32_t s = 0; s < n_scans; ++s) {
    const int64_t k0 = seg_offsets[s], k1 = seg_offsets[s + 1];
    if (k1 < k0) return false;
    if (k1 == k0) continue;
    if (!seg_close || !poses) return false;
    int32_t prev = 0;
    for (int64_t k = k0; k < k1; ++k) {
      if (seg_close[k] <= prev) return false;  // strictly increasing, the first past beam 0
      prev = seg_close[k];
    }
    if (prev != L.n_beams - 1) return false;
    for (int64_t p = (k0 + s) * 3; p < (k1 + s + 1) * 3; ++p)
      if (!std::isfinite(poses[p])) return false;
  }
  return true;
}

// Per-laser (cos, sin) of the float-arithmetic beam angles (:58, :281-282).
inline void beam_trig_table(const csm_laser& L, double* cs) {
  for (int32_t i = 0; i < L.n_beams; ++i) {
    double s, c;
    host_sincos(beam_angle(L, i), &s, &c);
    cs[2 * i] = c;
    cs[2 * i + 1] = s;
  }
}

// One scan of K >= 1 segments. close: K closing beams; poses: K + 1 (x, y, tf
// yaw). r and a are scratch of n_beams doubles each; cs the laser's table.
inline void deskew_scan(const csm_laser& L, const double* cs, const float* in, int32_t K, const int32_t* close,
                        const double* poses, double* r, double* a, float* out) {
  const int32_t n = L.n_beams;
  for (int32_t i = 0; i < n; ++i) {
    r[i] = sanitised_range(in[i]);
    a[i] = beam_angle(L, i);
  }
  const T2 base = base_transform(poses[0], poses[1], -poses[2]);  // frame_base_pose = the first start pose (:202)
  int32_t first = 0;
  for (int32_t k = 0; k < K; ++k) {
    const Segment g = make_segment(poses + 3 * k, poses + 3 * (k + 1), first, close[k] - first + 1);
    for (int32_t m = 0; m < g.cnt; ++m) {
      const int32_t i = first + m;
      double ca, sa;
      if (m == 0 && k > 0)  // a closing beam's second pass: its angle is the first's atan2
        host_sincos(a[i], &sa, &ca);
      else
        ca = cs[2 * i], sa = cs[2 * i + 1];
      update_beam(g, m, base, ca, sa, &r[i], &a[i]);
    }
    first = close[k];  // :222: the closing beam opens the next segment
  }
  for (int32_t i = 0; i < n; ++i) out[i] = 0.0f;  // :109-111
  const double amin = (double)L.angle_min, inc = (double)L.angle_increment;
  for (int32_t i = 0; i < n; ++i) {  // :112-116
    const int32_t j = beam_bin(a[i], amin, inc, n);
    if (j >= 0) out[j] = (float)r[i];
  }
}

// The interior closing beam close[k] (k < K - 1) of a scan, alone: its pass as
// the last beam of segment k, its pass as beam 0 of segment k + 1, its bin
// (-1: it writes nothing) and float range. What the device path leaves to the
// host: this beam's second pass reads the exact atan2 of its first.
inline void closing_beam(const csm_laser& L, const double* cs, const float* in, int32_t k, const int32_t* close,
                         const double* poses, const T2& base, int32_t* bin, float* range) {
  const int32_t i = close[k], first = k > 0 ? close[k - 1] : 0;
  double r = sanitised_range(in[i]), a = beam_angle(L, i);
  const Segment g0 = make_segment(poses + 3 * k, poses + 3 * (k + 1), first, i - first + 1);
  update_beam(g0, g0.cnt - 1, base, cs[2 * i], cs[2 * i + 1], &r, &a);
  const Segment g1 = make_segment(poses + 3 * (k + 1), poses + 3 * (k + 2), i, close[k + 1] - i + 1);
  double ca, sa;
  host_sincos(a, &sa, &ca);
  update_beam(g1, 0, base, ca, sa, &r, &a);
  *bin = beam_bin(a, (double)L.angle_min, (double)L.angle_increment, L.n_beams);
  *range = (float)r;
}

// Scan s of a batch (plan_valid holds) into `row` (n_beams floats; may be the
// scan's own ranges). r and a: scratch of n_beams doubles each.
inline void deskew_batch_scan(const csm_laser& L, const double* cs, int32_t s, const float* ranges,
                              const int64_t* seg_offsets, const int32_t* seg_close, const double* poses, double* r,
                              double* a, float* row) {
  const float* in = ranges + (int64_t)s * L.n_beams;
  const int64_t k0 = seg_offsets[s], K = seg_offsets[s + 1] - k0;
  if (K == 0) {  // Process :104 false: the message goes on as it came
    if (row != in) std::memmove(row, in, (size_t)L.n_beams * sizeof(float));
    return;
  }
  deskew_scan(L, cs, in, (int32_t)K, seg_close + k0, poses + (k0 + s) * 3, r, a, row);
}

// Scans [s0, s1) of a batch, scan s at out + s * n_beams.
inline void deskew_scans(const csm_laser& L, const double* cs, int32_t s0, int32_t s1, const float* ranges,
                         const int64_t* seg_offsets, const int32_t* seg_close, const double* poses, float* out) {
  std::vector<double> r((size_t)L.n_beams), a((size_t)L.n_beams);
  for (int32_t s = s0; s < s1; ++s)
    deskew_batch_scan(L, cs, s, ranges, seg_offsets, seg_close, poses, r.data(), a.data(),
                      out + (int64_t)s * L.n_beams);
}

}  // namespace deskew
}  // namespace csm
