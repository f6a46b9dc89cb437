// Swept-box geometry of the time-to-collision audit, one text for the kernel (k_audit_ttc: ttc_kernels.hip) and the host entry
// mind_debug_box_ttc: the first time at which two oriented rectangles that translate at constant velocity overlap.
//
// Reference: every agent carries a BBox by object type (agent.py:92-105, common/bbox.py) drawn centred on state[:2] (visualization.py:69-72);
// the reference never tests one box against anything, moving or not, so the definition below is this project's.  It is exact: rectangles
// that translate keep their orientations, so the four separating axes of bg_rect_rect (box_geom.h) are constant in time, the boxes overlap
// exactly while the offset's projection on every axis lies strictly inside that axis' reach, and each such condition is an open interval
// of time with a closed form.  No time sampling.
//
// The order of operations is the contract (tests/ttc_geom_restate.py restates it in numpy, operation for operation):
//  - float64 throughout, no fma() here, and the including file compiles with floating-point contraction off;
//  - every length is an OFFSET from the centre of box A, never a world coordinate (box_geom.h says why);
//  - (c, s) = (cos yaw, sin yaw) are inputs: the kernel takes them from mind_trig.h, the host entry may be handed them;
//  - min / max are the comparisons spelled below, not fmin / fmax.
// Conventions:
//  - boxes that overlap now give 0.0;
//  - boxes that only touch at an instant (corners grazing), or slide along each other in contact, are no hit -- "touching is no hit", as
//    everywhere else -- and give +inf; so do two point boxes (every reach is 0: no open interval);
//  - there is no horizon in here: it is the caller's, who reports a result above it as +inf;
//  - the set ttc == 0 and the set bg_rect_rect < 0 may differ in the last ulp of a boundary case: (|p| - a) - b < 0 and |p| < a + b round
//    differently.  Nothing may hold them equal closer than 1e-9 m.
#pragma once

#if defined(__HIPCC__)
#define TG_FN __host__ __device__ __forceinline__
#else
#define TG_FN static inline
#endif

// One separating axis u = (ux, uy) of reach R: the offset's projection p + q t lies in (-R, R) for t in (lo, hi); the running
// intersection (enter, exit) takes it in.  An axis the relative velocity does not move along (q == 0.0) constrains nothing when the
// boxes' shadows on it overlap, and separates them for ever otherwise: 0.
TG_FN int tg_axis(double ux, double uy, double R, double dx, double dy, double wx, double wy, double *enter, double *exit_) {
  const double p = ux * dx + uy * dy;
  const double q = ux * wx + uy * wy;
  if (q == 0.0) return fabs(p) < R ? 1 : 0;
  const double t1 = ((-R) - p) / q;
  const double t2 = (R - p) / q;
  const double lo = t1 < t2 ? t1 : t2, hi = t1 < t2 ? t2 : t1;
  if (lo > *enter) *enter = lo;
  if (hi < *exit_) *exit_ = hi;
  return 1;
}

// Time of first overlap of the rectangles A (ca, sa, La, Wa) and B (cb, sb, Lb, Wb); (dx, dy) = centre of B - centre of A at time 0,
// (wx, wy) = velocity of B - velocity of A.  The axes in bg_rect_rect's order, A-long, A-lat, B-long, B-lat, each with the sum of the two
// boxes' projected half-extents as bg_rect_rect forms them.  +inf: never (under these velocities).
TG_FN double tg_rect_rect_ttc(double dx, double dy, double wx, double wy, double ca, double sa, double La, double Wa, double cb, double sb, double Lb,
                              double Wb) {
  const double hla = 0.5 * La, hwa = 0.5 * Wa, hlb = 0.5 * Lb, hwb = 0.5 * Wb;
  const double cc = fabs(ca * cb + sa * sb);        // |A-long . B-long| = |A-lat . B-lat|
  const double cs = fabs(sa * cb - ca * sb);        // |A-long . B-lat| = |A-lat . B-long|
  const double R0 = hla + (hlb * cc + hwb * cs);
  const double R1 = hwa + (hlb * cs + hwb * cc);
  const double R2 = (hla * cc + hwa * cs) + hlb;
  const double R3 = (hla * cs + hwa * cc) + hwb;
  double enter = -INFINITY, exit_ = INFINITY;
  if (!tg_axis(ca, sa, R0, dx, dy, wx, wy, &enter, &exit_)) return INFINITY;
  if (!tg_axis(-sa, ca, R1, dx, dy, wx, wy, &enter, &exit_)) return INFINITY;
  if (!tg_axis(cb, sb, R2, dx, dy, wx, wy, &enter, &exit_)) return INFINITY;
  if (!tg_axis(-sb, cb, R3, dx, dy, wx, wy, &enter, &exit_)) return INFINITY;
  return enter < exit_ && exit_ > 0.0 ? (enter > 0.0 ? enter : 0.0) : INFINITY;
}
