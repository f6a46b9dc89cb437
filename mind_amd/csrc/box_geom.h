// Footprint geometry of the clearance audit, one text for the two audit kernels (k_audit_plan, k_audit_episode: audit_kernels.hip) and the
// host entry mind_debug_box_clearance: signed distance of a point to an oriented rectangle and signed clearance of two oriented rectangles.
//
// Reference: every agent carries a BBox by object type (agent.py:92-105, common/bbox.py) drawn centred on state[:2] (visualization.py:69-72);
// the reference never tests one box against anything, so the definitions below are this project's.
//
// The order of operations is the contract (tests/box_geom_restate.py restates it in numpy, operation for operation):
//  - float64 throughout, no fma() here, and the including file compiles with floating-point contraction off;
//  - every length is an OFFSET from one box centre, never a world coordinate (AV2 coordinates are thousands of metres: a corner formed as
//    cx + ... would carry 1e-12 m of rounding that depends on the last bit of the cosine);
//  - (c, s) = (cos yaw, sin yaw) are inputs: the kernels take them from mind_trig.h, the host entry may be handed them.
// Hit convention everywhere: clearance < 0.  Touching (exactly 0.0) is no hit.
#pragma once

#if defined(__HIPCC__)
#define BG_FN __host__ __device__ __forceinline__
#else
#define BG_FN static inline
#endif

// Signed distance of the point (dx, dy), given as an offset from the rectangle's centre, to the rectangle of length L (along (c, s)) and
// width W: > 0 outside (Euclidean distance to the boundary), <= 0 inside (minus the distance to the nearest edge).
BG_FN double bg_point_rect(double dx, double dy, double c, double s, double L, double W) {
  const double u = c * dx + s * dy;
  const double v = (-s) * dx + c * dy;
  const double qx = fabs(u) - 0.5 * L;
  const double qy = fabs(v) - 0.5 * W;
  if (qx > 0.0 || qy > 0.0) {
    const double mx = qx > 0.0 ? qx : 0.0, my = qy > 0.0 ? qy : 0.0;
    return sqrt(mx * mx + my * my);
  }
  return qx > qy ? qx : qy;
}

// Signed clearance of the rectangles A (ca, sa, La, Wa) and B (cb, sb, Lb, Wb); (dx, dy) = centre of B - centre of A.
//  1. separating axes: for the four edge directions u = A-long, A-lat, B-long, B-lat: d = |D.u| - r_A(u) - r_B(u) with the projected
//     half-extents r(u) = L/2 |u.long| + W/2 |u.lat| (a box's own axes give L/2 and W/2 themselves); sep = max d, the first axis wins ties.
//  2. sep <= 0: the boxes overlap or touch, the result is sep (the least penetration, negative).
//  3. otherwise the boxes are disjoint convex polygons and their distance is attained at a corner of one of them: the minimum of
//     bg_point_rect of the four corners of A against B, then of the four corners of B against A, corners in the order
//     (+,+), (+,-), (-,-), (-,+) of (long, lat); the first minimum wins.
BG_FN double bg_rect_rect(double dx, double dy, double ca, double sa, double La, double Wa, double cb, double sb, double Lb, double Wb) {
  const double hla = 0.5 * La, hwa = 0.5 * Wa, hlb = 0.5 * Lb, hwb = 0.5 * Wb;
  const double cc = fabs(ca * cb + sa * sb);        // |A-long . B-long| = |A-lat . B-lat|
  const double cs = fabs(sa * cb - ca * sb);        // |A-long . B-lat| = |A-lat . B-long|
  const double d0 = (fabs(ca * dx + sa * dy) - hla) - (hlb * cc + hwb * cs);
  const double d1 = (fabs((-sa) * dx + ca * dy) - hwa) - (hlb * cs + hwb * cc);
  const double d2 = (fabs(cb * dx + sb * dy) - (hla * cc + hwa * cs)) - hlb;
  const double d3 = (fabs((-sb) * dx + cb * dy) - (hla * cs + hwa * cc)) - hwb;
  double sep = d0;
  if (d1 > sep) sep = d1;
  if (d2 > sep) sep = d2;
  if (d3 > sep) sep = d3;
  if (sep <= 0.0) return sep;
  const double sl[4] = {1.0, 1.0, -1.0, -1.0}, sw[4] = {1.0, -1.0, -1.0, 1.0};
  double best = 0.0;
  for (int k = 0; k < 4; ++k) {                     // corners of A, as offsets from B's centre
    const double lx = sl[k] * hla, ly = sw[k] * hwa;
    const double ox = ca * lx - sa * ly, oy = sa * lx + ca * ly;
    const double d = bg_point_rect(ox - dx, oy - dy, cb, sb, Lb, Wb);
    if (k == 0 || d < best) best = d;
  }
  for (int k = 0; k < 4; ++k) {                     // corners of B, as offsets from A's centre
    const double lx = sl[k] * hlb, ly = sw[k] * hwb;
    const double ox = cb * lx - sb * ly, oy = sb * lx + cb * ly;
    const double d = bg_point_rect(dx + ox, dy + oy, ca, sa, La, Wa);
    if (d < best) best = d;
  }
  return best;
}
