// Lane geometry of the lane audit, one text for the kernel k_lane_boxes (lane_kernels.hip) and the host entry mind_debug_lane_project: the
// projection of an oriented box's centre on P >= 1 lane centrelines -- the lateral offset, the arc length, the heading against the direction
// of travel -- once over every segment (`any`) and once over the segments that go the box's way (`flow`).
//
// Reference: the reference projects one pose at a time on one polyline in Python (project_point_on_polyline, get_closest_semantic_lane) and
// scores no trace with it, so the definitions below are this project's.
//
// The order of operations is the contract (tests/lane_geom_restate.py restates it in numpy, operation for operation):
//  - float64 throughout, no fma() here, and the including file compiles with floating-point contraction off;
//  - every length is an OFFSET from the box centre, never a world coordinate: a vertex enters as A = vertex - centre (rg_rel of road_geom.h,
//    the centre being (x, y) + center_offset (c, s));
//  - (c, s) = (cos yaw, sin yaw) are inputs: the kernel takes them from mind_trig.h, the host entry may be handed them.
//
// Lanes: verts [V, 2] and lane_off [P + 1]; lane l is the OPEN polyline verts[lane_off[l] : lane_off[l + 1]] of at least two vertices, its
// vertex order the direction of travel.  Segment g -- the global index of its first vertex -- joins vertex g to vertex g + 1; the pair
// (last vertex of lane l, first vertex of lane l + 1) is NOT a segment.  cum [V] is the arc length at a vertex from its lane's first
// vertex (lg_cum: a sequential sum from 0.0 per lane of sqrt(dx dx + dy dy) over world-coordinate differences), formed once per call.
//
// One segment against the centre (lg_seg), offsets A, B:
//  - a segment whose end offsets are equal (A == B in both coordinates: a duplicated vertex) is SKIPPED -- the rule lives here;
//  - E = B - A, ll = E.E, rl = 1 / ll, t = -(A.E), cr = A.x B.y - A.y B.x;
//  - d2 = A.A if t <= 0; B.B if t >= ll; else (cr cr) rl;
//  - along = (c E.x + s E.y) / sqrt(ll).
// Two running minima per box, each over the key (d2, g) in lexicographic order (lg_take): `any` over every segment, `flow` over the
// segments with along >= cos_flow.  Replacement is strict < on d2, then the lower g: a NaN (or +inf) d2 never wins.  That minimum is
// associative and commutative, so the result is the sequential scan's bit for bit whoever walks (one thread per box, 64 lanes over the
// segments, any tile size, or the host).
// The winner's details (lg_finish), recomputed from g by the same formulas:
//  - dist = sqrt(d2); lat = cr >= 0 ? dist : -dist -- positive when the centre is LEFT of the direction of travel;
//  - s = cum[g] + clamp(t, 0, ll) / sqrt(ll);
//  - along as above, across = (s E.x - c E.y) / sqrt(ll) with s = sin yaw -- positive when the heading points left of the lane;
//  - lane = the l containing g, edge = g - lane_off[l].
// No winner (no qualifying segment): lat = +inf, lane = edge = -1, s = along = across = NaN.
// Margin (lg_margin), the audit's sign convention -- negative is bad: bound - |lat of flow|; a hit is margin < 0, exactly 0 is none;
// -inf when no segment goes the box's way.  A non-finite state row reports every double NaN, every index -1, the margin NaN (the callers'
// rule: lg_out_nan).
// No atan2 here: the heading error is arctan2(across, along), left to Python.
#pragma once
#include "road_geom.h"

#define LG_FN RG_FN

typedef struct { double d2; int g; } lg_min;                  // a running minimum over the key (d2, g); g = -1: none yet
typedef struct { lg_min any, flow; } lg_walk;
typedef struct { double lat, s, along, across; int lane, edge; } lg_out;

LG_FN void lg_begin(lg_walk *q) {
  q->any.d2 = INFINITY; q->any.g = -1;
  q->flow.d2 = INFINITY; q->flow.g = -1;
}

// (d2, g) against the running minimum, and one running minimum against another (the lanes' fold)
LG_FN void lg_take(lg_min *m, double d2, int g) {
  if (d2 < m->d2 || (d2 == m->d2 && g < m->g)) { m->d2 = d2; m->g = g; }
}

// the segment from A to B (offsets from the box centre): false when it is skipped; else its squared distance and the heading's cosine
// against it, with the terms lg_finish needs
LG_FN bool lg_seg(double Ax, double Ay, double Bx, double By, double c, double s, double *d2, double *along, double *t_out, double *ll_out,
                  double *cr_out, double *across) {
  if (Ax == Bx && Ay == By) return false;
  const double Ex = Bx - Ax, Ey = By - Ay;
  const double ll = Ex * Ex + Ey * Ey;
  const double rl = 1.0 / ll;
  const double t = -(Ax * Ex + Ay * Ey);
  const double cr = Ax * By - Ay * Bx;
  if (t <= 0.0) *d2 = Ax * Ax + Ay * Ay;
  else if (t >= ll) *d2 = Bx * Bx + By * By;
  else *d2 = (cr * cr) * rl;
  const double len = sqrt(ll);
  *along = (c * Ex + s * Ey) / len;
  *across = (s * Ex - c * Ey) / len;
  *t_out = t; *ll_out = ll; *cr_out = cr;
  return true;
}

// segment g against both running minima
LG_FN void lg_edge(lg_walk *q, double Ax, double Ay, double Bx, double By, double c, double s, double cos_flow, int g) {
  double d2, along, t, ll, cr, across;
  if (!lg_seg(Ax, Ay, Bx, By, c, s, &d2, &along, &t, &ll, &cr, &across)) return;
  lg_take(&q->any, d2, g);
  if (along >= cos_flow) lg_take(&q->flow, d2, g);
}

// the lane holding vertex g: the l with lane_off[l] <= g < lane_off[l + 1]
LG_FN int lg_lane_of(const int *lane_off, int P, int g) {
  int lo = 0, hi = P;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (lane_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

LG_FN void lg_out_nan(lg_out *o) {
  o->lat = NAN; o->s = NAN; o->along = NAN; o->across = NAN; o->lane = -1; o->edge = -1;
}

// the details of a running minimum's winner, recomputed from its segment
LG_FN void lg_finish(const lg_min *m, double px, double py, double c, double s, double off, const double *verts, const int *lane_off, int P,
                     const double *cum, lg_out *o) {
  if (m->g < 0) {
    o->lat = INFINITY; o->s = NAN; o->along = NAN; o->across = NAN; o->lane = -1; o->edge = -1;
    return;
  }
  const long g = m->g;
  double Ax, Ay, Bx, By, d2, along, t, ll, cr, across;
  rg_rel(verts[g * 2], verts[g * 2 + 1], px, py, off, c, s, &Ax, &Ay);
  rg_rel(verts[g * 2 + 2], verts[g * 2 + 3], px, py, off, c, s, &Bx, &By);
  lg_seg(Ax, Ay, Bx, By, c, s, &d2, &along, &t, &ll, &cr, &across);
  const double dist = sqrt(d2);
  o->lat = cr >= 0.0 ? dist : -dist;
  const double tc = t <= 0.0 ? 0.0 : (t >= ll ? ll : t);
  o->s = cum[g] + tc / sqrt(ll);
  o->along = along;
  o->across = across;
  o->lane = lg_lane_of(lane_off, P, (int)g);
  o->edge = (int)g - lane_off[o->lane];
}

LG_FN double lg_margin(double bound, double lat_flow) { return bound - fabs(lat_flow); }

// the arc length at every vertex from its lane's first vertex
LG_FN void lg_cum(const double *verts, const int *lane_off, int P, double *cum) {
  for (int l = 0; l < P; ++l) {
    double acc = 0.0;
    cum[lane_off[l]] = acc;
    for (long v = (long)lane_off[l] + 1; v < lane_off[l + 1]; ++v) {
      const double dx = verts[v * 2] - verts[v * 2 - 2], dy = verts[v * 2 + 1] - verts[v * 2 - 1];
      acc = acc + sqrt(dx * dx + dy * dy);
      cum[v] = acc;
    }
  }
}

// the whole walk in one piece (the host entry; the kernel walks the same calls over its staged tiles): the centre of the box at (px, py)
// carried `off` along (c, s) against the lanes verts [V, 2] / lane_off [P + 1] / cum [V] -> out[0] = any, out[1] = flow; the margin
LG_FN double lg_box_lanes(double px, double py, double c, double s, double off, double cos_flow, double bound, const double *verts,
                          const int *lane_off, int P, const double *cum, lg_out out[2]) {
  lg_walk q;
  lg_begin(&q);
  for (int l = 0; l < P; ++l) {
    const int v0 = lane_off[l], v1 = lane_off[l + 1];
    double Ax, Ay, Bx, By;
    rg_rel(verts[(long)v0 * 2], verts[(long)v0 * 2 + 1], px, py, off, c, s, &Ax, &Ay);
    for (int v = v0 + 1; v < v1; ++v) {
      rg_rel(verts[(long)v * 2], verts[(long)v * 2 + 1], px, py, off, c, s, &Bx, &By);
      lg_edge(&q, Ax, Ay, Bx, By, c, s, cos_flow, v - 1);
      Ax = Bx; Ay = By;
    }
  }
  lg_finish(&q.any, px, py, c, s, off, verts, lane_off, P, cum, &out[0]);
  lg_finish(&q.flow, px, py, c, s, off, verts, lane_off, P, cum, &out[1]);
  return lg_margin(bound, out[1].lat);
}
