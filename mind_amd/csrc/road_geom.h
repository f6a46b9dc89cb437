// Road geometry of the road audit, one text for the kernel k_road_boxes (road_kernels.hip) and the host entry mind_debug_road_margin: the
// signed margin of an oriented box's four corners to a drivable area given as P >= 1 rings (simple polygons, implicitly closed, no holes).
//
// Reference: every AV2 map carries `drivable_areas` beside `lane_segments`; the reference reads the file and never looks at them, so the
// definitions below are this project's.
//
// The order of operations is the contract (tests/road_geom_restate.py restates it in numpy, operation for operation):
//  - float64 throughout, no fma() here, and the including file compiles with floating-point contraction off;
//  - every length is an OFFSET from the box centre, never a world coordinate: a vertex enters as A = vertex - centre (the caller forms it,
//    rg_rel), a corner as its offset o from the centre, and the pair as a = A - o (box_geom.h gives the reason);
//  - (c, s) = (cos yaw, sin yaw) are inputs: the kernel takes them from mind_trig.h, the host entry may be handed them.
// Sign convention, the audit's: negative is bad.  Hit: margin < 0; touching (exactly 0.0, of either sign) is no hit.
//
// A ring of n vertices has the edges e = 0..n-1, edge e joining vertex e to vertex (e + 1) mod n; a walk visits them in that order and the
// rings in index order, so no result depends on who walks (one thread per box, any tile size, or the host).
//
// Point (a corner, offset o) against one ring, from the origin of a = A - o, b = B - o:
//  - zero-length edges: an edge whose end offsets are equal (A == B in both coordinates: a duplicated vertex) is SKIPPED by both passes
//    below -- the rule lives here (rg_edge), not in a caller;
//  - inside: the parity of the edges crossing the +x ray from the origin, half open and without a division: edge e counts when
//    (a.y > 0) != (b.y > 0) and cr = a.x b.y - a.y b.x has the sign of b.y - a.y (b.y > a.y ? cr > 0 : cr < 0).  A ray through a vertex
//    or along a horizontal edge is then counted consistently; a point exactly on an edge (cr == 0) does not count it;
//  - distance: the minimum over the edges of the squared clamped point-segment distance, with E = B - A, ll = E.E, rl = 1 / ll (formed
//    once per edge, shared by the four corners) and t = -(a.E):  t <= 0: a.a;  t >= ll: b.b;  otherwise (cr cr) rl.  Squared distances
//    are compared, the lowest edge index wins ties (two edges meeting in the nearest vertex tie exactly) and is reported; ONE sqrt per
//    ring.  A ring all of whose edges are skipped reports +inf, outside, edge -1.
// Point against the road:
//  - in at least one ring: margin = the maximum over the CONTAINING rings of that ring's distance, the lowest ring winning ties;
//  - otherwise: margin = -(the minimum over ALL rings of the distance), the lowest ring winning ties.
//  Outside, that is the exact distance to the road.  Inside, it is a LOWER BOUND of the distance to the boundary of the rings' union: exact
//  wherever the rings neither overlap nor abut near the point, too small where the nearest edge of the containing ring is shared with (or
//  covered by) a neighbouring ring.
// Box against the road: margin = the minimum of the four corner margins, corners in box_geom.h's order (+,+), (+,-), (-,-), (-,+) of
// (long, lat), the first minimum winning; its corner, ring and edge (index within the ring) are reported with it.  Corners only: a box
// whose corners all lie inside while a sliver of verge passes under its middle is not detected.
#pragma once

#if defined(__HIPCC__)
#define RG_FN __host__ __device__ __forceinline__
#else
#define RG_FN static inline
#endif

typedef struct {
  double ox, oy;                      // the corner's offset from the box centre
  double d2; int par, edge;           // the ring being walked: least squared distance, its edge, crossings so far
  double in_d, out_d;                 // across the rings done: the greatest distance of a containing ring; the least of all rings
  int in_ring, in_edge, out_ring, out_edge;
} rg_corner;

// a world coordinate pair as an offset from the centre of the box at (px, py) carried `off` along (c, s)
RG_FN void rg_rel(double vx, double vy, double px, double py, double off, double c, double s, double *Ax, double *Ay) {
  *Ax = (vx - px) - off * c;
  *Ay = (vy - py) - off * s;
}

RG_FN void rg_box_begin(rg_corner q[4], double c, double s, double L, double W) {
  const double hl = 0.5 * L, hw = 0.5 * W;
  const double sl[4] = {1.0, 1.0, -1.0, -1.0}, sw[4] = {1.0, -1.0, -1.0, 1.0};
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    const double lx = sl[k] * hl, ly = sw[k] * hw;
    q[k].ox = c * lx - s * ly;
    q[k].oy = s * lx + c * ly;
    q[k].in_d = 0.0; q[k].out_d = 0.0;
    q[k].in_ring = -1; q[k].in_edge = -1; q[k].out_ring = -1; q[k].out_edge = -1;
    q[k].d2 = 0.0; q[k].par = 0; q[k].edge = -1;
  }
}

RG_FN void rg_ring_begin(rg_corner q[4]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) { q[k].d2 = INFINITY; q[k].par = 0; q[k].edge = -1; }
}

// edge e of the ring being walked, from A to B (offsets from the box centre), against the four corners
RG_FN void rg_edge(rg_corner q[4], double Ax, double Ay, double Bx, double By, int e) {
  if (Ax == Bx && Ay == By) return;
  const double Ex = Bx - Ax, Ey = By - Ay;
  const double ll = Ex * Ex + Ey * Ey;
  const double rl = 1.0 / ll;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    const double ax = Ax - q[k].ox, ay = Ay - q[k].oy, bx = Bx - q[k].ox, by = By - q[k].oy;
    const double cr = ax * by - ay * bx;
    if ((ay > 0.0) != (by > 0.0)) {
      if (by > ay ? cr > 0.0 : cr < 0.0) q[k].par ^= 1;
    }
    const double t = -(ax * Ex + ay * Ey);
    double d2;
    if (t <= 0.0) d2 = ax * ax + ay * ay;
    else if (t >= ll) d2 = bx * bx + by * by;
    else d2 = (cr * cr) * rl;
    if (d2 < q[k].d2) { q[k].d2 = d2; q[k].edge = e; }
  }
}

// ring r has been walked: fold it into the across-ring state
RG_FN void rg_ring_end(rg_corner q[4], int r) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    const double d = sqrt(q[k].d2);
    if (q[k].par && (q[k].in_ring < 0 || d > q[k].in_d)) { q[k].in_d = d; q[k].in_ring = r; q[k].in_edge = q[k].edge; }
    if (q[k].out_ring < 0 || d < q[k].out_d) { q[k].out_d = d; q[k].out_ring = r; q[k].out_edge = q[k].edge; }
  }
}

// every ring has been walked: the box's margin with its corner, ring and edge
RG_FN double rg_box_end(const rg_corner q[4], int *corner, int *ring, int *edge) {
  double best = 0.0;
  int bk = -1, br = -1, be = -1;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 4; ++k) {
    const bool in = q[k].in_ring >= 0;
    const double m = in ? q[k].in_d : -q[k].out_d;
    if (k == 0 || m < best) { best = m; bk = k; br = in ? q[k].in_ring : q[k].out_ring; be = in ? q[k].in_edge : q[k].out_edge; }
  }
  *corner = bk; *ring = br; *edge = be;
  return best;
}

// the whole walk in one piece (the host entry; the kernel walks the same calls in the same order over its staged tiles): the box of
// length L, width W at (px, py), carried `off` along (c, s), against the road verts [V, 2] / poly_off [P + 1]
RG_FN double rg_box_road(double px, double py, double c, double s, double L, double W, double off, const double *verts, const int *poly_off,
                         int P, int *corner, int *ring, int *edge) {
  rg_corner q[4];
  rg_box_begin(q, c, s, L, W);
  for (int r = 0; r < P; ++r) {
    const int v0 = poly_off[r], n = poly_off[r + 1] - v0;
    double Fx, Fy, Ax, Ay, Bx, By;
    rg_rel(verts[(long)v0 * 2], verts[(long)v0 * 2 + 1], px, py, off, c, s, &Fx, &Fy);
    Ax = Fx; Ay = Fy;
    rg_ring_begin(q);
    for (int i = 1; i < n; ++i) {
      rg_rel(verts[(long)(v0 + i) * 2], verts[(long)(v0 + i) * 2 + 1], px, py, off, c, s, &Bx, &By);
      rg_edge(q, Ax, Ay, Bx, By, i - 1);
      Ax = Bx; Ay = By;
    }
    rg_edge(q, Ax, Ay, Fx, Fy, n - 1);
    rg_ring_end(q, r);
  }
  return rg_box_end(q, corner, ring, edge);
}
