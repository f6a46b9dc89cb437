// Road audit: what a plan's trajectory trees and a closed-loop episode did to the ROAD -- the ego box against the drivable area, computed
// from road_geom.h.
//
// k_road_boxes: n boxes, each one state row (x, y, .., yaw) of `stride` doubles, against the road verts [V, 2] / poly_off [P + 1]: per box
// the margin (road_geom.h: the least corner margin, negative off the road) with its corner, ring and edge.  A row holding a non-finite
// value reports NaN / -1 / -1 / -1.
//
// Shape.  A workgroup = RD_BB consecutive boxes, thread = box: all four corners of a box live in one thread's registers (rg_corner x 4:
// parity, least squared distance and its edge of the ring being walked, the across-ring state), so the fold over corners needs no
// exchange.  The vertices -- what every box shares -- are read from global memory once per workgroup, RD_TV at a time: thread i of a
// turn loads vertex v0 + i as one 16-byte (x, y) pair, consecutive lanes consecutive addresses, into LDS; the walk then reads staged
// vertex j in every lane at once -- one address, a broadcast, no bank conflict.  A ring may straddle turns: its first vertex and the
// previous vertex stay in registers, and a ring is folded (rg_ring_end) when its last vertex has been walked, edges in index order; the
// ring bounds come from poly_off by a wave-uniform index.  No result depends on RD_BB, RD_TV or the grid.  No atomics.
// The per-tree / per-ego reductions are the clearance audit's (audit_kernels.hip: k_audit_plan_trees, k_audit_episode_egos<true>), and so
// is the ego box (AuBox).
// Included by mind_hip.hip behind forecast_kernels.hip.
#pragma clang fp contract(off)
#include "road_geom.h"

#define RD_BB 256          // boxes per workgroup = threads
#define RD_TV 256          // vertices staged at a time (4 KB of LDS)

__global__ __launch_bounds__(RD_BB) void k_road_boxes(AuBox ego, long n_boxes, const double *__restrict__ states, int stride, int iyaw,
                                                      const double *__restrict__ verts, const int *__restrict__ poly_off, int V,
                                                      double *__restrict__ margin, int *__restrict__ corner, int *__restrict__ ring,
                                                      int *__restrict__ edge) {
  __shared__ double2 tile[RD_TV];
  const int tid = threadIdx.x;
  const long g = (long)blockIdx.x * RD_BB + tid;
  const bool act = g < n_boxes;
  const double *x = states + (size_t)(act ? g : 0) * (size_t)stride;      // (idle lanes shadow the first box and store nothing)
  bool ok = true;
  for (int q = 0; q < stride; ++q) ok = ok && au_finite(x[q]);
  const double px = ok ? x[0] : 0.0, py = ok ? x[1] : 0.0;
  double sn, cs;
  mind_sincos(ok ? x[iyaw] : 0.0, &sn, &cs);
  rg_corner q[4];
  rg_box_begin(q, cs, sn, ego.L, ego.W);
  int r = 0, rbeg = 0, rend = poly_off[1];
  double Fx = 0.0, Fy = 0.0, Ax = 0.0, Ay = 0.0;
  for (int v0 = 0; v0 < V; v0 += RD_TV) {
    if (v0 > 0) __syncthreads();
    if (v0 + tid < V) tile[tid] = reinterpret_cast<const double2 *>(verts)[v0 + tid];
    __syncthreads();
    const int nv = V - v0 < RD_TV ? V - v0 : RD_TV;
    for (int j = 0; j < nv; ++j) {
      const int gv = v0 + j;
      const double2 w = tile[j];
      double Bx, By;
      rg_rel(w.x, w.y, px, py, ego.off, cs, sn, &Bx, &By);
      if (gv == rbeg) {
        Fx = Bx; Fy = By;
        rg_ring_begin(q);
      } else {
        rg_edge(q, Ax, Ay, Bx, By, gv - 1 - rbeg);
      }
      Ax = Bx; Ay = By;
      if (gv + 1 == rend) {
        rg_edge(q, Ax, Ay, Fx, Fy, gv - rbeg);
        rg_ring_end(q, r);
        ++r;
        rbeg = rend;
        rend = poly_off[r + 1];         // (poly_off holds P + 2 entries on the device: the last repeats V)
      }
    }
  }
  int bk, br, be;
  double m = rg_box_end(q, &bk, &br, &be);
  if (!ok) { m = NAN; bk = -1; br = -1; be = -1; }
  if (act) { margin[g] = m; corner[g] = bk; ring[g] = br; edge[g] = be; }
}
