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
// k_road_plan_trees / k_road_episode_egos: one thread per (candidate, tree) / per ego, sequential in key / step order.
// Included by mind_hip.hip behind forecast_kernels.hip.
#pragma clang fp contract(off)
#include "road_geom.h"

#define RD_BB 256          // boxes per workgroup = threads
#define RD_TV 256          // vertices staged at a time (4 KB of LDS)

struct RdBox { double L, W, off; };                 // mind_audit_box

__global__ __launch_bounds__(RD_BB) void k_road_boxes(RdBox ego, long n_boxes, const double *__restrict__ states, int stride, int iyaw,
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

// per (candidate, tree): the least margin with its node and corner (the lowest key wins ties), the nodes off the road, the first of them
// and their probability mass.  A tree holding a NaN node reports min = NaN, node = the lowest such key, corner = -1, hits = -1,
// first = -1, mass = NaN (the rule of k_audit_plan_trees).
__global__ __launch_bounds__(256) void k_road_plan_trees(int Mtot, int n_cand, int n_trees, const AuTree *__restrict__ trees,
                                                         const float *__restrict__ prob, const double *__restrict__ node_margin,
                                                         const int *__restrict__ node_corner, double *__restrict__ tree_min,
                                                         int *__restrict__ tree_node, int *__restrict__ tree_corner, int *__restrict__ tree_hits,
                                                         int *__restrict__ tree_first, double *__restrict__ tree_mass) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)n_cand * n_trees) return;
  const int c = (int)(e / n_trees), t = (int)(e % n_trees);
  const AuTree T = trees[t];
  const size_t row = (size_t)c * (size_t)Mtot + (size_t)T.moff;
  double mn = INFINITY, mass = 0.0;
  int mi = -1, mc = -1, hits = 0, first = -1, bad = -1;
  for (int i = 0; i < T.M; ++i) {
    const double d = node_margin[row + i];
    if (d != d) { bad = i; break; }
    if (i == 0 || d < mn) { mn = d; mi = i; mc = node_corner[row + i]; }
    if (d < 0.0) {
      if (first < 0) first = i;
      ++hits;
      mass += (double)prob[T.moff + i];
    }
  }
  if (bad >= 0) { mn = NAN; mi = bad; mc = -1; hits = -1; first = -1; mass = NAN; }
  tree_min[e] = mn; tree_node[e] = mi; tree_corner[e] = mc; tree_hits[e] = hits; tree_first[e] = first; tree_mass[e] = mass;
}

// per ego: the least margin over the steps with its step and corner (the lowest step wins ties), the steps off the road and the first of
// them.  A trace holding a NaN step reports min = NaN, step = the first such step, corner = -1, hits = -1, first = -1.
__global__ __launch_bounds__(64) void k_road_episode_egos(int n_ego, int S, const double *__restrict__ step_margin, const int *__restrict__ step_corner,
                                                          double *__restrict__ ego_min, int *__restrict__ ego_step, int *__restrict__ ego_corner,
                                                          int *__restrict__ ego_hits, int *__restrict__ ego_first) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n_ego) return;
  const size_t row = (size_t)g * (size_t)S;
  double mn = INFINITY;
  int ms = -1, mc = -1, hits = 0, first = -1, bad = -1;
  for (int s = 0; s < S; ++s) {
    const double d = step_margin[row + s];
    if (d != d) { bad = s; break; }
    if (s == 0 || d < mn) { mn = d; ms = s; mc = step_corner[row + s]; }
    if (d < 0.0) {
      if (first < 0) first = s;
      ++hits;
    }
  }
  if (bad >= 0) { mn = NAN; ms = bad; mc = -1; hits = -1; first = -1; }
  ego_min[g] = mn; ego_step[g] = ms; ego_corner[g] = mc; ego_hits[g] = hits; ego_first[g] = first;
}
