// Lane audit: whether a plan's trajectory trees and a closed-loop episode drove where they were told to drive -- the ego box's centre
// against the lane centrelines, computed from lane_geom.h.
//
// k_lane_boxes<FORM>: n boxes, each one state row (x, y, .., yaw) of `stride` doubles, against the lanes verts [V, 2] / lane_off [P + 1] /
// cum [V]: per box the lateral offset, arc length, heading cosine and sine, lane and edge of the nearest segment (row k = 0 of the outputs,
// [2, n] each) and of the nearest segment that goes the box's way (k = 1), and the margin bound - |lat of k = 1|.  A row holding a
// non-finite value reports NaN / -1.
//
// Shapes.  The vertices -- what every box shares -- are staged in LDS LG_TV at a time, thread i of a turn loading vertex v0 + i (+ a
// multiple of the block) as one 16-byte (x, y) pair, consecutive lanes consecutive addresses (k_road_boxes' staging).
//   FORM == 1: a workgroup = LG_BB consecutive boxes, thread = box.  Every thread walks the staged vertices in index order -- one LDS
//     address per step in every lane, a broadcast --, the previous vertex in registers, the lane's end tracked by a wave-uniform index
//     into lane_off.  Right for many candidate rows.
//   FORM == 2: a workgroup = ONE wavefront = one box.  A turn stages LG_TV + 1 vertices (the next turn's first once more), lane i takes
//     the staged segments i, i + 64, ..: its segments ascend.  The 64 lanes are then folded by __shfl_xor on the key (d2, g), once for
//     `any` and once for `flow` (k_audit_ttc<2>'s fold); lane 0 runs lg_finish and stores.  Right for the auditor's single trace against
//     a whole map, where FORM 1 keeps one workgroup busy.
// The minimum over (d2, g) is associative and commutative: no output depends on FORM, LG_TV, LG_BB or the grid.  No atomics.
// The per-tree / per-ego reductions are the clearance audit's (audit_kernels.hip: k_audit_plan_trees, k_audit_episode_egos<true>) over the
// margin with the with-flow lane as the tag; k_lane_progress adds the arc length covered.
// Included by mind_hip.hip behind ttc_kernels.hip.
#pragma clang fp contract(off)
#include "lane_geom.h"

#define LG_BB 256          // boxes per workgroup = threads (FORM 1)
#define LG_TV 256          // vertices staged at a time (4 KB of LDS)

template <int FORM>
__global__ __launch_bounds__(FORM == 1 ? LG_BB : 64) void k_lane_boxes(AuBox ego, double cos_flow, double bound, long n_boxes,
                                                                        const double *__restrict__ states, int stride, int iyaw,
                                                                        const double *__restrict__ verts, const int *__restrict__ lane_off, int P,
                                                                        int V, const double *__restrict__ cum, double *__restrict__ lat,
                                                                        double *__restrict__ arc, double *__restrict__ along,
                                                                        double *__restrict__ across, int *__restrict__ lane,
                                                                        int *__restrict__ edge, double *__restrict__ margin) {
  static_assert(FORM == 1 || FORM == 2, "thread per box, or one wavefront per box");
  constexpr int NTHR = FORM == 1 ? LG_BB : 64;
  __shared__ double2 tile[LG_TV + 1];
  const int tid = threadIdx.x;
  const long g = FORM == 1 ? (long)blockIdx.x * LG_BB + tid : (long)blockIdx.x;
  const bool act = g < n_boxes;
  const double *x = states + (size_t)(act ? g : 0) * (size_t)stride;      // (idle lanes shadow the first box and store nothing)
  bool ok = true;
  for (int q = 0; q < stride; ++q) ok = ok && au_finite(x[q]);
  const double px = ok ? x[0] : 0.0, py = ok ? x[1] : 0.0;
  double sn, cs;
  mind_sincos(ok ? x[iyaw] : 0.0, &sn, &cs);
  lg_walk w;
  lg_begin(&w);
  if constexpr (FORM == 1) {
    int l = 0, lbeg = 0, lend = lane_off[1];
    double Ax = 0.0, Ay = 0.0;
    for (int v0 = 0; v0 < V; v0 += LG_TV) {
      if (v0 > 0) __syncthreads();
      const int nv = V - v0 < LG_TV ? V - v0 : LG_TV;
      for (int i = tid; i < nv; i += NTHR) tile[i] = reinterpret_cast<const double2 *>(verts)[v0 + i];
      __syncthreads();
      for (int j = 0; j < nv; ++j) {
        const int gv = v0 + j;
        const double2 p = tile[j];
        double Bx, By;
        rg_rel(p.x, p.y, px, py, ego.off, cs, sn, &Bx, &By);
        if (gv != lbeg) lg_edge(&w, Ax, Ay, Bx, By, cs, sn, cos_flow, gv - 1);
        Ax = Bx; Ay = By;
        if (gv + 1 == lend) {
          ++l;
          lbeg = lend;
          lend = lane_off[l + 1];         // (lane_off holds P + 2 entries on the device: the last repeats V)
        }
      }
    }
  } else {
    for (int v0 = 0; v0 < V - 1; v0 += LG_TV) {
      if (v0 > 0) __syncthreads();
      const int nv = V - v0 < LG_TV + 1 ? V - v0 : LG_TV + 1;             // the staged vertices; its segments: nv - 1
      for (int i = tid; i < nv; i += NTHR) tile[i] = reinterpret_cast<const double2 *>(verts)[v0 + i];
      __syncthreads();
      for (int i = tid; i < nv - 1; i += NTHR) {
        const int gv = v0 + i;
        const int l = lg_lane_of(lane_off, P, gv);
        if (gv + 1 >= lane_off[l + 1]) continue;                          // (a lane's last vertex begins no segment)
        const double2 a = tile[i], b = tile[i + 1];
        double Ax, Ay, Bx, By;
        rg_rel(a.x, a.y, px, py, ego.off, cs, sn, &Ax, &Ay);
        rg_rel(b.x, b.y, px, py, ego.off, cs, sn, &Bx, &By);
        lg_edge(&w, Ax, Ay, Bx, By, cs, sn, cos_flow, gv);
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      lg_take(&w.any, __shfl_xor(w.any.d2, m), __shfl_xor(w.any.g, m));
      lg_take(&w.flow, __shfl_xor(w.flow.d2, m), __shfl_xor(w.flow.g, m));
    }
  }
  if (act && (FORM == 1 || tid == 0)) {
    lg_out o[2];
    double mg;
    if (ok) {
      lg_finish(&w.any, px, py, cs, sn, ego.off, verts, lane_off, P, cum, &o[0]);
      lg_finish(&w.flow, px, py, cs, sn, ego.off, verts, lane_off, P, cum, &o[1]);
      mg = lg_margin(bound, o[1].lat);
    } else {
      lg_out_nan(&o[0]);
      lg_out_nan(&o[1]);
      mg = NAN;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const size_t r = (size_t)k * (size_t)n_boxes + (size_t)g;
      lat[r] = o[k].lat; arc[r] = o[k].s; along[r] = o[k].along; across[r] = o[k].across; lane[r] = o[k].lane; edge[r] = o[k].edge;
    }
    margin[g] = mg;
  }
}

// the arc length covered, one thread per trace, sequential in step / key order from 0.0, over the `any` rows of k_lane_boxes' outputs.
//   PLAN == false, thread = ego over its S steps: for the steps k >= 1 with lane[k] == lane[k - 1] >= 0, d = s[k] - s[k - 1]:
//     progress += d, and back += d when d < 0.
//   PLAN == true, thread = (candidate, tree): for the nodes i with parent[i] >= 0 and the same lane (>= 0) as the parent,
//     progress += (double)prob[i] (s[i] - s[parent[i]]); `back` is not written.
template <bool PLAN>
__global__ __launch_bounds__(64) void k_lane_progress(int n_outer, int S, int n_trees, const AuTree *__restrict__ trees, const int *__restrict__ parent,
                                                      const float *__restrict__ prob, const int *__restrict__ lane_any, const double *__restrict__ s_any,
                                                      double *__restrict__ progress, double *__restrict__ back) {
  const long e = (long)blockIdx.x * 64 + threadIdx.x;
  if constexpr (PLAN) {
    if (e >= (long)n_outer * n_trees) return;
    const int c = (int)(e / n_trees), t = (int)(e % n_trees);
    const AuTree T = trees[t];
    const size_t row = (size_t)c * (size_t)S + (size_t)T.moff;           // (S: the call's nodes, sum M)
    double acc = 0.0;
    for (int i = 0; i < T.M; ++i) {
      const int p = parent[T.moff + i];
      if (p < 0) continue;
      const int li = lane_any[row + i];
      if (li < 0 || li != lane_any[row + p]) continue;
      acc = acc + (double)prob[T.moff + i] * (s_any[row + i] - s_any[row + p]);
    }
    progress[e] = acc;
  } else {
    if (e >= n_outer) return;
    const size_t row = (size_t)e * (size_t)S;
    double acc = 0.0, bk = 0.0;
    for (int k = 1; k < S; ++k) {
      const int lk = lane_any[row + k];
      if (lk < 0 || lk != lane_any[row + k - 1]) continue;
      const double d = s_any[row + k] - s_any[row + k - 1];
      acc = acc + d;
      if (d < 0.0) bk = bk + d;
    }
    progress[e] = acc; back[e] = bk;
  }
}
