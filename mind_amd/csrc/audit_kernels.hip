// Clearance audit: what a plan's trajectory trees and a closed-loop episode did to the other road users, computed from box_geom.h.
//
// k_audit_plan / k_audit_plan_trees: n_cand candidate state sets on the cost trees of a plan.  For (candidate, trajectory node i of tree t)
//   clear[i] = min over exo agents j = 1..a_t-1 of bg_point_rect(mean[i,j] - centre(xs[i]), yaw = xs[i][3], ego box) - ((double)cov[i,j] + exo_margin),
// the lowest j winning ties: the pairing of xs[i] with agent_mean[i] is the solver's own (trajectory_tree.py:78-118), the disc is the one
// the exo term prices (trajectory_tree.py:95-102).  a_t == 1: +inf / -1; a node whose state is not finite: NaN / -1.
// k_audit_episode / k_audit_episode_egos: n_ego ego traces (x, y, v, yaw) against one replayed scene (the layouts of mind_loop_desc.exo_obs /
// exo_valid, row 0 unused): per (ego, step) the minimum bg_rect_rect over the valid tracks 1..n-1, the lowest track winning ties; no valid
// track: +inf / -1.
//
// Shapes.  k_audit_plan: a workgroup = (AU_NB consecutive nodes of the call, AU_CB candidates); thread = candidate.  The nodes' discs -- what
// every candidate shares -- are staged in LDS once per workgroup, AU_CH agents at a time; a tree of more agents takes further turns, its
// running minimum kept in the output arrays.  k_audit_episode: a workgroup = (one step, 64 egos); thread = ego; the step's valid tracks
// (centre, cos, sin, box) are staged in LDS, AU_TCH at a time.  The per-tree / per-ego reductions are one thread each, sequential in key /
// step order: deterministic, and hit_mass is the sequential sum from 0.0 mind_ilqr_policy_rollouts defines for its J.
// Included by mind_hip.hip behind ilqr_policy_kernels.hip.
#pragma clang fp contract(off)
#include "box_geom.h"

#define AU_CB 256          // candidates per workgroup (k_audit_plan)
#define AU_NB 8            // nodes per workgroup
#define AU_CH 16           // agents of a node staged at a time
#define AU_EB 64           // egos per workgroup (k_audit_episode)
#define AU_TCH 64          // tracks of a step staged at a time

struct AuBox { double L, W, off; };                 // mind_audit_box
struct AuNode { int ag_off, a; };                   // a node's first agent row among the call's (node, agent) rows; its tree's agent count
struct AuTree { int moff, M; };                     // a tree's first node among the call's nodes; its node count

__device__ __forceinline__ bool au_finite(double v) { return fabs(v) <= 0x1.fffffffffffffp+1023; }      // false for NaN and +-inf

__global__ __launch_bounds__(AU_CB) void k_audit_plan(AuBox ego, double exo_margin, int Mtot, int n_cand, const AuNode *__restrict__ nodes,
                                                      const float *__restrict__ mean, const float *__restrict__ cov,
                                                      const double *__restrict__ xs, double *__restrict__ node_clear, int *__restrict__ node_agent) {
  __shared__ double dsc[AU_NB][AU_CH][3];           // (x, y, radius) of the staged discs
  __shared__ AuNode nd[AU_NB];
  const int g0 = blockIdx.x * AU_NB;
  const int nn = Mtot - g0 < AU_NB ? Mtot - g0 : AU_NB;
  const int tid = threadIdx.x, c = blockIdx.y * AU_CB + tid;
  if (tid < nn) nd[tid] = nodes[g0 + tid];
  __syncthreads();
  int amax = 1;
  for (int k = 0; k < nn; ++k) amax = nd[k].a > amax ? nd[k].a : amax;
  // the first turn runs even without an exo agent: it writes +inf / -1 (or NaN / -1)
  for (int j0 = 1; j0 == 1 || j0 < amax; j0 += AU_CH) {
    if (j0 > 1) __syncthreads();
    for (int e = tid; e < nn * AU_CH; e += AU_CB) {
      const int k = e / AU_CH, j = j0 + e % AU_CH;
      if (j < nd[k].a) {
        const size_t r = (size_t)nd[k].ag_off + (size_t)j;
        dsc[k][e % AU_CH][0] = (double)mean[r * 2];
        dsc[k][e % AU_CH][1] = (double)mean[r * 2 + 1];
        dsc[k][e % AU_CH][2] = (double)cov[r] + exo_margin;
      }
    }
    __syncthreads();
    if (c < n_cand) {
      for (int k = 0; k < nn; ++k) {
        const size_t row = (size_t)c * (size_t)Mtot + (size_t)(g0 + k);
        const double *x = xs + row * 6;
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 6; ++q) ok = ok && au_finite(x[q]);
        double best = INFINITY;
        int bj = -1;
        if (!ok) {
          best = NAN;
        } else {
          if (j0 > 1) { best = node_clear[row]; bj = node_agent[row]; }
          double sn, cs;
          mind_sincos(x[3], &sn, &cs);
          const double px = x[0], py = x[1];
          const int ja = nd[k].a - j0 < AU_CH ? nd[k].a - j0 : AU_CH;
          for (int j = 0; j < ja; ++j) {
            const double dx = (dsc[k][j][0] - px) - ego.off * cs, dy = (dsc[k][j][1] - py) - ego.off * sn;
            const double d = bg_point_rect(dx, dy, cs, sn, ego.L, ego.W) - dsc[k][j][2];
            if (d < best) { best = d; bj = j0 + j; }
          }
        }
        if (j0 == 1 || ok) { node_clear[row] = best; node_agent[row] = bj; }
      }
    }
  }
}

// per (candidate, tree), for both audits -- mind_audit_plan folds (node_clear, node_agent), mind_audit_road_plan (node_margin, node_corner):
// the minimum value with its node and that node's tag (the lowest key wins ties), the nodes below zero (hits), the first of them and
// their probability mass.  A tree holding a NaN node reports min = NaN, node = the lowest such key, tag = -1, hits = -1, first = -1,
// mass = NaN.
__global__ __launch_bounds__(256) void k_audit_plan_trees(int Mtot, int n_cand, int n_trees, const AuTree *__restrict__ trees,
                                                          const float *__restrict__ prob, const double *__restrict__ node_val,
                                                          const int *__restrict__ node_tag, double *__restrict__ tree_min,
                                                          int *__restrict__ tree_node, int *__restrict__ tree_tag, int *__restrict__ tree_hits,
                                                          int *__restrict__ tree_first, double *__restrict__ tree_mass) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)n_cand * n_trees) return;
  const int c = (int)(e / n_trees), t = (int)(e % n_trees);
  const AuTree T = trees[t];
  const size_t row = (size_t)c * (size_t)Mtot + (size_t)T.moff;
  double mn = INFINITY, mass = 0.0;
  int mi = -1, mt = -1, hits = 0, first = -1, bad = -1;
  for (int i = 0; i < T.M; ++i) {
    const double d = node_val[row + i];
    if (d != d) { bad = i; break; }
    if (i == 0 || d < mn) { mn = d; mi = i; mt = node_tag[row + i]; }
    if (d < 0.0) {
      if (first < 0) first = i;
      ++hits;
      mass += (double)prob[T.moff + i];
    }
  }
  if (bad >= 0) { mn = NAN; mi = bad; mt = -1; hits = -1; first = -1; mass = NAN; }
  tree_min[e] = mn; tree_node[e] = mi; tree_tag[e] = mt; tree_hits[e] = hits; tree_first[e] = first; tree_mass[e] = mass;
}

__global__ __launch_bounds__(AU_EB) void k_audit_episode(AuBox ego, int n_ego, int S, int n, const double *__restrict__ ego_states,
                                                         const double *__restrict__ exo, const unsigned char *__restrict__ valid,
                                                         const double *__restrict__ boxes, double *__restrict__ step_clear,
                                                         int *__restrict__ step_track) {
  __shared__ double trk[AU_TCH][6];                 // (x, y, cos, sin, L, W) of the staged tracks
  __shared__ int trk_ok[AU_TCH];
  const int s = blockIdx.x, tid = threadIdx.x, g = blockIdx.y * AU_EB + tid;
  const bool act = g < n_ego;
  const size_t row = (size_t)(act ? g : 0) * (size_t)S + (size_t)s;      // (idle lanes shadow the first ego and store nothing)
  const double px = ego_states[row * 4], py = ego_states[row * 4 + 1];
  double sn, cs;
  mind_sincos(ego_states[row * 4 + 3], &sn, &cs);
  double best = INFINITY;
  int bj = -1;
  for (int j0 = 1; j0 < n; j0 += AU_TCH) {
    if (j0 > 1) __syncthreads();
    {
      const int j = j0 + tid;
      const bool v = j < n && valid[(size_t)s * n + j] != 0;
      const double *r = exo + ((size_t)s * n + (v ? j : 0)) * 5;
      double ts, tc;
      mind_sincos(v ? r[2] : 0.0, &ts, &tc);
      trk_ok[tid] = v;
      if (v) {
        trk[tid][0] = r[0]; trk[tid][1] = r[1]; trk[tid][2] = tc; trk[tid][3] = ts;
        trk[tid][4] = boxes[(size_t)j * 2]; trk[tid][5] = boxes[(size_t)j * 2 + 1];
      }
    }
    __syncthreads();
    const int nj = n - j0 < AU_TCH ? n - j0 : AU_TCH;
    for (int j = 0; j < nj; ++j) {
      if (!trk_ok[j]) continue;
      const double dx = (trk[j][0] - px) - ego.off * cs, dy = (trk[j][1] - py) - ego.off * sn;
      const double d = bg_rect_rect(dx, dy, cs, sn, ego.L, ego.W, trk[j][2], trk[j][3], trk[j][4], trk[j][5]);
      if (d < best) { best = d; bj = j0 + j; }
    }
  }
  if (act) { step_clear[row] = best; step_track[row] = bj; }
}

// per ego, for both audits -- mind_audit_episode folds (step_clear, step_track), mind_audit_road_episode (step_margin, step_corner): the
// minimum value over the steps with its step and that step's tag (the lowest step wins ties), the steps below the bar (hits; both audits
// hand 0.0, mind_audit_ttc its `bound` over (step_ttc, step_track)) and the first of them.  NAN_STEP (the road audit, whose boxes report NaN for a non-finite state row): a trace holding a NaN step reports min = NaN,
// step = the first such step, tag = -1, hits = -1, first = -1.  Without it (the clearance audit, whose host entry admits finite inputs
// only) a NaN is compared like any value: at step 0 it stays the minimum, at a later step it is passed over.
template <bool NAN_STEP>
__global__ __launch_bounds__(64) void k_audit_episode_egos(int n_ego, int S, double bar, const double *__restrict__ step_val, const int *__restrict__ step_tag,
                                                           double *__restrict__ ego_min, int *__restrict__ ego_step, int *__restrict__ ego_tag,
                                                           int *__restrict__ ego_hits, int *__restrict__ ego_first) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n_ego) return;
  const size_t row = (size_t)g * (size_t)S;
  double mn = INFINITY;
  int ms = -1, mt = -1, hits = 0, first = -1, bad = -1;
  for (int s = 0; s < S; ++s) {
    const double d = step_val[row + s];
    if constexpr (NAN_STEP)
      if (d != d) { bad = s; break; }
    if (s == 0 || d < mn) { mn = d; ms = s; mt = step_tag[row + s]; }
    if (d < bar) {
      if (first < 0) first = s;
      ++hits;
    }
  }
  if constexpr (NAN_STEP)
    if (bad >= 0) { mn = NAN; ms = bad; mt = -1; hits = -1; first = -1; }
  ego_min[g] = mn; ego_step[g] = ms; ego_tag[g] = mt; ego_hits[g] = hits; ego_first[g] = first;
}
