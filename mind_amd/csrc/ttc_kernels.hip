// Time-to-collision audit: how close to a collision a closed-loop episode drove, computed from ttc_geom.h.
//
// k_audit_ttc<LANES>: n_ego ego traces (x, y, v, yaw) against one replayed scene (the inputs of k_audit_episode: audit_kernels.hip).  Both the
// ego box and every track's box are swept at the constant velocity they have at the step -- the ego's v (cos yaw, sin yaw), the track's
// (vx, vy) -- and per (ego, step)
//   ttc[s] = min over the valid tracks j = 1..n-1 of tg_rect_rect_ttc(centre_j - centre_ego, velocity_j - velocity_ego, ...),
// the lowest track winning ties; a minimum above the horizon, +inf included: +inf / -1.
//
// Shapes.  A workgroup is one wavefront; a step's valid tracks (centre, cos, sin, box, velocity) are staged in LDS, AU_TCH at a time, lane i
// of a turn staging track j0 + i.
//   LANES == 1: a workgroup = (one step, 64 egos); thread = ego, walking the staged tracks in index order.  k_audit_episode's shape: right
//     for many candidate traces, one active lane of 64 for the auditor's single trace.
//   LANES == 2: a workgroup = (one step, ONE ego); lane i of a turn takes the staged track i, keeps its own (ttc, track) over the turns
//     -- its tracks ascend, so a strict < keeps the lowest -- and the 64 lanes are then folded by __shfl_xor on the lexicographic order
//     (ttc, track).  That minimum is associative and commutative: the result is the sequential scan's, bit for bit, whatever the order.
// The per-ego fold is k_audit_episode_egos<false> with the bar `bound` (audit_kernels.hip).
// Included by mind_hip.hip behind road_kernels.hip.
#pragma clang fp contract(off)
#include "ttc_geom.h"

template <int LANES>
__global__ __launch_bounds__(AU_EB) void k_audit_ttc(AuBox ego, double horizon, int n_ego, int S, int n, const double *__restrict__ ego_states,
                                                     const double *__restrict__ exo, const unsigned char *__restrict__ valid,
                                                     const double *__restrict__ boxes, double *__restrict__ step_ttc, int *__restrict__ step_track) {
  static_assert(LANES == 1 || LANES == 2, "thread per ego, or lanes over tracks");
  static_assert(AU_EB == 64 && AU_TCH == 64, "one wavefront per workgroup, one staged track per lane");
  __shared__ double trk[AU_TCH][8];                 // (x, y, cos, sin, L, W, vx, vy) of the staged tracks
  __shared__ int trk_ok[AU_TCH];
  // blockIdx.x = step + S * (LANES == 1: block of 64 egos; LANES == 2: ego)
  const int s = (int)(blockIdx.x % (unsigned)S), eb = (int)(blockIdx.x / (unsigned)S), tid = threadIdx.x;
  const int g = LANES == 1 ? eb * AU_EB + tid : eb;
  const bool act = g < n_ego;
  const size_t row = (size_t)(act ? g : 0) * (size_t)S + (size_t)s;      // (idle lanes shadow the first ego and store nothing)
  const double px = ego_states[row * 4], py = ego_states[row * 4 + 1], pv = ego_states[row * 4 + 2];
  double sn, cs;
  mind_sincos(ego_states[row * 4 + 3], &sn, &cs);
  const double evx = pv * cs, evy = pv * sn;
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
        trk[tid][6] = r[3]; trk[tid][7] = r[4];
      }
    }
    __syncthreads();
    const int nj = n - j0 < AU_TCH ? n - j0 : AU_TCH;
    const auto take = [&](int j) {
      if (!trk_ok[j]) return;
      const double dx = (trk[j][0] - px) - ego.off * cs, dy = (trk[j][1] - py) - ego.off * sn;
      const double t = tg_rect_rect_ttc(dx, dy, trk[j][6] - evx, trk[j][7] - evy, cs, sn, ego.L, ego.W, trk[j][2], trk[j][3], trk[j][4], trk[j][5]);
      if (t < best) { best = t; bj = j0 + j; }
    };
    if constexpr (LANES == 1) {
      for (int j = 0; j < nj; ++j) take(j);
    } else {
      if (tid < nj) take(tid);
    }
  }
  if constexpr (LANES == 2) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ot = __shfl_xor(best, m);
      const int oj = __shfl_xor(bj, m);
      if (ot < best || (ot == best && oj < bj)) { best = ot; bj = oj; }
    }
  }
  if (best > horizon) { best = INFINITY; bj = -1; }
  if (act && (LANES == 1 || tid == 0)) { step_ttc[row] = best; step_track[row] = bj; }
}
