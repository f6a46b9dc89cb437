// The tree-iLQR's feedback policy: the gains of one backward pass about given controls (k_ilqr_gains, solver.py:332-373) and closed-loop
// rollouts under given gains from perturbed start states (k_ilqr_policy, solver.py:202-253).  Both are stand-alone kernels built from the
// solver's own device functions (ilqr_kernels.hip) and the scoring kernel's sum (ilqr_score_kernels.hip); k_ilqr and its launch choice do not
// know of them.  Every output is the oracle's arithmetic (oracle/ilqr_ref.c: forward_rollout, gains, solve2, backward_rec, line_search),
// operation for operation -- tests/test_gpu_ilqr_policy.py pins them bit for bit.
//
// k_ilqr_gains<GEN>: one workgroup per cost tree, nothing shared between workgroups, no waiting on memory words; every loop is bounded by M
// or by the number of levels.  For tree t with controls T.us and regularisation mu[t]:
//  1. nominal rollout: xs[i] = f(xs[parent[i]], us[i] + 0.0), node 0 from x0 (the states k_ilqr_score produces); one thread, the only
//     serial part besides the level order.
//  2. derivatives: the M nodes dealt over the waves, il_stage_agents + il_node_derivs per node (l, l_x, l_xx, F_x at the POST state);
//     l_u = 2 (w u), l_uu = diag 2 w from the controls and the node weights, as il_backward_segment forms them.
//  3. backward sweep by tree levels, deepest first (T.level_start / level_nodes / child_start / child_list): one wave per node, one matrix
//     entry per lane.  A node's entry value function is 0 + V[c1] + V[c2] + ... over its children in key order; then per entry the six-term
//     sums with r ascending, addend + s, Q_ux = 0.0 + s, the LAPACK-order 2x2 solve with partial pivoting, the two-step value update and
//     the symmetrisation.  A workgroup barrier between levels.
//  4. dV[i] = (k0 Qu0 + k1 Qu1) + 0.5 ((k0 Q00 + k1 Q10) k0 + (k0 Q01 + k1 Q11) k1).
// Outputs per node: k [2], K [2,6], dV, V_x [6], V_xx [6,6] (the values AFTER the node's own update), the nominal xs, L; per tree J = numpy's
// pairwise L.sum() and bad_node.  The reference's root key -1 aliases numpy row -1, so its V_x / V_xx row M-1 additionally holds node 0's
// value (solver.py:344-350, oracle "Q2"); here row M-1 is that node's own value and nothing else.
// A singular Q_uu (the oracle's solve2 returns 1) neither faults nor raises: bad_node[t] = the lowest key among the nodes whose own Q_uu was
// singular while all their descendants were fine (-1: none), the tree's gains and values are zero-filled, its xs / L / J stay valid.
// One workgroup per tree is correct for any M; the call is meant for planner-size trees (tens to hundreds of nodes).  A 12 288-node stress
// tree is served, but slowly: its rollout runs on one thread and a level has eight waves.
//
// k_ilqr_policy<GEN>: the shape of k_ilqr_score -- one workgroup per (block of cb <= 64 candidates, cost tree), lane = candidate in the serial
// state recursion.  Candidate c carries a step size alpha[c] and a start offset dx0[c][6].  Per node, in line_search's order:
//   s_a = sum_j K[i][a][j] (x_new[p][j] - xs[p][j])  (j ascending from 0.0),  u_new = us + alpha k + s,  x_new = f(x_new[p], u_new);
// for node 0 the parent pair is (x0 + dx0, x0) -- the one extension over the reference, whose node 0 has no feedback term (dx0 = 0 adds +0.0).
// The nominal states xs are recomputed here from us (stage 0, one thread per workgroup, into the block's own rows of xnom), not taken from
// the caller.  Node costs exactly as k_ilqr_score prices them (L keeps mind_cost_eval's bits); J[c, t] is the LINE SEARCH's sum -- python's
// sum(), sequential from 0.0 in key order (solver.py:242-253) -- not numpy's pairwise sum.
// Included by mind_hip.hip behind ilqr_score_kernels.hip.
#pragma clang fp contract(off)

#define IL_PG_THREADS 512
#define IL_PG_WAVES (IL_PG_THREADS / 64)
// per-wave LDS scratch of the backward sweep (doubles); il_field uses the first 73 during the derivatives
#define IL_PG_FX 0        // F_x [6,6]
#define IL_PG_VXX 36      // children-summed V_xx [6,6]
#define IL_PG_VX 72       // children-summed V_x [6]
#define IL_PG_TM 78       // F_x^T V_xx [6,6]
#define IL_PG_R 114       // dt (V_xx[4 + a][j] + mu [j == 4 + a]) [2,6]
#define IL_PG_QUX 126     // [2,6]
#define IL_PG_QU 138      // [2]
#define IL_PG_QUU 140     // [2,2]
#define IL_PG_KK 144      // K [2,6]
#define IL_PG_K 156       // k [2]
#define IL_PG_VN 158      // V_xx before the symmetrisation [6,6]
#define IL_PG_SCR 194

// The nominal states of tree T from its nominal controls (the _forward_rollout recursion): xs[i] = f(xs[parent[i]], us[i] + 0.0), node 0 from
// x0, into px [M, 6].  ONE thread: it reads back only what it stored itself (a branch point reloads the parent's state).
__device__ __forceinline__ void il_pg_nominal(const IlqrConst &C, const IlqrTreeDev &T, double IL_AS1 *px) {
  double xp[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) xp[k] = C.x0[k];
  for (int i = 0; i < T.M; ++i) {
    const int p = T.parent[i];
    if (i > 0 && p != i - 1) {
#pragma unroll
      for (int k = 0; k < 6; ++k) xp[k] = px[(size_t)p * 6 + k];
    }
    const il_d2 uc = *(T.us + (size_t)i * 2).as<const il_d2>();
    const double u[2] = {uc.x + 0.0, uc.y + 0.0};
    double x[6];
    il_dyn_sc(C, xp, u, x);
#pragma unroll
    for (int k = 0; k < 6; ++k) { px[(size_t)i * 6 + k] = x[k]; xp[k] = x[k]; }
  }
}

// One node of the backward sweep, one wave (gains() of oracle/ilqr_ref.c).  Returns (wave-uniform) 0 fine, 1 a descendant was bad, 2 this
// node's Q_uu is singular.
template <bool GEN>
__device__ __forceinline__ int il_pg_node(const IlqrConst &C, const IlqrTreeDev &T, int c, size_t moff, double mu, double *scr, int IL_AS1 *flag,
                                          double IL_AS1 *k_out, double IL_AS1 *K_out, double IL_AS1 *dV_out, double IL_AS1 *Vx_out,
                                          double IL_AS1 *Vxx_out) {
  const int lane = threadIdx.x & 63;
  const int i = lane / 6, j = lane % 6;
  const double dt = C.dt;
  const int cs = __builtin_amdgcn_readfirstlane(T.child_start[c]), ce = __builtin_amdgcn_readfirstlane(T.child_start[c + 1]);
  int below = 0;
  for (int q = cs; q < ce; ++q) below |= flag[T.child_list[q]];
  if (__builtin_amdgcn_readfirstlane(below)) return 1;
  // ---- the entry value function (0 + V[c1] + V[c2] + ..., children in key order), F_x
  IL_WFENCE();
  if (lane < 36) {
    double v = 0.0;
    for (int q = cs; q < ce; ++q) v += Vxx_out[(moff + (size_t)T.child_list[q]) * 36 + lane];
    scr[IL_PG_VXX + lane] = v;
    scr[IL_PG_FX + lane] = T.Fx[(size_t)c * 36 + lane];
  } else if (lane < 42) {
    double v = 0.0;
    for (int q = cs; q < ce; ++q) v += Vx_out[(moff + (size_t)T.child_list[q]) * 6 + (lane - 36)];
    scr[IL_PG_VX + (lane - 36)] = v;
  }
  IL_WFENCE();
  // control weights and controls of the node: l_u = 2 (w u), l_uu = diag 2 w
  double w[2], u[2];
  {
    const il_d2 uu = *(T.us + (size_t)c * 2).template as<const il_d2>();
    u[0] = uu.x; u[1] = uu.y;
    if (GEN) { w[0] = T.node_w[(size_t)c * IL_NW + 24]; w[1] = T.node_w[(size_t)c * IL_NW + 25]; }
    else { const double pp = (double)T.prob[c]; w[0] = C.w_ctrl[0] * pp; w[1] = C.w_ctrl[1] * pp; }
  }
  // ---- stage A: T = F_x^T V_xx (36 lanes), Q_x (6), the regularised scaled rows R (12), Q_u (2)
  double qx = 0.0;
  if (lane < 36) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += scr[IL_PG_FX + r * 6 + i] * scr[IL_PG_VXX + r * 6 + j];
    scr[IL_PG_TM + lane] = s;
  } else if (lane < 42) {
    const int e = lane - 36;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += scr[IL_PG_FX + r * 6 + e] * scr[IL_PG_VX + r];
    qx = T.Lx[(size_t)c * 6 + e] + s;
  } else if (lane < 54) {
    const int a = (lane - 42) / 6, jj = (lane - 42) % 6;
    scr[IL_PG_R + a * 6 + jj] = dt * (scr[IL_PG_VXX + (4 + a) * 6 + jj] + (jj == 4 + a ? mu : 0.0));
  } else if (lane < 56) {
    const int a = lane - 54;
    const double lu = 2.0 * ((a ? w[1] : w[0]) * (a ? u[1] : u[0]));
    scr[IL_PG_QU + a] = lu + dt * scr[IL_PG_VX + 4 + a];
  }
  IL_WFENCE();
  // ---- stage B: Q_xx = l_xx + T F_x (36 lanes, kept), Q_ux = 0.0 + R F_x (12), Q_uu = l_uu + R[.][4 + b] dt (4)
  double qxx = 0.0;
  if (lane < 36) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += scr[IL_PG_TM + i * 6 + r] * scr[IL_PG_FX + r * 6 + j];
    qxx = T.Lxx[(size_t)c * 36 + lane] + s;
  } else if (lane < 48) {
    const int a = (lane - 36) / 6, jj = (lane - 36) % 6;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += scr[IL_PG_R + a * 6 + r] * scr[IL_PG_FX + r * 6 + jj];
    scr[IL_PG_QUX + a * 6 + jj] = 0.0 + s;
  } else if (lane < 52) {
    const int a = (lane - 48) / 2, b = (lane - 48) % 2;
    const double luu = a == b ? 2.0 * (a ? w[1] : w[0]) : 0.0;
    scr[IL_PG_QUU + a * 2 + b] = luu + scr[IL_PG_R + a * 6 + 4 + b] * dt;
  }
  IL_WFENCE();
  // ---- the 2x2 solves (solve2: LAPACK dgesv order, partial pivoting): every lane factorises Q_uu, lanes 0..5 own a column of Q_ux, lane 6 Q_u
  const double q00 = scr[IL_PG_QUU], q01 = scr[IL_PG_QUU + 1], q10 = scr[IL_PG_QUU + 2], q11 = scr[IL_PG_QUU + 3];
  const double qu0 = scr[IL_PG_QU], qu1 = scr[IL_PG_QU + 1];
  {
    double a00 = q00, a01 = q01, a10 = q10, a11 = q11;
    const int rho = lane < 6 ? lane : 0;
    double b0 = lane < 6 ? scr[IL_PG_QUX + rho] : qu0, b1 = lane < 6 ? scr[IL_PG_QUX + 6 + rho] : qu1;
    const bool swp = fabs(a10) > fabs(a00);
    if (swp) { double t = a00; a00 = a10; a10 = t; t = a01; a01 = a11; a11 = t; t = b0; b0 = b1; b1 = t; }
    const double l = a10 / a00;
    const double u11 = a11 - l * a01;
    if (__builtin_amdgcn_readfirstlane((int)((a00 == 0.0) || (u11 == 0.0)))) return 2;
    b1 = b1 - l * b0;
    const double x1 = b1 / u11;
    const double x0 = (b0 - a01 * x1) / a00;
    if (lane < 6) {
      scr[IL_PG_KK + lane] = -x0; scr[IL_PG_KK + 6 + lane] = -x1;
      K_out[(moff + (size_t)c) * 12 + lane] = -x0; K_out[(moff + (size_t)c) * 12 + 6 + lane] = -x1;
    } else if (lane == 6) {
      scr[IL_PG_K] = -x0; scr[IL_PG_K + 1] = -x1;
      k_out[(moff + (size_t)c) * 2] = -x0; k_out[(moff + (size_t)c) * 2 + 1] = -x1;
    }
  }
  IL_WFENCE();
  // ---- value update: V = Q + K^T Q_uu K, then += K^T Q_u. + Q_.u K; V_xx symmetrised
  const double k0 = scr[IL_PG_K], k1 = scr[IL_PG_K + 1];
  if (lane < 36) {
    const double Kj0 = scr[IL_PG_KK + j], Kj1 = scr[IL_PG_KK + 6 + j], Ki0 = scr[IL_PG_KK + i], Ki1 = scr[IL_PG_KK + 6 + i];
    const double Uj0 = scr[IL_PG_QUX + j], Uj1 = scr[IL_PG_QUX + 6 + j], Ui0 = scr[IL_PG_QUX + i], Ui1 = scr[IL_PG_QUX + 6 + i];
    const double QuuK0 = q00 * Kj0 + q01 * Kj1;
    const double QuuK1 = q10 * Kj0 + q11 * Kj1;
    double v = qxx + (Ki0 * QuuK0 + Ki1 * QuuK1);
    v += (Ki0 * Uj0 + Ki1 * Uj1) + (Ui0 * Kj0 + Ui1 * Kj1);
    scr[IL_PG_VN + lane] = v;
  } else if (lane < 42) {
    const int e = lane - 36;
    const double Ke0 = scr[IL_PG_KK + e], Ke1 = scr[IL_PG_KK + 6 + e], Ue0 = scr[IL_PG_QUX + e], Ue1 = scr[IL_PG_QUX + 6 + e];
    const double Quuk0 = q00 * k0 + q01 * k1;
    const double Quuk1 = q10 * k0 + q11 * k1;
    double v = qx + (Ke0 * Quuk0 + Ke1 * Quuk1);
    v += (Ke0 * qu0 + Ke1 * qu1) + (Ue0 * k0 + Ue1 * k1);
    Vx_out[(moff + (size_t)c) * 6 + e] = v;
  } else if (lane == 42) {
    dV_out[moff + (size_t)c] = (k0 * qu0 + k1 * qu1) + 0.5 * ((k0 * q00 + k1 * q10) * k0 + (k0 * q01 + k1 * q11) * k1);
  }
  IL_WFENCE();
  if (lane < 36) Vxx_out[(moff + (size_t)c) * 36 + lane] = 0.5 * (scr[IL_PG_VN + lane] + scr[IL_PG_VN + j * 6 + i]);
  IL_WFENCE();
  return 0;
}

template <bool GEN>
__global__ __launch_bounds__(IL_PG_THREADS) void k_ilqr_gains(const IlqrTreeDev *__restrict__ trees, IlqrConst C, int n_trees, int ag_doubles,
                                                              const double *__restrict__ mu_in, double *__restrict__ k_o, double *__restrict__ K_o,
                                                              double *__restrict__ dV_o, double *__restrict__ Vx_o, double *__restrict__ Vxx_o,
                                                              double *__restrict__ xs_o, double *__restrict__ L_o, double *__restrict__ J_o,
                                                              double *__restrict__ bad_o) {
  extern __shared__ double il_dsm[];
  __shared__ double fr_left[IL_SC_DEPTH];
  __shared__ int fr_lo[IL_SC_DEPTH], fr_n[IL_SC_DEPTH];
  __shared__ int sh_bad;
  const int t = blockIdx.x;
  if (t >= n_trees) return;
  const IlqrTreeDev T = trees[t];
  size_t moff = 0;                                  // the tree's first row among the call's nodes
  for (int k = 0; k < t; ++k) moff += (size_t)trees[k].M;
  const int M = T.M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double mu = mu_in[t];
  const GP<double> XS(xs_o), LL(L_o), KS(k_o), KK(K_o), DV(dV_o), VX(Vx_o), VXX(Vxx_o);
  double IL_AS1 *px = (XS + moff * 6).g();
  if (tid == 0) sh_bad = 0x7fffffff;

  // ---- 1. nominal rollout (the _forward_rollout recursion)
  if (tid == 0) il_pg_nominal(C, T, px);
  __threadfence_block();
  __syncthreads();

  // ---- 2. derivatives: a node per wave and turn
  double *scr = il_dsm + (size_t)wave * (IL_PG_SCR + ag_doubles), *ag = scr + IL_PG_SCR;
  for (int i = wave; i < M; i += IL_PG_WAVES) {
    if (C.use_exo) il_stage_agents(C, T, i, ag);
    double x[6], u[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = px[(size_t)i * 6 + k];
    const il_d2 uc = *(T.us + (size_t)i * 2).template as<const il_d2>();
    u[0] = uc.x; u[1] = uc.y;
    il_node_derivs<GEN>(C, T, i, x, u, scr, ag, (T.Lxx + (size_t)i * 36).p, (T.Fx + (size_t)i * 36).p, (T.Lx + (size_t)i * 6).p, L_o + moff + i);
  }
  __threadfence_block();
  __syncthreads();

  // ---- 3. backward sweep, deepest level first; T.rel[c] = 1 marks a node without a value function (singular itself or below)
  int IL_AS1 *flag = T.rel.g();
  for (int lv = T.n_levels - 1; lv >= 0; --lv) {
    const int l0 = T.level_start[lv], l1 = T.level_start[lv + 1];
    for (int q = l0 + wave; q < l1; q += IL_PG_WAVES) {
      const int c = __builtin_amdgcn_readfirstlane(T.level_nodes[q]);
      const int r = il_pg_node<GEN>(C, T, c, moff, mu, scr, flag, KS.g(), KK.g(), DV.g(), VX.g(), VXX.g());
      if (lane == 0) {
        flag[c] = r != 0;
        if (r == 2) atomicMin(&sh_bad, c);
      }
    }
    __threadfence_block();
    __syncthreads();
  }

  // ---- 4. a tree with a singular Q_uu reports the node and hands back zeros; J = L.sum() in numpy's order
  const int bad = sh_bad;
  if (bad != 0x7fffffff) {
    for (size_t e = tid; e < (size_t)M * 36; e += IL_PG_THREADS) {
      VXX[moff * 36 + e] = 0.0;
      if (e < (size_t)M * 12) KK[moff * 12 + e] = 0.0;
      if (e < (size_t)M * 6) VX[moff * 6 + e] = 0.0;
      if (e < (size_t)M * 2) KS[moff * 2 + e] = 0.0;
      if (e < (size_t)M) DV[moff + e] = 0.0;
    }
  }
  if (tid == 0) {
    bad_o[t] = bad != 0x7fffffff ? (double)bad : -1.0;      // (a double, so that one read-back brings every output)
    J_o[t] = il_sc_np_sum((LL + moff).g(), M, fr_left, fr_lo, fr_n, 1);
  }
}

// dynamic LDS of a gains launch whose trees hold at most `amax` agents
static inline size_t il_gains_lds_bytes(int amax) {
  return (size_t)IL_PG_WAVES * (IL_PG_SCR + (size_t)il_ag_doubles(amax)) * sizeof(double);
}

template <bool GEN>
__global__ __launch_bounds__(IL_SC_THREADS) void k_ilqr_policy(const IlqrTreeDev *__restrict__ trees, IlqrConst C, int n_trees, int n_cand, int cb,
                                                               long Mtot, int ag_doubles, const double *__restrict__ k_in,
                                                               const double *__restrict__ K_in, const double *__restrict__ alpha_in,
                                                               const double *__restrict__ dx0_in, double *__restrict__ xnom,
                                                               double *__restrict__ xs_out, double *__restrict__ us_out,
                                                               double *__restrict__ L_out, double *__restrict__ J_out) {
  extern __shared__ double il_dsm[];
  const int t = blockIdx.y;
  if (t >= n_trees) return;
  const IlqrTreeDev T = trees[t];
  size_t moff = 0;
  for (int k = 0; k < t; ++k) moff += (size_t)trees[k].M;
  const int M = T.M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * cb;
  if (c0 >= n_cand) return;
  const int nc = n_cand - c0 < cb ? n_cand - c0 : cb;
  const GP<const double> KS(k_in), KK(K_in);
  const GP<double> XS(xs_out), US(us_out), LL(L_out);
  // the block's own rows of the nominal states
  double IL_AS1 *pn = (GP<double>(xnom) + ((size_t)blockIdx.x * (size_t)Mtot + moff) * 6).g();

  // ---- 0. nominal states from the nominal controls, as k_ilqr_score's stage 1 (every candidate block repeats it into rows of its own:
  //         M dynamics steps on one thread, against sharing rows between workgroups)
  if (tid == 0) il_pg_nominal(C, T, pn);
  __threadfence_block();
  __syncthreads();

  // ---- 1. states under the policy (the _line_search recursion): lane = candidate
  if (wave == 0) {
    const bool act = lane < nc;
    const int cc = c0 + (act ? lane : 0);           // (idle lanes shadow the block's first candidate and store nothing)
    const size_t row = (size_t)cc * (size_t)Mtot + moff;
    double IL_AS1 *px = (XS + row * 6).g();
    double IL_AS1 *pu = (US + row * 2).g();
    const double al = alpha_in[cc];
    double xp[6], sp[6];                            // the parent's state under the policy / its nominal state
#pragma unroll
    for (int k = 0; k < 6; ++k) { sp[k] = C.x0[k]; xp[k] = C.x0[k] + dx0_in[(size_t)cc * 6 + k]; }
    for (int i = 0; i < M; ++i) {
      const int p = __builtin_amdgcn_readfirstlane(T.parent[i]);
      if (i > 0) {
        if (p != i - 1) {                           // a branch point: the parent's state was stored earlier by this very lane
#pragma unroll
          for (int k = 0; k < 6; ++k) xp[k] = px[(size_t)p * 6 + k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) sp[k] = pn[(size_t)p * 6 + k];
      }
      const il_d2 uc = *(T.us + (size_t)i * 2).template as<const il_d2>();
      const il_d2 kc = *(KS + (moff + (size_t)i) * 2).template as<const il_d2>();
      const auto Kr = (KK + (moff + (size_t)i) * 12).template as<const il_d2>();
      double Kn[12];
#pragma unroll
      for (int k = 0; k < 6; ++k) { const il_d2 v = Kr[k]; Kn[2 * k] = v.x; Kn[2 * k + 1] = v.y; }
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) { const double d = xp[k] - sp[k]; s0 += Kn[k] * d; s1 += Kn[6 + k] * d; }
      const double u[2] = {uc.x + al * kc.x + s0, uc.y + al * kc.y + s1};
      double x[6];
      il_dyn_sc(C, xp, u, x);
      if (act) {
        const auto xn = (il_d2 IL_AS1 *)(px + (size_t)i * 6);
        xn[0] = il_d2{x[0], x[1]}; xn[1] = il_d2{x[2], x[3]}; xn[2] = il_d2{x[4], x[5]};
        *(il_d2 IL_AS1 *)(pu + (size_t)i * 2) = il_d2{u[0], u[1]};
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) xp[k] = x[k];
    }
  }
  __threadfence_block();
  __syncthreads();

  // ---- 2. node costs, as k_ilqr_score's stage 2 at the new states and controls
  {
    double *scr = il_dsm + (size_t)wave * (IL_SC_SCR + ag_doubles), *ag = scr + IL_SC_SCR;
    for (int i = wave; i < M; i += IL_SC_WAVES) {
      if (C.use_exo) il_stage_agents(C, T, i, ag);
      const IlNodeW<GEN> NW{C, GEN ? (T.node_w + (size_t)i * IL_NW).p : nullptr, GEN ? 0.0 : (double)T.prob[i]};
      for (int k = 0; k < nc; ++k) {
        const size_t e = (size_t)(c0 + k) * (size_t)Mtot + moff + (size_t)i;
        double x[6], u[2];
        {
          const auto qx = (XS + e * 6).template as<const il_d2>();
          const il_d2 v0 = qx[0], v1 = qx[1], v2 = qx[2], vu = *(US + e * 2).template as<const il_d2>();
          x[0] = v0.x; x[1] = v0.y; x[2] = v1.x; x[3] = v1.y; x[4] = v2.x; x[5] = v2.y; u[0] = vu.x; u[1] = vu.y;
        }
        FieldOut fe;
        il_field<GEN>(C, T, i, x[0], x[1], scr, ag, false, fe);
        if (lane == 0) LL[e] = il_node_cost<GEN>(NW, x, u, fe);
      }
    }
  }
  __threadfence_block();
  __syncthreads();

  // ---- 3. J = python's sum(L): sequential from 0.0 in key order, a candidate per thread
  if (tid < nc) {
    const double IL_AS1 *Lr = (LL + ((size_t)(c0 + tid) * (size_t)Mtot + moff)).g();
    double J = 0.0;
    for (int i = 0; i < M; ++i) J += Lr[i];
    J_out[(size_t)(c0 + tid) * (size_t)n_trees + t] = J;
  }
}
