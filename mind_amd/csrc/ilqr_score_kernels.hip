// Scoring of candidate control trees: rollout + TreeCost of n_cand control trees per cost tree, no optimisation (solver.py:255-330 without
// the derivatives).  For candidate c and node i: xs[c][i] = f(xs[c][parent[i]], us[c][i]) (node 0 hangs off x0), L[c][i] = TreeCost.l at
// that state and control, J[c] = numpy's pairwise L[c].sum() -- the J_opt a fit of one iteration from us[c] reports.
//
// Built from the solver's own device functions (ilqr_kernels.hip): il_dyn_sc for the states, il_stage_agents + il_field + il_node_cost for the
// node costs (the wave-cooperative form k_cost_eval runs, so L equals mind_cost_eval's bits), and the recursion of il_np_sum for the sums.
//
// One workgroup per (block of `cb` <= 64 candidates, cost tree); nothing is shared between workgroups.
//  1. states: wave 0, lane = candidate, the node index walks the keys 0..M-1 (parent[i] < i; wave-uniform).  Only this part is serial.  A
//     node whose parent is the node before it continues from registers, a branch point reloads the parent's state from xs.
//  2. node costs: the M nodes are dealt over the waves; a wave stages a node's agents once and prices the node for every candidate of the
//     block, one il_field per (node, candidate).
//  3. sums: thread c < candidates of the block adds its row of L in numpy's order.
// All arrays are indexed (candidate, node) -> (size_t)c * Mtot + node offset of the tree + i.
// Included by mind_hip.hip behind ilqr_kernels.hip.
#pragma clang fp contract(off)

#define IL_SC_THREADS 512
#define IL_SC_WAVES (IL_SC_THREADS / 64)
#define IL_SC_CB 64        // candidates per workgroup at most: one lane each in the state recursion
#define IL_SC_SCR 80       // doubles of per-wave LDS scratch: il_field's 9 window cells behind 64 spare ones
#define IL_SC_DEPTH 16     // frames of the pairwise sum's recursion: a row of n doubles holds at most log2(n / 128) + 1 at a time (14 for the 2^20 the host admits)

// one leaf of numpy's add.reduce (n <= 128): il_np_sum's first two branches
__device__ __forceinline__ double il_sc_leaf(const double IL_AS1 *a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
  int i;
#pragma unroll
  for (i = 0; i < 8; ++i) r[i] = a[i];
  for (i = 8; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// il_np_sum(a, n) without the call stack: the same splits (n2 = n / 2 rounded down to a multiple of 8), the same leaves, left + right at
// every level.  A frame holds the right half still to be summed and, once known, the left half's sum; frames live in LDS, `nthr` apart.
__device__ __forceinline__ double il_sc_np_sum(const double IL_AS1 *a, int n, double *fr_left, int *fr_lo, int *fr_n, int nthr) {
  int sp = 0, lo = 0;
  for (;;) {
    while (n > 128 && sp < IL_SC_DEPTH) {           // (the depth bound cannot be reached: see IL_SC_DEPTH)
      int n2 = n / 2;
      n2 -= n2 % 8;
      fr_lo[sp * nthr] = lo + n2; fr_n[sp * nthr] = -(n - n2);      // negative length: the left half's sum is not there yet
      ++sp;
      n = n2;
    }
    double v = il_sc_leaf(a + lo, n);
    bool right = false;
    while (sp > 0) {
      const int fn = fr_n[(sp - 1) * nthr];
      if (fn < 0) {                                 // v is the left half: keep it, sum the right half next
        fr_left[(sp - 1) * nthr] = v; fr_n[(sp - 1) * nthr] = -fn;
        lo = fr_lo[(sp - 1) * nthr]; n = -fn;
        right = true;
        break;
      }
      v = fr_left[(sp - 1) * nthr] + v;             // v is the right half
      --sp;
    }
    if (!right) return v;
  }
}

template <bool GEN>
__global__ __launch_bounds__(IL_SC_THREADS) void k_ilqr_score(const IlqrTreeDev *__restrict__ trees, IlqrConst C, int n_trees, int n_cand, int cb,
                                                              long Mtot, int ag_doubles, const double *__restrict__ us_cand,
                                                              double *__restrict__ xs_out, double *__restrict__ L_out, double *__restrict__ J_out) {
  extern __shared__ double il_dsm[];
  __shared__ double fr_left[IL_SC_DEPTH * IL_SC_CB];
  __shared__ int fr_lo[IL_SC_DEPTH * IL_SC_CB], fr_n[IL_SC_DEPTH * IL_SC_CB];
  const int t = blockIdx.y;
  if (t >= n_trees) return;
  const IlqrTreeDev T = trees[t];
  size_t moff = 0;                                  // the tree's first row among the call's nodes
  for (int k = 0; k < t; ++k) moff += (size_t)trees[k].M;
  const int M = T.M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * cb;
  if (c0 >= n_cand) return;
  const int nc = n_cand - c0 < cb ? n_cand - c0 : cb;
  const GP<const double> US(us_cand);
  const GP<double> XS(xs_out), LL(L_out);

  // ---- 1. states (the _forward_rollout recursion): lane = candidate
  if (wave == 0) {
    const bool act = lane < nc;
    const size_t row = (size_t)(c0 + (act ? lane : 0)) * (size_t)Mtot + moff;      // (idle lanes shadow the block's first candidate and store nothing)
    const auto pu = (US + row * 2).as<const il_d2>();
    double IL_AS1 *px = (XS + row * 6).g();
    double xp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) xp[k] = C.x0[k];
    il_d2 un = pu[0];
    for (int i = 0; i < M; ++i) {
      const il_d2 uc = un;
      if (i + 1 < M) un = pu[i + 1];
      const int p = __builtin_amdgcn_readfirstlane(T.parent[i]);
      if (i > 0 && p != i - 1) {                    // a branch point: the parent's state was stored earlier by this very lane
#pragma unroll
        for (int k = 0; k < 6; ++k) xp[k] = px[(size_t)p * 6 + k];
      }
      // the control as the solver's nominal rollout forms it (us + alpha k, alpha = 0, k = 0)
      const double u[2] = {uc.x + 0.0, uc.y + 0.0};
      double x[6];
      il_dyn_sc(C, xp, u, x);
      if (act) {
        const auto xn = (il_d2 IL_AS1 *)(px + (size_t)i * 6);
        xn[0] = il_d2{x[0], x[1]}; xn[1] = il_d2{x[2], x[3]}; xn[2] = il_d2{x[4], x[5]};
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) xp[k] = x[k];
    }
  }
  __threadfence_block();
  __syncthreads();

  // ---- 2. node costs: a node per wave and turn, every candidate of the block at it
  {
    double *scr = il_dsm + (size_t)wave * (IL_SC_SCR + ag_doubles), *ag = scr + IL_SC_SCR;
    for (int i = wave; i < M; i += IL_SC_WAVES) {
      if (C.use_exo) il_stage_agents(C, T, i, ag);
      const IlNodeW<GEN> NW{C, GEN ? (T.node_w + (size_t)i * IL_NW).p : nullptr, GEN ? 0.0 : (double)T.prob[i]};
      for (int k = 0; k < nc; ++k) {
        const size_t e = (size_t)(c0 + k) * (size_t)Mtot + moff + (size_t)i;
        double x[6], u[2];
        {
          const auto qx = (XS + e * 6).as<const il_d2>();
          const il_d2 v0 = qx[0], v1 = qx[1], v2 = qx[2], vu = *(US + e * 2).as<const il_d2>();
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

  // ---- 3. J = L.sum() in numpy's order, a candidate per thread
  if (tid < nc) {
    const size_t e = (size_t)(c0 + tid) * (size_t)Mtot + moff;
    J_out[(size_t)(c0 + tid) * (size_t)n_trees + t] = il_sc_np_sum((LL + e).g(), M, fr_left + tid, fr_lo + tid, fr_n + tid, IL_SC_CB);
  }
}

// dynamic LDS of a launch whose trees hold at most `amax` agents
static inline size_t il_score_lds_bytes(int amax) {
  return (size_t)IL_SC_WAVES * (IL_SC_SCR + (size_t)il_ag_doubles(amax)) * sizeof(double);
}
