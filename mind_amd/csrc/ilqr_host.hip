// Host side of the tree-iLQR exports (mind_ilqr_solve_trees / _solve_fields / _contingency* / mind_cost_eval) and of the native loop's
// speculative solve: one call = check, choose, build tables, lay out, stage, upload, launch, finish (il_solve).  What can be decided without a
// device -- knobs, launch form, index tables, arena layout -- lives in ilqr_choice.h.  Included by mind_hip.hip behind the context.
// grid coordinates exactly as numpy builds them (ilqr/utils.py:7-13): linspace(0, size, n) + offset
static void il_make_grid(int W, int H, double res, const double *ego_xy, double *gx, double *gy, double &offx, double &offy) {
  const double fsx = (double)(W - 1) * res, fsy = (double)(H - 1) * res;
  offx = ego_xy[0] - 0.5 * fsx; offy = ego_xy[1] - 0.5 * fsy;
  const double sx = fsx / (double)(W - 1), sy = fsy / (double)(H - 1);
  for (int i = 0; i < W; ++i) gx[i] = (double)i * sx + 0.0;
  gx[W - 1] = fsx;
  for (int i = 0; i < H; ++i) gy[i] = (double)i * sy + 0.0;
  gy[H - 1] = fsy;
  for (int i = 0; i < W; ++i) gx[i] += offx;
  for (int i = 0; i < H; ++i) gy[i] += offy;
}

// gen_dist_field (ilqr/utils.py:5-22): distance of every grid centroid to the polyline
extern "C" int mind_lane_dist_field(mind_ctx *c, const double *ego_xy, const double *lane, int n_pts, int W, int H,
                                    double res, double *offset, double *gx, double *gy, double *dist) {
  if (!c || !ego_xy || !lane || n_pts < 2 || W < 2 || H < 2 || !(res > 0) || !offset || !gx || !gy || !dist)
    return fail(c, MIND_EINVAL, "mind_lane_dist_field: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  il_make_grid(W, H, res, ego_xy, gx, gy, offset[0], offset[1]);
  const size_t nd = (size_t)W + H + 2 * (size_t)n_pts + (size_t)W * H;
  int rc;
  if ((rc = ensure(c, c->ilqr_dev, nd * sizeof(double)))) return rc;
  double *d = (double *)c->ilqr_dev.p;
  HIPCHK(c, hipMemcpyAsync(d, gx, W * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + W, gy, H * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d + W + H, lane, 2 * (size_t)n_pts * sizeof(double), hipMemcpyHostToDevice, st));
  double *out = d + W + H + 2 * (size_t)n_pts;
  hipLaunchKernelGGL(k_lane_field, dim3((W * H + 255) / 256), dim3(256), 0, st, d, d + W, W, H, d + W + H, n_pts, out, 0);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(dist, out, (size_t)W * H * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return MIND_OK;
}

namespace { int pl_pin(mind_ctx *c, int which, size_t bytes); }     // page-locked staging buffers of the context (aime_plan.hip)

// Upload of a few ten KB from the context's page-locked staging (hipHostMalloc: mapped into the device's address space) as a KERNEL on the
// consumer's own queue: the device reads the host buffer over PCIe (a few us) and the consumer follows back to back.  hipMemcpyAsync sends
// copies above its blit threshold to the SDMA engine, whose hand-over to the compute queue stood 10-15 us on either side of the copy in the
// plan's timeline (root scene: 60 KB, the solver's tables: 40 KB; profiles/r06az_timeline.txt).  16-byte words; large uploads stay copies.
typedef unsigned up_u4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_upload(const up_u4 *__restrict__ src, up_u4 *__restrict__ dst, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = __builtin_nontemporal_load(src + i);
}
static int pl_upload(mind_ctx *c, void *dst, const void *pinned_src, size_t bytes, hipStream_t s) {
  if (!bytes) return MIND_OK;
  if (c->ct.upload_kernel_max > 0 && bytes <= (size_t)c->ct.upload_kernel_max && bytes % 16 == 0 && (uintptr_t)dst % 16 == 0 && (uintptr_t)pinned_src % 16 == 0) {
    const size_t n16 = bytes / 16;
    hipLaunchKernelGGL(k_upload, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 256)), dim3(256), 0, s, (const up_u4 *)pinned_src, (up_u4 *)dst, n16);
    HIPCHK(c, hipGetLastError());
    return MIND_OK;
  }
  HIPCHK(c, hipMemcpyAsync(dst, pinned_src, bytes, hipMemcpyHostToDevice, s));
  return MIND_OK;
}

// the field of the NEXT tree-iLQR call on this context, ahead of it: grid + lane up, k_lane_field on `s`, an event behind it
static int il_field_prepare(mind_ctx *c, const mind_ilqr_cfg *cfg, const double *x0, const double *lane, int n_lane_pts, hipStream_t s) {
  c->il_field_valid = false;
  const int W = cfg->grid_w, H = cfg->grid_h;
  if (W < 3 || H < 3 || n_lane_pts < 2 || !(cfg->grid_res > 0)) return MIND_OK;        // (the call itself reports bad arguments)
  const size_t nin = (size_t)W + H + 2 * (size_t)n_lane_pts, nd = nin + (size_t)W * H;
  int rc;
  if ((rc = ensure(c, c->il_field, nd * sizeof(double)))) return rc;
  if (c->il_field_pin.cap < nin * sizeof(double)) {
    if (c->il_field_pin.alloc(2 * nin * sizeof(double)) != hipSuccess) return MIND_OK;
  }
  if (!c->ev_field) HIPCHK(c, c->ev_field.create(hipEventDisableTiming));
  double *h = c->il_field_pin.as<double>(), ox, oy;
  il_make_grid(W, H, cfg->grid_res, x0, h, h + W, ox, oy);
  memcpy(h + W + H, lane, 2 * (size_t)n_lane_pts * sizeof(double));
  double *d = (double *)c->il_field.p;
  HIPCHK(c, hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_lane_field, dim3((W * H + 255) / 256), dim3(256), 0, s, d, d + W, W, H, d + W + H, n_lane_pts, d + nin);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev_field, s));
  c->il_field_key[0] = x0[0]; c->il_field_key[1] = x0[1]; c->il_field_key[2] = W; c->il_field_key[3] = H; c->il_field_key[4] = cfg->grid_res;
  c->il_field_lane.assign(lane, lane + 2 * (size_t)n_lane_pts);
  c->il_field_valid = true;
  return MIND_OK;
}

// -------------------------------------------------------------------------------------------------
// one tree-iLQR call
// -------------------------------------------------------------------------------------------------
struct IlqrEvalReq { int nq; const int32_t *node; const double *x, *u; double *out; };
// rollout + node costs + their sum of n_cand candidate control trees per cost tree: us_cand [n_cand, sum M, 2] -> xs [n_cand, sum M, 6] (or null),
// L [n_cand, sum M] (or null), J [n_cand, n_trees]
struct IlqrScoreReq { int n_cand; const double *us_cand; double *xs, *L, *J; };
#define IL_SCORE_MAX_ROWS (1L << 20)      // n_cand x sum M a scoring call admits (48 MB of states)
// the gains of one backward pass about the controls us [sum M, 2] with regularisation mu [n_trees] (k_ilqr_gains): per-node k, K, dV, V_x, V_xx,
// the nominal xs and L, per-tree J and bad_node
struct IlqrGainsReq { const double *us, *mu; const mind_ilqr_gains_out *out; };
// closed-loop rollouts of n_cand (alpha [n_cand], dx0 [n_cand, 6] or null) under the gains k [sum M, 2], K [sum M, 12] about us (k_ilqr_policy):
// -> xs [n_cand, sum M, 6], us_out [n_cand, sum M, 2], L [n_cand, sum M] (each or null), J [n_cand, n_trees]
struct IlqrPolicyReq { int n_cand; const double *us, *k, *K, *alpha, *dx0; double *xs, *us_out, *L, *J; };

// What a caller asks of il_solve.  cfg2 != nullptr: two fits in one launch -- (cfg, lane term only) then, from its controls, (cfg2, full
// cost); grid != nullptr: the generic mode (materialised per-node fields + per-node weights); ev != nullptr: node costs at the requested
// points instead of a solve; sc != nullptr: candidate control trees priced instead of a solve (any number of trees); ga / po != nullptr: the
// gains about us_init / policy rollouts under given gains instead of a solve (any number of trees; us_init = the request's us)
struct IlqrCall {
  const mind_ilqr_cfg *cfg = nullptr, *cfg2 = nullptr;
  const mind_field_grid *grid = nullptr;
  const mind_cost_tree *trees = nullptr;
  int n_trees = 0;
  const double *x0 = nullptr, *lane = nullptr;
  int n_lane_pts = 0;
  double target_vel = 0.0;
  int use_exo = 0;
  const double *us_init = nullptr;
  double *xs = nullptr, *us = nullptr;
  mind_ilqr_stats *stats = nullptr, *stats2 = nullptr;      // of the first / the second fit
  const IlqrEvalReq *ev = nullptr;
  const IlqrScoreReq *sc = nullptr;
  const IlqrGainsReq *ga = nullptr;
  const IlqrPolicyReq *po = nullptr;
  bool begin_only = false;      // return behind the launch: the other half stays in c->il_finish (mind_ilqr_finish)
  bool dev_flat = false;        // the trees are the context's last plan's: read their agent arrays where k_aime_flat wrote them (tree t at node offset plan.book.tree_off[t])
};

// what the steps of one call share
struct IlRun {
  const IlqrCall &q;
  bool gen = false, dev_flat = false, field_ahead = false;
  int n_phases = 1, use_exo = 0, use_exo_first = 0, n_lane_pts = 0, W = 0, H = 0, trace_cap = 0, amax = 1;
  int pol_cb = 0;                       // candidates per workgroup of a policy-rollout call (il_score_block)
  long Mtot = 0;
  double grid_res = 0, fsx = 0, fsy = 0, offx = 0, offy = 0;
  std::vector<double> gx, gy;
  std::vector<int> n_agents;
  IlqrChoice ch;
  IlArena A;
  char *base = nullptr;                 // the device arena
  const char *up = nullptr;             // its uploaded part's image (page-locked)
  // where the results land on the host: xs of all trees and, right behind them, the stats of all trees (n_hx doubles); us; the abort word of
  // a wide launch; the trees' completion words
  double *hx = nullptr, *hus = nullptr;
  unsigned *h_abort = nullptr, *h_done = nullptr;
  size_t n_xs = 0, n_hx = 0, n_us = 0;
  std::vector<IlqrTreeDev> hT;
  IlqrConst K[2];                       // the constants of the two fits
  explicit IlRun(const IlqrCall &call) : q(call) {}
  double *Dp(size_t o) const { return o < A.nd_in ? (double *)base + o : (double *)(base + A.o_work) + (o - A.nd_in); }      // uploaded | produced doubles
  float *dF() const { return (float *)(base + A.bytesIn); }
  int *dI() const { return (int *)(base + A.bytesIn + A.bytesF); }
};

// MIND_PLAN_TRACE=1: host time stamps of a call's sections on stderr (as in mind_aime_plan)
struct IlStamp {
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char *what) const {
    static const bool on = getenv("MIND_PLAN_TRACE") != nullptr;
    if (on) fprintf(stderr, "[ilqr] %8.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what);
  }
};

// ---- 1. check: the arguments, before any device work; derives the call's mode
static int il_check(mind_ctx *c, const IlqrCall &q, IlRun &R) {
  const mind_ilqr_cfg *cfg = q.cfg, *cfg2 = q.cfg2;
  const IlqrEvalReq *ev = q.ev;
  if (!c || !cfg || !q.trees || q.n_trees <= 0 || !q.x0) return fail(c, MIND_EINVAL, "iLQR: bad argument");
  if (c->il_finish) return fail(c, MIND_ESTATE, "a tree-iLQR call begun with mind_ilqr_contingency_begin has not been finished (mind_ilqr_finish)");
  const IlqrScoreReq *sc = q.sc;
  const IlqrGainsReq *ga = q.ga;
  const IlqrPolicyReq *po = q.po;
  if (!ev && !sc && !ga && !po && (!q.xs || !q.us)) return fail(c, MIND_EINVAL, "iLQR: null output");
  if (ga && (!ga->us || !ga->mu || !ga->out || !ga->out->k || !ga->out->K || !ga->out->bad_node))
    return fail(c, MIND_EINVAL, "mind_ilqr_gains: null us / mu / out / out->k / out->K / out->bad_node");
  if (po && po->n_cand < 1) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: n_cand = %d, at least one candidate is needed", po->n_cand);
  if (po && (!po->us || !po->k || !po->K || !po->alpha || !po->J)) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: null us / k / K / alpha / J");
  if (sc && sc->n_cand < 1) return fail(c, MIND_EINVAL, "mind_ilqr_score_trees: n_cand = %d, at least one candidate is needed", sc->n_cand);
  if (sc && (!sc->us_cand || !sc->J)) return fail(c, MIND_EINVAL, "mind_ilqr_score_trees: null us_cand / J");
  const bool gen = R.gen = q.grid != nullptr;
  if (!gen && (!q.lane || q.n_lane_pts < 2)) return fail(c, MIND_EINVAL, "iLQR: target lane needs >= 2 points");
  R.n_phases = cfg2 ? 2 : 1;
  R.use_exo_first = cfg2 ? 0 : q.use_exo;
  R.use_exo = gen ? 0 : cfg2 ? 1 : q.use_exo;
  R.n_lane_pts = gen ? 0 : q.n_lane_pts;
  const int W = R.W = gen ? q.grid->W : cfg->grid_w, H = R.H = gen ? q.grid->H : cfg->grid_h;
  if (W < 3 || H < 3 || cfg->max_iter < 0) return fail(c, MIND_EINVAL, "bad grid / max_iter");
  if (gen && (!q.grid->gx || !q.grid->gy || !(q.grid->res > 0))) return fail(c, MIND_EINVAL, "bad field grid");
  if (cfg2 && (cfg2->dt != cfg->dt || cfg2->wheelbase != cfg->wheelbase || cfg2->grid_res != cfg->grid_res || cfg2->grid_w != cfg->grid_w ||
               cfg2->grid_h != cfg->grid_h))
    return fail(c, MIND_EINVAL, "mind_ilqr_contingency: both configurations must share dt / wheelbase / grid");
  R.dev_flat = q.dev_flat && !gen && !ev && !sc && c->plan.dev_fmean && c->plan.dev_fcov;
  R.n_agents.resize(q.n_trees);
  for (int t = 0; t < q.n_trees; ++t) {
    const mind_cost_tree &tr = q.trees[t];
    if (gen != (tr.field != nullptr) || gen != (tr.node_w != nullptr))
      return fail(c, MIND_EINVAL, "tree %d: field / node_w must be given exactly in the generic (grid) mode", t);
  }
  for (int t = 0; t < q.n_trees; ++t) {
    const mind_cost_tree &tr = q.trees[t];
    if (tr.n_nodes <= 0 || !tr.parent || (!gen && (!tr.prob || tr.n_agents <= 0)) || (R.use_exo && !R.dev_flat && (!tr.agent_mean || !tr.agent_cov)))
      return fail(c, MIND_EINVAL, "tree %d: bad arrays", t);
    if (tr.n_agents > IL_MAXA) return fail(c, MIND_EINVAL, "tree %d: %d agents > %d supported", t, tr.n_agents, IL_MAXA);
    R.n_agents[t] = gen ? 1 : tr.n_agents;
    R.amax = std::max(R.amax, R.n_agents[t]);
    R.Mtot += tr.n_nodes;
  }
  if (ev)
    for (int i = 0; i < ev->nq; ++i)
      if (ev->node[i] < 0 || ev->node[i] >= q.trees[0].n_nodes) return fail(c, MIND_EINVAL, "mind_cost_eval: node %d out of range", ev->node[i]);
  if (sc) {
    if (q.n_trees > 65535) return fail(c, MIND_EINVAL, "mind_ilqr_score_trees: %d cost trees > 65535 supported", q.n_trees);
    if ((long)sc->n_cand * R.Mtot > IL_SCORE_MAX_ROWS)
      return fail(c, MIND_EINVAL, "mind_ilqr_score_trees: %d candidates x %ld nodes > %ld rows supported", sc->n_cand, R.Mtot, IL_SCORE_MAX_ROWS);
    const size_t n = (size_t)sc->n_cand * (size_t)R.Mtot * 2;
    for (size_t i = 0; i < n; ++i)
      if (!std::isfinite(sc->us_cand[i]))
        return fail(c, MIND_EINVAL, "mind_ilqr_score_trees: candidate %ld has a non-finite control at node %ld", (long)(i / ((size_t)R.Mtot * 2)),
                    (long)(i / 2 % (size_t)R.Mtot));
  }
  // index of the first non-finite entry of a[0..n), -1 when there is none
  const auto first_bad = [](const double *a, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(a[i])) return (long)i; return -1L; };
  if (ga) {
    if (q.n_trees > 65535) return fail(c, MIND_EINVAL, "mind_ilqr_gains: %d cost trees > 65535 supported", q.n_trees);
    long b;
    if ((b = first_bad(ga->us, (size_t)R.Mtot * 2)) >= 0) return fail(c, MIND_EINVAL, "mind_ilqr_gains: non-finite control at node %ld", b / 2);
    if ((b = first_bad(ga->mu, (size_t)q.n_trees)) >= 0) return fail(c, MIND_EINVAL, "mind_ilqr_gains: non-finite mu of tree %ld", b);
    for (int t = 0; t < q.n_trees; ++t)
      if (ga->mu[t] < 0.0) return fail(c, MIND_EINVAL, "mind_ilqr_gains: negative mu of tree %d", t);
  }
  if (po) {
    if (q.n_trees > 65535) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: %d cost trees > 65535 supported", q.n_trees);
    if ((long)po->n_cand * R.Mtot > IL_SCORE_MAX_ROWS)
      return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: %d candidates x %ld nodes > %ld rows supported", po->n_cand, R.Mtot, IL_SCORE_MAX_ROWS);
    long b;
    if ((b = first_bad(po->us, (size_t)R.Mtot * 2)) >= 0) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: non-finite control at node %ld", b / 2);
    if ((b = first_bad(po->k, (size_t)R.Mtot * 2)) >= 0) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: non-finite k at node %ld", b / 2);
    if ((b = first_bad(po->K, (size_t)R.Mtot * 12)) >= 0) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: non-finite K at node %ld", b / 12);
    if ((b = first_bad(po->alpha, (size_t)po->n_cand)) >= 0) return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: non-finite alpha of candidate %ld", b);
    if (po->dx0 && (b = first_bad(po->dx0, (size_t)po->n_cand * 6)) >= 0)
      return fail(c, MIND_EINVAL, "mind_ilqr_policy_rollouts: non-finite dx0 of candidate %ld", b / 6);
  }
  R.trace_cap = std::min(256, std::max(cfg->max_iter, cfg2 ? cfg2->max_iter : 0));      // rows of the per-iteration trace, per phase
  return MIND_OK;
}

// grid coordinates exactly as numpy builds them (ilqr/utils.py:7-13)
static void il_grid(IlRun &R) {
  const IlqrCall &q = R.q;
  const bool gen = R.gen;
  const int W = R.W, H = R.H;
  R.grid_res = gen ? q.grid->res : q.cfg->grid_res;
  R.fsx = (double)(W - 1) * R.grid_res; R.fsy = (double)(H - 1) * R.grid_res;
  R.offx = gen ? q.grid->off_x : q.x0[0] - 0.5 * R.fsx; R.offy = gen ? q.grid->off_y : q.x0[1] - 0.5 * R.fsy;
  R.gx.resize(W); R.gy.resize(H);
  if (gen) {
    memcpy(R.gx.data(), q.grid->gx, W * sizeof(double));
    memcpy(R.gy.data(), q.grid->gy, H * sizeof(double));
  } else {
    double ox, oy;
    il_make_grid(W, H, R.grid_res, q.x0, R.gx.data(), R.gy.data(), ox, oy);
  }
}

// ---- 3. the index tables of every tree (kept in the context: their capacity survives the call)
static int il_build_tables(mind_ctx *c, const IlqrCall &q) {
  if ((int)c->il_tab.size() < q.n_trees) c->il_tab.resize(q.n_trees);
  for (int t = 0; t < q.n_trees; ++t) {
    const int bad = il_tree_tables(q.trees[t].parent, q.trees[t].n_nodes, c->it.ilqr_chunk, c->il_tab[t]);
    if (bad >= 0) return fail(c, MIND_EINVAL, "tree %d: node %d has parent %d", t, bad, q.trees[t].parent[bad]);
  }
  return MIND_OK;
}

// the constants of one fit: `cfg`'s weights and limits over the call's state, grid and lane field
static void il_fill_const(IlqrConst &K, const mind_ilqr_cfg *cfg, int use_exo, const IlRun &R, double *quad) {
  const int W = R.W, H = R.H;
  memset(&K, 0, sizeof(K));
  K.dt = cfg->dt; K.wb = cfg->wheelbase;
  for (int i = 0; i < 6; ++i) { K.w_des[i] = cfg->w_des_state[i]; K.w_con[i] = cfg->w_state_con[i]; K.lb[i] = cfg->state_lower[i]; K.ub[i] = cfg->state_upper[i]; K.x0[i] = R.q.x0[i]; }
  K.w_ctrl[0] = cfg->w_ctrl[0]; K.w_ctrl[1] = cfg->w_ctrl[1];
  K.w_tgt = cfg->w_tgt; K.w_ego = cfg->w_ego; K.w_ego_off = cfg->w_ego_cov_offset; K.w_exo = cfg->w_exo;
  K.w_exo_off = cfg->w_exo_cov_offset; K.w_exo_cost = cfg->w_exo_cost_offset;
  K.res = R.grid_res; K.off_x = R.offx; K.off_y = R.offy; K.target_vel = R.q.target_vel;
  K.W = W; K.H = H; K.max_iter = cfg->max_iter; K.use_exo = use_exo;
  for (int j = 0; j < IL_NA; ++j) K.alphas[j] = std::pow(1.1, -(double)(j * j));
  K.gx = R.Dp(R.A.o_gx); K.gy = R.Dp(R.A.o_gy); K.quad = quad;
  // cell centres are computed in the kernels when the grid is the numpy linspace (always in the planner mode)
  K.stepx = R.fsx / (double)(W - 1); K.stepy = R.fsy / (double)(H - 1); K.fsx = R.fsx; K.fsy = R.fsy;
  K.lin = 1;
  for (int i = 0; i < W && K.lin; ++i) K.lin = R.gx[i] == ((i == W - 1 ? K.fsx : (double)i * K.stepx) + R.offx);
  for (int i = 0; i < H && K.lin; ++i) K.lin = R.gy[i] == ((i == H - 1 ? K.fsy : (double)i * K.stepy) + R.offy);
  K.in_x0 = R.offx + 1.5 * R.grid_res; K.in_x1 = R.offx + ((double)W - 2.5) * R.grid_res;
  K.in_y0 = R.offy + 1.5 * R.grid_res; K.in_y1 = R.offy + ((double)H - 2.5) * R.grid_res;
  // reach of the relevant-agent lists beyond sigma + offset + IL_RMARGIN: a query's window cells lie within 1.5 cells of it along either
  // axis, 1.5 * sqrt(2) = 2.1214 cells away at most
  K.rel_reach = 2.125 * R.grid_res;
}

// ---- 5. stage: the device arena and the host staging of the results; the image of the arena's read-only part (c->il_img), the trees'
// device records and the constants
static int il_stage(mind_ctx *c, IlRun &R) {
  const IlqrCall &q = R.q;
  const IlArena &A = R.A;
  const IlqrChoice &ch = R.ch;
  const IlqrEvalReq *ev = q.ev;
  const int n_trees = q.n_trees;
  const bool gen = R.gen;
  int rc;
  if ((rc = ensure(c, c->ilqr_dev, A.total))) return rc;
  R.base = (char *)c->ilqr_dev.p;
  auto &hD = c->il_img.hD; auto &hF = c->il_img.hF; auto &hI = c->il_img.hI;
  hD.assign(A.nd_in, 0.0); hF.assign(A.nf, 0.f); hI.assign(A.ni, 0);
  memcpy(hD.data() + A.o_gx, R.gx.data(), R.W * sizeof(double));
  memcpy(hD.data() + A.o_gy, R.gy.data(), R.H * sizeof(double));
  if (R.n_lane_pts) memcpy(hD.data() + A.o_lane, q.lane, (size_t)R.n_lane_pts * 2 * sizeof(double));
  if (ev) {
    memcpy(hD.data() + A.o_evx, ev->x, (size_t)ev->nq * 6 * sizeof(double));
    memcpy(hD.data() + A.o_evu, ev->u, (size_t)ev->nq * 2 * sizeof(double));
    memcpy(hI.data() + A.o_evn, ev->node, (size_t)ev->nq * sizeof(int));
  }
  if (q.sc) memcpy(hD.data() + A.o_scu, q.sc->us_cand, (size_t)q.sc->n_cand * (size_t)R.Mtot * 2 * sizeof(double));
  if (q.ga) memcpy(hD.data() + A.o_gmu, q.ga->mu, (size_t)n_trees * sizeof(double));
  if (q.po) {
    const IlqrPolicyReq *po = q.po;
    memcpy(hD.data() + A.o_pk, po->k, (size_t)R.Mtot * 2 * sizeof(double));
    memcpy(hD.data() + A.o_pK, po->K, (size_t)R.Mtot * 12 * sizeof(double));
    memcpy(hD.data() + A.o_pal, po->alpha, (size_t)po->n_cand * sizeof(double));
    if (po->dx0) memcpy(hD.data() + A.o_pdx, po->dx0, (size_t)po->n_cand * 6 * sizeof(double));      // (null: the zeros of the image)
  }
  // A launch of small trees writes its results to the host ITSELF at its end (k_ilqr: the staging is page-locked and mapped), instead of two
  // copies behind it
  const IlTreeOff &L0 = A.tree[0];
  R.n_xs = L0.stats - L0.xs;
  R.n_hx = R.n_xs + (size_t)2 * IL_NSTAT * n_trees; R.n_us = (size_t)R.Mtot * 2;
  if ((rc = pl_pin(c, 5, (R.n_hx + R.n_us + 2) * sizeof(double) + (size_t)n_trees * sizeof(unsigned)))) return rc;
  R.hx = c->pl_pin[5].as<double>(); R.hus = R.hx + R.n_hx;
  R.h_abort = (unsigned *)(R.hus + R.n_us);
  R.h_done = R.h_abort + 4;               // (behind the two doubles kept for the abort word)
  c->il_early = mind_ctx::IlEarly();
  if (ch.early) {
    c->il_gen += 1u;
    if (c->il_gen == 0u) c->il_gen = 1u;
    for (int t = 0; t < n_trees; ++t) R.h_done[t] = 0u;
    c->il_early.xs = R.hx; c->il_early.us = R.hus; c->il_early.done = R.h_done; c->il_early.gen = c->il_gen; c->il_early.n_trees = n_trees; c->il_early.nodes = R.Mtot;
  }
  float *dF = R.dF();
  int *dI = R.dI();
  R.hT.resize(n_trees);
  long moff = 0;
  for (int t = 0; t < n_trees; ++t) {
    const mind_cost_tree &tr = q.trees[t];
    const IlTreeOff &L = A.tree[t];
    const IlTables &T = c->il_tab[t];
    const size_t M = tr.n_nodes, a = R.n_agents[t];
    if (q.us_init) memcpy(hD.data() + L.us, q.us_init + moff * 2, 2 * M * sizeof(double));
    if (tr.prob) memcpy(hF.data() + L.prob, tr.prob, M * sizeof(float));
    if (gen) memcpy(hD.data() + L.nodew, tr.node_w, M * IL_NW * sizeof(double));
    if (tr.agent_mean && !gen && !R.dev_flat) memcpy(hF.data() + L.mean, tr.agent_mean, M * a * 2 * sizeof(float));
    if (tr.agent_cov && !gen && !R.dev_flat) memcpy(hF.data() + L.cov, tr.agent_cov, M * a * sizeof(float));
    il_stage_ints(L, tr.parent, T, hI.data());
    IlqrTreeDev &D = R.hT[t];
    D.M = tr.n_nodes; D.n_agents = (int)a; D.n_levels = T.nl; D.pad = 0;
    D.parent = dI + L.parent; D.level_start = dI + L.lstart; D.level_nodes = dI + L.lnodes;
    D.child_start = dI + L.cstart; D.child_list = dI + L.clist;
    D.rel = dI + L.rel;
    D.relag = R.Dp(L.relag);
    D.field = gen ? (const double *)(R.base + L.field) : nullptr;
    D.node_w = gen ? R.Dp(L.nodew) : nullptr;
    D.n_segs = T.nseg; D.n_slevels = T.nsl; D.max_level_segs = T.maxls; D.pad2 = 0;
    D.seg_start = dI + L.sstart; D.seg_nodes = dI + L.snodes; D.slevel_start = dI + L.slstart; D.slevel_segs = dI + L.slsegs; D.seg_rec = dI + L.segrec;
    D.n_fsteps = T.nfs; D.padf = 0;
    D.trace = R.trace_cap > 0 ? R.Dp(L.trace) : nullptr; D.trace_cap = R.trace_cap; D.padt = 0;
    D.fstep_start = dI + L.fsstart; D.fstep_q0 = dI + L.fsitems; D.fstep_q1 = dI + L.fsq1; D.fstep_nstart = dI + L.fsnstart; D.fstep_nodes = dI + L.fsnodes;
    D.prob = dF + L.prob; D.mean = dF + L.mean; D.cov = dF + L.cov;
    if (R.dev_flat) { D.mean = c->plan.dev_fmean + (size_t)moff * a * 2; D.cov = c->plan.dev_fcov + (size_t)moff * a; }
    D.xs = R.Dp(L.xs); D.us = R.Dp(L.us); D.Fx = R.Dp(L.Fx); D.L = R.Dp(L.L); D.Lx = R.Dp(L.Lx); D.Lxx = R.Dp(L.Lxx);
    D.k = R.Dp(L.k); D.K = R.Dp(L.K); D.Vx = R.Dp(L.Vx); D.Vxx = R.Dp(L.Vxx);
    D.xs_new = R.Dp(L.xsn); D.us_new = R.Dp(L.usn); D.L_new = R.Dp(L.Ln); D.stats = R.Dp(L.stats);
    D.ctl = ch.form == 2 ? (IlSlotCtl *)(dI + A.o_ctl + A.ctl_ints * (size_t)t) : nullptr;
    D.h_xs = ch.host_out ? R.hx + (L.xs - L0.xs) : nullptr; D.h_us = ch.host_out ? R.hus + (L.us - L0.us) : nullptr;
    D.h_stats = ch.host_out ? R.hx + (L.stats - L0.xs) : nullptr;
    D.h_done = ch.early ? R.h_done + t : nullptr; D.h_gen = c->il_gen; D.pad_h = 0;
    if (ch.early && ((L.xs - L0.xs) != (size_t)moff * 6 || (L.us - L0.us) != (size_t)moff * 2)) return fail(c, MIND_EINVAL, "tree-iLQR arena: results are not contiguous");
    D.dset = ch.spec ? (long long)L.Fx2 - (long long)L.Fx : 0; D.drel = ch.spec ? (long long)L.rel2 - (long long)L.rel : 0;
    if (ch.spec && (L.L2 - L.L != L.Fx2 - L.Fx || L.Lx2 - L.Lx != L.Fx2 - L.Fx || L.Lxx2 - L.Lxx != L.Fx2 - L.Fx || (R.use_exo && L.relag2 - L.relag != L.Fx2 - L.Fx)))
      return fail(c, MIND_EINVAL, "tree-iLQR arena: the two derivative sets are laid out differently");
    moff += (long)M;
  }
  // a field prepared ahead for exactly this grid and lane (il_field_prepare): the kernels read it where it is
  R.field_ahead = !gen && !ev && !q.sc && !q.ga && !q.po && c->il_field_valid && c->il_field_key[0] == q.x0[0] && c->il_field_key[1] == q.x0[1] && c->il_field_key[2] == (double)R.W &&
                  c->il_field_key[3] == (double)R.H && c->il_field_key[4] == R.grid_res && c->il_field_lane.size() == 2 * (size_t)R.n_lane_pts &&
                  memcmp(c->il_field_lane.data(), q.lane, c->il_field_lane.size() * sizeof(double)) == 0;
  c->il_field_valid = false;         // (one call's worth: the next call makes its own or prepares again)
  double *quad = R.field_ahead ? (double *)c->il_field.p + (size_t)R.W + R.H + 2 * (size_t)R.n_lane_pts : R.Dp(A.o_quad);
  il_fill_const(R.K[0], q.cfg, R.use_exo_first, R, quad);
  if (q.cfg2) il_fill_const(R.K[1], q.cfg2, 1, R, quad);      // the full-cost fit: same grid / state / lane field, its own weights
  else R.K[1] = R.K[0];
  {
    const auto off = [&R](size_t o) { return (size_t)((const char *)R.Dp(o) - R.base); };
    c->il_dbg[0] = off(L0.L); c->il_dbg[1] = off(L0.Lx); c->il_dbg[2] = off(L0.Lxx); c->il_dbg[3] = off(L0.Fx); c->il_dbg[4] = off(L0.xs);
    c->il_dbg[5] = (size_t)q.trees[0].n_nodes;
  }
  return MIND_OK;
}

// ---- 6. upload: one staged copy of everything the host provides (+ the materialised fields of the generic mode)
// (page-locked staging: a pageable source makes hipMemcpyAsync a blocking staged copy that also stalls the other contexts of the
// process -- several planner threads on one GPU then run slower together than one alone)
static int il_upload(mind_ctx *c, IlRun &R, hipStream_t st) {
  const IlArena &A = R.A;
  const int n_trees = R.q.n_trees;
  for (int t = 0; t < n_trees && R.gen; ++t)
    HIPCHK(c, hipMemcpyAsync(R.base + A.tree[t].field, R.q.trees[t].field, (size_t)R.q.trees[t].n_nodes * R.W * R.H * sizeof(double), hipMemcpyHostToDevice, st));
  int rc;
  if ((rc = pl_pin(c, 4, A.o_work))) return rc;
  char *up = c->pl_pin[4].as<char>();
  memset(up, 0, A.o_work);
  memcpy(up, c->il_img.hD.data(), A.bytesIn);
  if (A.bytesF) memcpy(up + A.bytesIn, c->il_img.hF.data(), A.bytesF);
  if (A.bytesI) memcpy(up + A.bytesIn + A.bytesF, c->il_img.hI.data(), A.bytesI);
  if (R.ch.starve_followers) ((unsigned *)(up + A.bytesIn + A.bytesF))[A.o_bars + 4 * (size_t)n_trees + 1] = 1u;
  memcpy(up + A.o_structs, R.hT.data(), (size_t)n_trees * sizeof(IlqrTreeDev));
  memcpy(up + A.o_consts, R.K, 2 * sizeof(IlqrConst));
  R.up = up;
  return pl_upload(c, R.base, up, A.o_work, st);
}

// ---- 8. finish: everything behind the launch -- the wait, the fallback of a launch that was not resident, the outputs -- over a record of
// plain values: run at once, or kept in the context by a call with begin_only and run by mind_ilqr_finish (the caller's thread is free meanwhile)
struct IlPending {
  hipStream_t st;
  bool gen;
  int n_trees, n_phases, use_exo, trace_cap;
  long Mtot;
  IlqrChoice ch;
  // the launch's arguments and its upload (the fallback repeats both)
  const IlqrTreeDev *dT;
  const IlqrConst *dK;
  unsigned *dBars;
  size_t il_lds, o_work;
  char *base;
  const char *up;
  // results: on the device, in the host staging, and where the caller wants them
  const double *d_xs, *d_us;
  double *hx, *hus;
  const unsigned *h_abort;
  size_t n_xs, n_hx, n_us;
  double *xs, *us;
  mind_ilqr_stats *stats, *stats2;
  struct Tree { int M, nl, nseg, nsl, maxls, a; const double *trace; };
  std::vector<Tree> tree;
};

static void il_launch_kernel(const IlPending &P, int form) {
  const IlqrChoice &ch = P.ch;
  const int nt = P.n_trees;
  const dim3 block(IL_THREADS);
  if (P.gen) hipLaunchKernelGGL((k_ilqr<true, 0>), dim3(nt), block, P.il_lds, P.st, P.dT, P.dK, P.n_phases, nt, 1, P.dBars, 0);
  else if (form == 2) hipLaunchKernelGGL((k_ilqr<false, 2>), dim3(ch.grid), block, P.il_lds, P.st, P.dT, P.dK, P.n_phases, nt, ch.GS, P.dBars, ch.spec);
  else if (form == 1) hipLaunchKernelGGL((k_ilqr<false, 1>), dim3(ch.grid), block, P.il_lds, P.st, P.dT, P.dK, P.n_phases, nt, ch.G, P.dBars, 0);
  else hipLaunchKernelGGL((k_ilqr<false, 0>), dim3(nt), block, P.il_lds, P.st, P.dT, P.dK, P.n_phases, nt, 1, P.dBars, 0);
}

static int il_read_back(mind_ctx *c, const IlPending &P) {
  if (P.ch.host_out) return MIND_OK;
  HIPCHK(c, hipMemcpyAsync(P.hx, P.d_xs, P.n_hx * sizeof(double), hipMemcpyDeviceToHost, P.st));
  HIPCHK(c, hipMemcpyAsync(P.hus, P.d_us, P.n_us * sizeof(double), hipMemcpyDeviceToHost, P.st));
  return MIND_OK;
}

static int il_finish_run(mind_ctx *c, const IlPending &P) {
  static const bool trace = getenv("MIND_ILQR_TRACE") != nullptr;
  const int n_trees = P.n_trees, n_phases = P.n_phases;
  int rc;
  HIPCHK(c, hipStreamSynchronize(P.st));
  if (c->profiling) HIPCHK(c, hipEventElapsedTime(&c->ilqr_ms, c->ev_il0, c->ev_il1));
  if (P.ch.form == 1 && *P.h_abort) {
    // the workgroups of a wide tree did not meet at a barrier within ~2 s: the launch was not fully resident (another context or
    // stream held CUs -- several planners on one GPU).  The one-workgroup-per-tree kernel needs no co-residency: the upload (initial
    // controls, zeroed barrier words) is repeated and the call solved with it -- same arithmetic, same results, just slower.
    c->n_ilqr_fallbacks++;
    HIPCHK(c, hipMemcpyAsync(P.base, P.up, P.o_work, hipMemcpyHostToDevice, P.st));
    il_launch_kernel(P, 0);
    HIPCHK(c, hipGetLastError());
    c->ilqr_multi = 1;
    if ((rc = il_read_back(c, P))) return rc;
    HIPCHK(c, hipStreamSynchronize(P.st));
  }
  memcpy(P.xs, P.hx, (size_t)P.Mtot * 6 * sizeof(double));
  memcpy(P.us, P.hus, P.n_us * sizeof(double));
  // a tree's statistics of one fit, in the page-locked staging
  const auto hstat = [&P](int t, int ph) { return P.hx + P.n_xs + (size_t)2 * IL_NSTAT * t + (size_t)ph * IL_NSTAT; };
  c->il_trace_dev.assign(n_trees, nullptr);
  c->il_trace_its.assign((size_t)2 * n_trees, 0);
  c->il_trace_cap = P.trace_cap; c->il_trace_phases = n_phases;
  for (int t = 0; t < n_trees; ++t) {
    c->il_trace_dev[t] = P.trace_cap > 0 ? P.tree[t].trace : nullptr;
    for (int ph = 0; ph < n_phases; ++ph) c->il_trace_its[2 * t + ph] = (int)hstat(t, ph)[0];
  }
  c->il_spec_req = 0; c->il_spec_hit = 0;
#ifndef IL_PROFILE
  for (int t = 0; t < n_trees; ++t)
    for (int ph = 0; ph < n_phases; ++ph) { c->il_spec_req += (long long)hstat(t, ph)[9]; c->il_spec_hit += (long long)hstat(t, ph)[10]; }
#endif
  // phase cycles of the launch's critical tree (the one with the most cycles over all its fits): what bounds the launch
  double best = -1.0;
  for (int t = 0; t < n_trees; ++t) {
    double tot = 0.0, ph_c[5] = {0, 0, 0, 0, 0}, passes = 0.0;
    for (int ph = 0; ph < n_phases; ++ph) {
      const double *h = hstat(t, ph);
      ph_c[0] += h[4]; ph_c[1] += h[5]; ph_c[2] += h[8]; ph_c[3] += h[6]; ph_c[4] += h[7];
      passes += h[IL_NSTAT - 1];
    }
    for (double v : ph_c) tot += v;
    if (tot > best) {
      best = tot;
      double *o = c->il_prof;
      o[0] = P.tree[t].M; o[1] = P.tree[t].nl; o[2] = passes;
      for (int k = 0; k < 5; ++k) o[3 + k] = ph_c[k];       // derivatives, backward, state chain, cost pass, selection
      o[8] = (double)n_trees;
    }
  }
  for (int ph = 0; ph < n_phases; ++ph) {
    mind_ilqr_stats *so = ph == 0 ? P.stats : P.stats2;
    if (!so) continue;
    for (int t = 0; t < n_trees; ++t) {
      const double *h = hstat(t, ph);
      const IlPending::Tree &T = P.tree[t];
      so[t].iterations = (int)h[0]; so[t].converged = (int)h[1];
      so[t].J = h[2]; so[t].mu = h[3];
      if (!trace) continue;
      fprintf(stderr, "[k_ilqr] tree %d exo %d M %d segs %d seg-levels %d widest %d agents %d it %d passes %.0f: cycles derivatives %.0f backward %.0f state chain %.0f cost pass %.0f select %.0f\n", t,
              n_phases == 2 ? ph : P.use_exo, T.M, T.nseg, T.nsl, T.maxls, T.a, so[t].iterations, h[IL_NSTAT - 1], h[4], h[5], h[8], h[6], h[7]);
#ifdef IL_PROFILE
      fprintf(stderr, "[k_ilqr prof] wave0: chain node (n=%.0f): stage %.0f u+dyn+store %.0f | cost chunk (n=%.0f): stage+loads %.0f field %.0f cost+store %.0f | riccati node (n=%.0f): products %.0f Qxx %.0f solve %.0f update %.0f | deriv block (n=%.0f): setup %.0f tasks %.0f assemble %.0f\n",
              h[13], h[8] / fmax(h[13], 1), h[9] / fmax(h[13], 1),
              h[23], h[10] / fmax(h[23], 1), h[11] / fmax(h[23], 1), h[12] / fmax(h[23], 1),
              h[18], h[14] / fmax(h[18], 1), h[15] / fmax(h[18], 1), h[16] / fmax(h[18], 1), h[17] / fmax(h[18], 1),
              h[22], h[19] / fmax(h[22], 1), h[20] / fmax(h[22], 1), h[21] / fmax(h[22], 1));
#endif
    }
  }
  return MIND_OK;
}

// the cost evaluation's launch: node costs at the requested points, read back at once
static int il_eval(mind_ctx *c, const IlRun &R, hipStream_t st) {
  const IlqrEvalReq *ev = R.q.ev;
  const IlArena &A = R.A;
  const IlqrTreeDev *dT = (const IlqrTreeDev *)(R.base + A.o_structs);
  const size_t lds = (IL_SCR + (size_t)4 * R.amax) * sizeof(double);
  if (R.gen) hipLaunchKernelGGL(k_cost_eval<true>, dim3(ev->nq), dim3(64), lds, st, dT, R.K[0], ev->nq, R.dI() + A.o_evn, R.Dp(A.o_evx), R.Dp(A.o_evu), R.Dp(A.o_evo));
  else hipLaunchKernelGGL(k_cost_eval<false>, dim3(ev->nq), dim3(64), lds, st, dT, R.K[0], ev->nq, R.dI() + A.o_evn, R.Dp(A.o_evx), R.Dp(A.o_evu), R.Dp(A.o_evo));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(ev->out, R.Dp(A.o_evo), (size_t)ev->nq * IL_EVAL_OUT * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return MIND_OK;
}

// the scoring launch: states, node costs and their sums of every (candidate, tree), read back at once
static int il_score(mind_ctx *c, const IlRun &R, hipStream_t st) {
  const IlqrScoreReq *sc = R.q.sc;
  const IlArena &A = R.A;
  const int n_trees = R.q.n_trees;
  const IlqrTreeDev *dT = (const IlqrTreeDev *)(R.base + A.o_structs);
  const int cb = il_score_block(c->it, c->n_cu, n_trees, sc->n_cand);
  const dim3 grid((sc->n_cand + cb - 1) / cb, n_trees), block(IL_SC_THREADS);
  const size_t lds = il_score_lds_bytes(R.amax);
  const size_t rows = (size_t)sc->n_cand * (size_t)R.Mtot;
  if (R.gen) hipLaunchKernelGGL(k_ilqr_score<true>, grid, block, lds, st, dT, R.K[0], n_trees, sc->n_cand, cb, R.Mtot, il_ag_doubles(R.amax), R.Dp(A.o_scu), R.Dp(A.o_scx), R.Dp(A.o_scl), R.Dp(A.o_scj));
  else hipLaunchKernelGGL(k_ilqr_score<false>, grid, block, lds, st, dT, R.K[0], n_trees, sc->n_cand, cb, R.Mtot, il_ag_doubles(R.amax), R.Dp(A.o_scu), R.Dp(A.o_scx), R.Dp(A.o_scl), R.Dp(A.o_scj));
  HIPCHK(c, hipGetLastError());
  if (sc->xs) HIPCHK(c, hipMemcpyAsync(sc->xs, R.Dp(A.o_scx), rows * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (sc->L) HIPCHK(c, hipMemcpyAsync(sc->L, R.Dp(A.o_scl), rows * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(sc->J, R.Dp(A.o_scj), (size_t)sc->n_cand * n_trees * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return MIND_OK;
}

// the gains launch: one workgroup per tree; the outputs lie back to back in the arena (il_layout) and come back in ONE copy into the
// page-locked read-back staging, from where the wanted ones are handed out
static int il_gains(mind_ctx *c, const IlRun &R, hipStream_t st) {
  const mind_ilqr_gains_out *o = R.q.ga->out;
  const IlArena &A = R.A;
  const int n_trees = R.q.n_trees;
  const IlqrTreeDev *dT = (const IlqrTreeDev *)(R.base + A.o_structs);
  const size_t lds = il_gains_lds_bytes(R.amax), M = (size_t)R.Mtot;
  if (R.gen) hipLaunchKernelGGL(k_ilqr_gains<true>, dim3(n_trees), dim3(IL_PG_THREADS), lds, st, dT, R.K[0], n_trees, il_ag_doubles(R.amax), R.Dp(A.o_gmu), R.Dp(A.o_gk), R.Dp(A.o_gK), R.Dp(A.o_gdv), R.Dp(A.o_gvx), R.Dp(A.o_gvxx), R.Dp(A.o_gxs), R.Dp(A.o_gl), R.Dp(A.o_gj), R.Dp(A.o_gbad));
  else hipLaunchKernelGGL(k_ilqr_gains<false>, dim3(n_trees), dim3(IL_PG_THREADS), lds, st, dT, R.K[0], n_trees, il_ag_doubles(R.amax), R.Dp(A.o_gmu), R.Dp(A.o_gk), R.Dp(A.o_gK), R.Dp(A.o_gdv), R.Dp(A.o_gvx), R.Dp(A.o_gvxx), R.Dp(A.o_gxs), R.Dp(A.o_gl), R.Dp(A.o_gj), R.Dp(A.o_gbad));
  HIPCHK(c, hipGetLastError());
  const size_t span = A.o_gbad + (size_t)n_trees - A.o_gk;
  int rc;
  if ((rc = pl_pin(c, 5, span * sizeof(double)))) return rc;      // (grows the staging il_stage sized for a solve; this call uses none of that)
  const double *h = c->pl_pin[5].as<double>();
  HIPCHK(c, hipMemcpyAsync(c->pl_pin[5], R.Dp(A.o_gk), span * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const struct { double *dst; size_t src, n; } outs[8] = {{o->k, A.o_gk, 2 * M}, {o->K, A.o_gK, 12 * M}, {o->dV, A.o_gdv, M}, {o->V_x, A.o_gvx, 6 * M},
                                                          {o->V_xx, A.o_gvxx, 36 * M}, {o->xs, A.o_gxs, 6 * M}, {o->L, A.o_gl, M}, {o->J, A.o_gj, (size_t)n_trees}};
  for (const auto &e : outs)
    if (e.dst) memcpy(e.dst, h + (e.src - A.o_gk), e.n * sizeof(double));
  for (int t = 0; t < n_trees; ++t) o->bad_node[t] = (int32_t)h[A.o_gbad - A.o_gk + t];
  return MIND_OK;
}

// the policy-rollout launch: states, controls, node costs and their sums of every (candidate, tree), read back at once
static int il_policy(mind_ctx *c, const IlRun &R, hipStream_t st, int cb) {
  const IlqrPolicyReq *po = R.q.po;
  const IlArena &A = R.A;
  const int n_trees = R.q.n_trees;
  const IlqrTreeDev *dT = (const IlqrTreeDev *)(R.base + A.o_structs);
  const dim3 grid((po->n_cand + cb - 1) / cb, n_trees), block(IL_SC_THREADS);
  const size_t lds = il_score_lds_bytes(R.amax);
  const size_t rows = (size_t)po->n_cand * (size_t)R.Mtot;
  if (R.gen) hipLaunchKernelGGL(k_ilqr_policy<true>, grid, block, lds, st, dT, R.K[0], n_trees, po->n_cand, cb, R.Mtot, il_ag_doubles(R.amax), R.Dp(A.o_pk), R.Dp(A.o_pK), R.Dp(A.o_pal), R.Dp(A.o_pdx), R.Dp(A.o_pxn), R.Dp(A.o_pxs), R.Dp(A.o_pus), R.Dp(A.o_pl), R.Dp(A.o_pj));
  else hipLaunchKernelGGL(k_ilqr_policy<false>, grid, block, lds, st, dT, R.K[0], n_trees, po->n_cand, cb, R.Mtot, il_ag_doubles(R.amax), R.Dp(A.o_pk), R.Dp(A.o_pK), R.Dp(A.o_pal), R.Dp(A.o_pdx), R.Dp(A.o_pxn), R.Dp(A.o_pxs), R.Dp(A.o_pus), R.Dp(A.o_pl), R.Dp(A.o_pj));
  HIPCHK(c, hipGetLastError());
  if (po->xs) HIPCHK(c, hipMemcpyAsync(po->xs, R.Dp(A.o_pxs), rows * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (po->us_out) HIPCHK(c, hipMemcpyAsync(po->us_out, R.Dp(A.o_pus), rows * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (po->L) HIPCHK(c, hipMemcpyAsync(po->L, R.Dp(A.o_pl), rows * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(po->J, R.Dp(A.o_pj), (size_t)po->n_cand * n_trees * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return MIND_OK;
}

// ---- 7. launch: the lane field (unless one was prepared ahead), k_ilqr in the chosen form, the copies behind it; leaves what il_finish_run needs in P
static int il_launch(mind_ctx *c, const IlRun &R, hipStream_t st, IlPending &P) {
  const IlqrCall &q = R.q;
  const IlArena &A = R.A;
  const IlqrChoice &ch = R.ch;
  const int n_trees = q.n_trees;
  if (R.field_ahead) HIPCHK(c, hipStreamWaitEvent(st, c->ev_field, 0));
  else if (!R.gen) hipLaunchKernelGGL(k_lane_field, dim3((R.W * R.H + 255) / 256), dim3(256), 0, st, R.K[0].gx.p, R.K[0].gy.p, R.W, R.H, R.Dp(A.o_lane), R.n_lane_pts, R.Dp(A.o_quad));
  if (q.ev) return il_eval(c, R, st);
  if (q.sc) return il_score(c, R, st);
  if (q.ga) return il_gains(c, R, st);
  if (q.po) return il_policy(c, R, st, R.pol_cb);
  P.st = st; P.gen = R.gen; P.n_trees = n_trees; P.n_phases = R.n_phases; P.use_exo = R.use_exo; P.trace_cap = R.trace_cap; P.Mtot = R.Mtot; P.ch = ch;
  P.dT = (const IlqrTreeDev *)(R.base + A.o_structs); P.dK = (const IlqrConst *)(R.base + A.o_consts);
  P.dBars = (unsigned *)(R.dI() + A.o_bars);
  P.il_lds = il_lds_bytes(R.amax); P.o_work = A.o_work; P.base = R.base; P.up = R.up;
  P.d_xs = R.Dp(A.tree[0].xs); P.d_us = R.Dp(A.tree[0].us);
  P.hx = R.hx; P.hus = R.hus; P.h_abort = R.h_abort; P.n_xs = R.n_xs; P.n_hx = R.n_hx; P.n_us = R.n_us;
  P.xs = q.xs; P.us = q.us; P.stats = q.stats; P.stats2 = q.stats2;
  P.tree.resize(n_trees);
  for (int t = 0; t < n_trees; ++t) {
    const IlTables &T = c->il_tab[t];
    P.tree[t] = {q.trees[t].n_nodes, T.nl, T.nseg, T.nsl, T.maxls, R.n_agents[t], R.Dp(A.tree[t].trace)};
  }
  if (c->profiling) {
    if (!c->ev_il0) { HIPCHK(c, c->ev_il0.create()); HIPCHK(c, c->ev_il1.create()); }
    HIPCHK(c, hipEventRecord(c->ev_il0, st));
  }
  c->ilqr_trees = n_trees; c->ilqr_multi = ch.wgs_per_tree; c->ilqr_ms = 0.f;
  il_launch_kernel(P, ch.form);
  HIPCHK(c, hipGetLastError());
  if (c->profiling) HIPCHK(c, hipEventRecord(c->ev_il1, st));
  int rc;
  if ((rc = il_read_back(c, P))) return rc;
  if (ch.form == 1) HIPCHK(c, hipMemcpyAsync(R.h_abort, P.dBars + 4 * (size_t)n_trees, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  return MIND_OK;
}

// Shared host side of the tree-iLQR exports: build the device arena, then either run the solver (q.ev == nullptr) or evaluate node costs at
// the requested points
static int il_solve(mind_ctx *c, const IlqrCall &q) {
  IlRun R(q);
  int rc;
  if ((rc = il_check(c, q, R))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  IlStamp stamp;
  il_grid(R);
  int maxM = 0;
  for (int t = 0; t < q.n_trees; ++t) maxM = std::max(maxM, q.trees[t].n_nodes);
  const bool other = q.ev || q.sc || q.ga || q.po;      // a request served instead of a solve
  R.ch = il_choose(c->it, c->n_cu, q.n_trees, maxM, R.Mtot, R.gen, other);
  if ((rc = il_build_tables(c, q))) return rc;
  IlShape shape{R.W, R.H, R.n_lane_pts, q.ev ? q.ev->nq : 0, q.n_trees, R.n_agents.data(), R.gen, R.use_exo != 0, R.dev_flat, R.trace_cap, q.sc ? q.sc->n_cand : 0};
  shape.gains = q.ga != nullptr;
  if (q.po) {
    R.pol_cb = il_score_block(c->it, c->n_cu, q.n_trees, q.po->n_cand);
    shape.n_pol = q.po->n_cand; shape.n_pol_blk = (q.po->n_cand + R.pol_cb - 1) / R.pol_cb;
  }
  il_layout(shape, R.ch, c->il_tab.data(), R.A);
  stamp("tables built");
  if ((rc = il_stage(c, R))) return rc;
  stamp("staged in vectors");
  if ((rc = il_upload(c, R, st))) return rc;
  stamp("upload queued");
  IlPending P;
  if ((rc = il_launch(c, R, st, P)) || other) return rc;
  stamp("kernel launched");
  if (!q.begin_only) return il_finish_run(c, P);
  c->il_finish = [c, P = std::move(P)]() { return il_finish_run(c, P); };
  return MIND_OK;
}

// -------------------------------------------------------------------------------------------------
// exports
// -------------------------------------------------------------------------------------------------
static IlqrCall il_contingency_call(const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full, const mind_cost_tree *trees, int n_trees, const double *x0,
                                    const double *target_lane, int n_lane_pts, double target_vel, double *xs, double *us, mind_ilqr_stats *stats_warm,
                                    mind_ilqr_stats *stats_full) {
  IlqrCall q;
  q.cfg = cfg_warm; q.cfg2 = cfg_full; q.trees = trees; q.n_trees = n_trees; q.x0 = x0; q.lane = target_lane; q.n_lane_pts = n_lane_pts;
  q.target_vel = target_vel; q.xs = xs; q.us = us; q.stats = stats_warm; q.stats2 = stats_full;
  return q;
}

extern "C" int mind_ilqr_contingency_begin(mind_ctx *c, const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full,
                                           const mind_cost_tree *trees, int n_trees, const double *x0, const double *target_lane,
                                           int n_lane_pts, double target_vel, double *xs, double *us,
                                           mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full) {
  if (!c || !cfg_full) return fail(c, MIND_EINVAL, "mind_ilqr_contingency_begin: null configuration");
  IlqrCall q = il_contingency_call(cfg_warm, cfg_full, trees, n_trees, x0, target_lane, n_lane_pts, target_vel, xs, us, stats_warm, stats_full);
  q.begin_only = true;
  return il_solve(c, q);
}

// mind_ilqr_contingency_begin on the cost trees the last mind_aime_plan of this context flattened (its library-owned tables: no tree
// arrays cross the boundary again)
extern "C" int mind_ilqr_contingency_begin_plan(mind_ctx *c, const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full, const double *x0,
                                                const double *target_lane, int n_lane_pts, double target_vel, double *xs, double *us,
                                                mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full) {
  if (!c || !cfg_full) return fail(c, MIND_EINVAL, "mind_ilqr_contingency_begin_plan: null configuration");
  const int nt = (int)c->plan.book.tree_top.size();
  if (nt <= 0 || c->plan.agents <= 0) return fail(c, MIND_ESTATE, "mind_ilqr_contingency_begin_plan: the context holds no planned cost trees");
  const int a = c->plan.agents;
  std::vector<mind_cost_tree> trees(nt);
  for (int t = 0; t < nt; ++t) {
    const size_t lo = (size_t)c->plan.book.tree_off[t];
    mind_cost_tree &T = trees[t];
    memset(&T, 0, sizeof(T));
    T.n_nodes = c->plan.book.tree_off[t + 1] - c->plan.book.tree_off[t];
    T.parent = c->plan.book.flat_parent.data() + lo; T.prob = c->plan.book.flat_prob.data() + lo;
    T.n_agents = a;
    // (host copies when the plan has read them back already; the call itself reads the device buffers k_aime_flat filled)
    T.agent_mean = c->plan.fmean_p ? c->plan.fmean_p + lo * a * 2 : nullptr; T.agent_cov = c->plan.fcov_p ? c->plan.fcov_p + lo * a : nullptr;
  }
  IlqrCall q = il_contingency_call(cfg_warm, cfg_full, trees.data(), nt, x0, target_lane, n_lane_pts, target_vel, xs, us, stats_warm, stats_full);
  q.begin_only = true;
  q.dev_flat = true;
  return il_solve(c, q);
}

extern "C" int mind_ilqr_finish(mind_ctx *c) {
  if (!c) return MIND_EINVAL;
  if (!c->il_finish) return fail(c, MIND_ESTATE, "mind_ilqr_finish: no tree-iLQR call was begun on this context");
  std::function<int()> fin = std::move(c->il_finish);
  c->il_finish = nullptr;
  c->il_finish_owned = false;
  c->il_early = mind_ctx::IlEarly();
  return fin();
}

extern "C" int mind_ilqr_contingency(mind_ctx *c, const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full,
                                     const mind_cost_tree *trees, int n_trees, const double *x0, const double *target_lane,
                                     int n_lane_pts, double target_vel, double *xs, double *us,
                                     mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full) {
  if (!cfg_full) return fail(c, MIND_EINVAL, "mind_ilqr_contingency: null configuration");
  return il_solve(c, il_contingency_call(cfg_warm, cfg_full, trees, n_trees, x0, target_lane, n_lane_pts, target_vel, xs, us, stats_warm, stats_full));
}

extern "C" int mind_ilqr_solve_trees(mind_ctx *c, const mind_ilqr_cfg *cfg, const mind_cost_tree *trees, int n_trees,
                                     const double *x0, const double *target_lane, int n_lane_pts, double target_vel,
                                     int use_exo, const double *us_init, double *xs, double *us,
                                     mind_ilqr_stats *stats) {
  IlqrCall q;
  q.cfg = cfg; q.trees = trees; q.n_trees = n_trees; q.x0 = x0; q.lane = target_lane; q.n_lane_pts = n_lane_pts; q.target_vel = target_vel;
  q.use_exo = use_exo; q.us_init = us_init; q.xs = xs; q.us = us; q.stats = stats;
  return il_solve(c, q);
}

extern "C" int mind_ilqr_solve_fields(mind_ctx *c, const mind_ilqr_cfg *cfg, const mind_field_grid *grid,
                                      const mind_cost_tree *trees, int n_trees, const double *x0,
                                      const double *us_init, double *xs, double *us, mind_ilqr_stats *stats) {
  if (!grid) return fail(c, MIND_EINVAL, "mind_ilqr_solve_fields: null grid");
  IlqrCall q;
  q.cfg = cfg; q.grid = grid; q.trees = trees; q.n_trees = n_trees; q.x0 = x0; q.us_init = us_init; q.xs = xs; q.us = us; q.stats = stats;
  return il_solve(c, q);
}

extern "C" int mind_cost_eval(mind_ctx *c, const mind_ilqr_cfg *cfg, const mind_field_grid *grid, const mind_cost_tree *tree,
                              const double *x0, const double *target_lane, int n_lane_pts, double target_vel, int use_exo,
                              int n_query, const int32_t *node, const double *x, const double *u, double *out) {
  if (n_query <= 0 || !node || !x || !u || !out) return fail(c, MIND_EINVAL, "mind_cost_eval: bad argument");
  const IlqrEvalReq ev{n_query, node, x, u, out};
  IlqrCall q;
  q.cfg = cfg; q.grid = grid; q.trees = tree; q.n_trees = 1; q.x0 = x0; q.lane = target_lane; q.n_lane_pts = n_lane_pts; q.target_vel = target_vel;
  q.use_exo = use_exo; q.ev = &ev;
  return il_solve(c, q);
}

extern "C" int mind_ilqr_score_trees(mind_ctx *c, const mind_ilqr_cfg *cfg, const mind_field_grid *grid, const mind_cost_tree *trees, int n_trees,
                                     const double *x0, const double *target_lane, int n_lane_pts, double target_vel, int use_exo, int n_cand,
                                     const double *us_cand, double *xs, double *L, double *J) {
  const IlqrScoreReq sc{n_cand, us_cand, xs, L, J};
  IlqrCall q;
  q.cfg = cfg; q.grid = grid; q.trees = trees; q.n_trees = n_trees; q.x0 = x0; q.lane = target_lane; q.n_lane_pts = n_lane_pts; q.target_vel = target_vel;
  q.use_exo = use_exo; q.sc = &sc;
  return il_solve(c, q);
}

extern "C" int mind_ilqr_gains(mind_ctx *c, const mind_ilqr_cfg *cfg, const mind_field_grid *grid, const mind_cost_tree *trees, int n_trees,
                               const double *x0, const double *target_lane, int n_lane_pts, double target_vel, int use_exo, const double *us,
                               const double *mu, const mind_ilqr_gains_out *out) {
  const IlqrGainsReq ga{us, mu, out};
  IlqrCall q;
  q.cfg = cfg; q.grid = grid; q.trees = trees; q.n_trees = n_trees; q.x0 = x0; q.lane = target_lane; q.n_lane_pts = n_lane_pts; q.target_vel = target_vel;
  q.use_exo = use_exo; q.us_init = us; q.ga = &ga;
  return il_solve(c, q);
}

extern "C" int mind_ilqr_policy_rollouts(mind_ctx *c, const mind_ilqr_cfg *cfg, const mind_field_grid *grid, const mind_cost_tree *trees, int n_trees,
                                         const double *x0, const double *target_lane, int n_lane_pts, double target_vel, int use_exo,
                                         const double *us, const double *k, const double *K, int n_cand, const double *alpha, const double *dx0,
                                         double *xs, double *us_out, double *L, double *J) {
  const IlqrPolicyReq po{n_cand, us, k, K, alpha, dx0, xs, us_out, L, J};
  IlqrCall q;
  q.cfg = cfg; q.grid = grid; q.trees = trees; q.n_trees = n_trees; q.x0 = x0; q.lane = target_lane; q.n_lane_pts = n_lane_pts; q.target_vel = target_vel;
  q.use_exo = use_exo; q.us_init = us; q.po = &po;
  return il_solve(c, q);
}

// il_choose's record and il_tree_tables' tables for a call of the given knobs, device size and trees (layout: include/mind_hip.h)
#define IL_PLAN_HEADER 16
extern "C" int mind_debug_ilqr_plan(const char *const *knob_names, const int *knob_values, int n_knobs, int n_cu, int mode, int n_trees,
                                    const int *n_nodes, const int32_t *parents, long long *out, int cap, int *bad) {
  if (bad) bad[0] = bad[1] = -1;
  if (n_knobs < 0 || (n_knobs > 0 && (!knob_names || !knob_values)) || n_cu <= 0 || mode < 0 || mode > 7 || n_trees <= 0 || !n_nodes || !parents ||
      cap < 0 || (cap > 0 && !out))
    return MIND_EINVAL;
  IlqrTuning t;
  const TnRefs own{nullptr, &t, nullptr};      // (the solver's knobs alone: any other name is rejected)
  for (int k = 0; k < n_knobs; ++k)
    if (!knob_names[k] || !tn_set(own, knob_names[k], knob_values[k])) return MIND_EINVAL;
  int maxM = 0;
  long Mtot = 0;
  for (int i = 0; i < n_trees; ++i) {
    if (n_nodes[i] <= 0) return MIND_EINVAL;
    maxM = std::max(maxM, n_nodes[i]); Mtot += n_nodes[i];
  }
  const IlqrChoice ch = il_choose(t, n_cu, n_trees, maxM, Mtot, (mode & 1) != 0, (mode & 2) != 0);
  std::vector<long long> rec = {IL_PLAN_HEADER, n_trees, ch.form, ch.G, ch.GS, ch.spec, ch.nslot, ch.grid, ch.wgs_per_tree, ch.host_out, ch.early,
                                ch.starve_followers, 0, 0, 0, 0};
  IlTables T;
  const int32_t *parent = parents;
  for (int i = 0; i < n_trees; parent += n_nodes[i], ++i) {
    const int node = il_tree_tables(parent, n_nodes[i], t.ilqr_chunk, T);
    if (node >= 0) {
      if (bad) { bad[0] = i; bad[1] = node; }
      return MIND_EINVAL;
    }
    const std::vector<int> *tabs[14] = {&T.lvl_start, &T.lvl_nodes, &T.child_start, &T.child_list, &T.seg_start, &T.seg_nodes, &T.slvl_start,
                                        &T.slvl_segs, &T.seg_rec, &T.fs_start, &T.fs_items, &T.fs_q1, &T.fs_nstart, &T.fs_nodes};
    rec.insert(rec.end(), {n_nodes[i], T.nl, T.nseg, T.nsl, T.maxls, T.nfs});
    for (const std::vector<int> *v : tabs) rec.push_back((long long)v->size());
    for (const std::vector<int> *v : tabs) rec.insert(rec.end(), v->begin(), v->end());
  }
  for (size_t i = 0; i < rec.size() && (int)i < cap; ++i) out[i] = rec[i];
  return (int)rec.size();
}
