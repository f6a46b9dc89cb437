// mind_aime_plan: ScenarioTreeGenerator.branch_aime (planners/mind/scenario_tree.py:38-58) in one call.  Included by mind_hip.hip
// (uses mind_ctx, ensure / fail / HIPCHK, mind_predict_batch and the kernels of aime_kernels.hip).
//
// Per round the device runs  predictor -> k_aime_world -> k_aime_select -> k_aime_branch  and the host reads ONE small buffer (kept
// modes, path probabilities, branch-time bits: 96 B per scene); create_nodes / decide_branch (scenario_tree.py:73-100) and everything else
// that needs no device -- the internal tree, the sharding arithmetic, the chunk size, the buffer layouts -- is in aime_book.h (AimeBook,
// pl_route, pl_chunk, RootLayout / InLayout; tests reach it through mind_debug_aime_book at the end of this file).  Here: the HIP calls, as
// stages over one PlanRun record -- pl_check, pl_root, per round pl_round_buffers / pl_round_launch (pl_round_tables behind the first
// predictor launch) / pl_round_decisions / AimeBook::round / pl_rebase_next / pl_exchange_next / pl_next_inputs, then pl_pack_results and
// pl_hand_out.  The branching nodes' observations are re-based where they are (k_aime_windows from k_aime_world's rows and the parents'
// windows, k_aime_rebase) and the next predictor call is queued before the host looks at anything else.  Every small table goes through
// page-locked staging, so no copy waits for the stream to drain.  At the end one gather kernel packs the rows get_scenario_tree
// (scenario_tree.py:208-272) attaches to the nodes of finished branches.
//
// Sharded (mind_set_exchange, include/mind_hip.h): the scenes of a round are block-distributed over the ranks; a rank runs the device
// part of the round on its block only, the decisions (96 B per scene) are all-gathered, the bookkeeping below is replayed identically on
// every rank, the rank that holds a branching node's parent scene re-bases it; of the next round's inputs only the small per-scene frames
// (28 floats: the replicated tree's node records) + LaneNet's output travel in one all-gather, a re-based scene's inputs + history windows go
// by an all-to-all from the rank that re-based it to the rank whose block of the next round holds it (MIND_XCHG_ALLTOALLV: on a full tree the
// same rank except at block boundaries; packed / unpacked by k_copy_segs; a round whose ranges coincide on every rank is skipped); the final
// rows / cost-tree entries are completed by one all-reduce over zero-filled buffers.  world == 1 runs the same code without the exchanges.
#include <chrono>
namespace {

int pl_pin(mind_ctx *c, int which, size_t bytes) {      // (declared ahead of il_solve in ilqr_host.hip)
  if (bytes <= c->pl_pin[which].cap) return MIND_OK;
  // (page-locked staging follows the device buffers' policy: small ones double from 1 MB -- hipHostFree + hipHostMalloc cost a millisecond)
  const size_t want = bytes < ((size_t)64 << 20) ? std::max<size_t>(2 * bytes, (size_t)1 << 20) : bytes + bytes / 2 + 4096;
  if (c->pl_pin[which].alloc(want) != hipSuccess) return fail(c, MIND_ENOMEM, "hipHostMalloc(%zu) failed", want);
  return MIND_OK;
}

struct CopySeg { const float *src; float *dst; long long n; };
// segment copies of the exchange packing: blockIdx.y = segment, blockIdx.x = 2048-float chunk of it
__global__ __launch_bounds__(256) void k_copy_segs(const CopySeg *__restrict__ segs) {
  const CopySeg S = segs[blockIdx.y];
  const long long i0 = (long long)blockIdx.x * 2048 + threadIdx.x;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long i = i0 + k * 256;
    if (i < S.n) S.dst[i] = S.src[i];
  }
}

int pl_exchange(mind_ctx *c, int op, void *send, void *recv, size_t bytes) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int rc = c->xfn(c->xuser, op, send, recv, (int64_t)bytes);
  if (rc) return fail(c, MIND_EHIP, "mind_aime_plan: the exchange callback failed (%d)", rc);
  c->x_collectives += 1;
  c->x_bytes += op == MIND_XCHG_ALLGATHER ? (long long)bytes * c->xw : (long long)bytes;
  return MIND_OK;
}

// all-to-all with per-pair sizes: table = [2][world] bytes this rank sends to / receives from every rank (send / recv are packed in rank order)
int pl_exchange_v(mind_ctx *c, void *send, void *recv, const int64_t *table) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int rc = c->xfn(c->xuser, MIND_XCHG_ALLTOALLV, send, recv, (int64_t)(intptr_t)table);
  if (rc) return fail(c, MIND_EHIP, "mind_aime_plan: the exchange callback failed (%d)", rc);
  c->x_collectives += 1;
  for (int r = 0; r < c->xw; ++r) c->x_bytes += (long long)table[(size_t)c->xw + r];
  return MIND_OK;
}

int pl_copy_segs(mind_ctx *c, const std::vector<CopySeg> &segs) {
  if (segs.empty()) return MIND_OK;
  long long mx = 0;
  for (const CopySeg &s : segs) mx = std::max(mx, s.n);
  if (mx == 0) return MIND_OK;
  int rc;
  if ((rc = ensure(c, c->x_seg, segs.size() * sizeof(CopySeg)))) return rc;
  if ((rc = pl_pin(c, 6, segs.size() * sizeof(CopySeg)))) return rc;      // (the previous table's copy completed: an exchange = a stream synchronisation lies between two uses)
  memcpy(c->pl_pin[6], segs.data(), segs.size() * sizeof(CopySeg));
  HIPCHK(c, hipMemcpyAsync(c->x_seg.p, c->pl_pin[6], segs.size() * sizeof(CopySeg), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_copy_segs, dim3((unsigned)((mx + 2047) / 2048), (unsigned)segs.size()), dim3(256), 0, c->stream, (const CopySeg *)c->x_seg.p);
  HIPCHK(c, hipGetLastError());
  return MIND_OK;
}

static_assert(PL_K == AIME_K && PL_OBS == RB_T, "aime_book.h restates the kernels' constants");
static_assert(sizeof(PlJob) == sizeof(AimeGather) && sizeof(PlJob) == sizeof(AimeFlat) && offsetof(PlJob, row0) == offsetof(AimeGather, row0) &&
                  offsetof(PlJob, row0) == offsetof(AimeFlat, row0) && offsetof(PlJob, n) == offsetof(AimeGather, dur) && offsetof(PlJob, n) == offsetof(AimeFlat, n) &&
                  offsetof(PlJob, dst) == offsetof(AimeGather, dst) && offsetof(PlJob, dst) == offsetof(AimeFlat, dst) && offsetof(PlJob, a) == offsetof(AimeGather, a) &&
                  offsetof(PlJob, a) == offsetof(AimeFlat, a), "JobTable holds the packing kernels' job records");

// MIND_PLAN_TRACE=1: host time stamps of a call's sections on stderr (diagnostic: where the host stands between the kernels)
struct PlTrace {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char *what) const {
    static const bool on = getenv("MIND_PLAN_TRACE") != nullptr;
    if (on) fprintf(stderr, "[plan] %8.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what);
  }
};

double pl_steady_now(void *) { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// one mind_aime_plan call: what its stages share
struct PlanRun {
  mind_ctx *c;
  const mind_aime_plan_in *in;
  mind_aime_plan_out *out;
  hipStream_t st;
  AimeBook &book;
  const int a, l, P, HZ;          // agents, lanes, target-lane points, planning horizon
  const bool raw;                 // root scene featurised on the device
  const int XW, XR;
  const bool dist;                // exchanges run (a forced one-rank group included)
  const RootLayout ro;
  const float *droot = nullptr;
  // the current round's inputs: which pl_in holds them (-1: the root upload), the windows they were re-based from
  int cur_in = -1;
  const float *prev_pos = nullptr, *prev_ang = nullptr, *prev_vel = nullptr, *cov_last_dev = nullptr;
  bool frames_pending = false;    // the frames (ROT, ORIG, TGT_PTS) of the current round's scenes are still on their way to page-locked slot 3
  int n_expanded = 0, pair_launches = 0;
  int lc_n = 0;      // the plan's pair launches pending in the launch clock's ring (their copy to the host rides behind the read-back)
  // the round in flight: its geometry, chunk size and small buffers (pl_round_buffers)
  PlGeom g = {0, 0, 0, 0, 0};
  int chunk = 1;
  bool all_small = false, tables_done = false;
  size_t bS = 0, bI = 0, bP = 0, tab_bytes = 0, n_back = 0;
  DevBuf *tabb = nullptr;
  float *d_topo = nullptr, *d_ego = nullptr, *d_sel = nullptr, *d_selp = nullptr, *h_mirror = nullptr, *d_world = nullptr;
  unsigned *d_hit = nullptr;
  // polled decisions ("dec_poll"): the word behind the mirror that the round's last kernel sets to want_gen (null: the stream is drained)
  unsigned *h_gen = nullptr, want_gen = 0;
  int round_no = 0;
  // the next round's inputs and windows (pl_rebase_next)
  int nxt = 0;
  InLayout q{0, 0, 0};
  float *d_in = nullptr, *w_pos = nullptr, *w_ang = nullptr, *w_vel = nullptr;
  // the plan's own contingency solves: wanted (asked for and there is a cost tree), begun, what beginning them returned
  bool want_solves = false, solves_tried = false;
  int solves_rc = MIND_OK;
  PlTrace TR;

  PlanRun(mind_ctx *c_, const mind_aime_plan_in *in_, mind_aime_plan_out *out_)
      : c(c_), in(in_), out(out_), st(c_->stream), book(c_->plan.book), a(in_->n_agents), l(in_->n_lanes), P(in_->n_lane_pts), HZ(in_->pred_len),
        raw(in_->raw_pos != nullptr), XW(c_->xfn ? c_->xw : 1), XR(c_->xfn ? c_->xr : 0), dist(pl_exchanges(c_->xfn != nullptr, c_->xw, c_->xforce)),
        ro(in_->n_agents, in_->n_lanes, in_->n_lane_pts, in_->raw_pos != nullptr) {}
  // the plan begins its contingency solves itself (given their inputs; not on a sharded context)
  bool solves_asked() const { return in->solve_cfg_full && in->solve_x0 && in->solve_lane && in->solve_n_lane_pts >= 2 && !dist; }
  int fail_book(const PlErr &e) const { return fail(c, MIND_ESTATE, pl_err_format(e.code), e.a0, e.a1); }
  // the stages, in the order mind_aime_plan runs them (pl_check needs no PlanRun), and the pieces they share
  int pl_root(), pl_root_raw(), pl_root_host(), pl_presize_next();
  int pl_round_buffers(int round), pl_round_launch(), pl_round_tables(), pl_round_decisions(const float *&h_dec);
  int pl_predict_chunk(int g0, int cb, float *d_cls, float *d_reg, float *d_vel, const float *&d_ctrs, const float *&d_vecs);
  int pl_rebase_next(), pl_exchange_next(int round), pl_next_inputs(), pl_pack_results(), pl_hand_out();
  void pl_begin_solves();
  int pl_side_hop(hipStream_t &rs), pl_frames_back(const float *d_fr, size_t S, hipStream_t rs);
  template <class Layout> RebaseArgs pl_rebase_args(float *base, const Layout &q, size_t s0, int l) const;
};

// Unsharded with a side stream: what feeds LaneNet / the token positions and the glue behind the predictor -- not ActorNet -- goes to the side
// stream, in front of the predictor's own side-stream work, behind what the context stream holds so far.  Else: the context stream.
int PlanRun::pl_side_hop(hipStream_t &rs) {
  rs = st;
  if (c->side && !dist) {
    if (!c->ev_root) HIPCHK(c, c->ev_root.create(hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_root, st));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_root, 0));
    rs = c->side;
  }
  return MIND_OK;
}

// the frames of S scenes come back into page-locked slot 3 (pl_round_tables waits for ev_pl)
int PlanRun::pl_frames_back(const float *d_fr, size_t S, hipStream_t rs) {
  int rc;
  if ((rc = pl_pin(c, 3, S * 28 * sizeof(float)))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->pl_pin[3], d_fr, S * 28 * sizeof(float), hipMemcpyDeviceToHost, rs));
  HIPCHK(c, hipEventRecord(c->ev_pl, rs));
  frames_pending = true;
  return MIND_OK;
}

// k_aime_rebase's arguments that follow from a layout: the outputs at scene s0 of `base` (l = 0: no lane anchors) and what every call shares
template <class Layout>
RebaseArgs PlanRun::pl_rebase_args(float *base, const Layout &q, size_t s0, int l) const {
  RebaseArgs R;
  R.a = a; R.l = l; R.n_lane = P;
  R.types = droot + ro.types; R.tlane = droot + ro.tl; R.tinfo = droot + ro.ti;
  R.time_ahead = in->time_ahead; R.min_vel = in->min_vel;
  R.actors = base + q.actors + s0 * a * 14 * 48; R.actor_ctrs = base + q.ctrs + s0 * a * 2; R.actor_vecs = base + q.vecs + s0 * a * 2;
  R.lane_ctrs = l ? base + q.lc + s0 * l * 2 : nullptr; R.lane_vecs = l ? base + q.lv + s0 * l * 2 : nullptr;
  R.tgt_nodes = base + q.tn + s0 * 160; R.tgt_rpe = base + q.tr + s0 * 20; R.frames = base + q.fr + s0 * 28;
  return R;
}

int pl_check(mind_ctx *c, const mind_aime_plan_in *in) {
  if (!c->have_weights) return fail(c, MIND_ESTATE, "weights not loaded");
  if (c->il_finish) {
    // A tree-iLQR call is pending on this context.  The solves a plan began itself write into the library's own pl_sol_* vectors and
    // staging tables, which this plan is about to resize: they are drained and dropped here (their caller gave them up -- an exception
    // between plan_start and plan_end, a planner that was reset).  A call begun by the caller (mind_ilqr_contingency_begin) writes into
    // the caller's arrays, whose lifetime the library cannot know: that one is refused.
    if (!c->il_finish_owned)
      return fail(c, MIND_ESTATE, "mind_aime_plan: a tree-iLQR call begun with mind_ilqr_contingency_begin is pending on this context (mind_ilqr_finish first)");
    (void)mind_ilqr_finish(c);
    c->pl_sol_xs.clear(); c->pl_sol_us.clear(); c->pl_sol_stw.clear(); c->pl_sol_stf.clear();
  }
  const bool raw = in->raw_pos != nullptr;
  if (in->n_agents <= 0 || in->n_lanes <= 0 || in->n_lane_pts < 12 || !in->types || !in->target_lane || !in->target_lane_info ||
      (raw ? (!in->raw_ang || !in->raw_vel || !in->raw_pad || !in->lane_pts || !in->lane_flags || !(in->travel0 >= 0.f))
           : (!in->actors || !in->actor_ctrs || !in->actor_vecs || !in->lanes || !in->lane_ctrs || !in->lane_vecs || !in->tgt_nodes ||
              !in->tgt_rpe || !in->rot || !in->orig || !in->tgt_pts || !in->hist)) || in->max_depth < 0 || in->max_rounds <= 0 || in->max_rounds > 32 || in->pred_len < 2 || in->pred_len > AIME_T)
    return fail(c, MIND_EINVAL, "mind_aime_plan: bad argument");
  if (in->script_cls && (!in->script_reg || !in->script_vel)) return fail(c, MIND_EINVAL, "mind_aime_plan: scripted modes need cls, reg and vel");
  return MIND_OK;
}

// ---- root upload (one page-locked staging buffer -> one async copy), raw: the device builds the root scene from it
int PlanRun::pl_root_raw() {
  const RootLayout &o = ro;
  const size_t OBS = RB_T;
  int rc;
  float *h = c->pl_pin[0].as<float>();
  memcpy(h + o.types, in->types, a * OBS * 7 * sizeof(float));
  memcpy(h + o.tl, in->target_lane, P * 2 * sizeof(float));
  memcpy(h + o.ti, in->target_lane_info, P * 12 * sizeof(float));
  memcpy(h + o.rpos, in->raw_pos, a * OBS * 2 * sizeof(float));
  memcpy(h + o.rang, in->raw_ang, a * OBS * sizeof(float));
  memcpy(h + o.rvel, in->raw_vel, a * OBS * 2 * sizeof(float));
  memcpy(h + o.rpad, in->raw_pad, a * OBS * sizeof(float));
  memcpy(h + o.lpts, in->lane_pts, l * 22 * sizeof(double));
  memcpy(h + o.lfl, in->lane_flags, l * 6 * sizeof(int));
  // one copy: [types .. lane flags] (the slots before `types` are produced on the device)
  if ((rc = pl_upload(c, (float *)c->pl_root.p + o.types, h + o.types, (o.total - o.types) * sizeof(float), st))) return rc;
  float *d = (float *)c->pl_root.p;
  RebaseArgs R = pl_rebase_args(d, o, 0, 0);
  R.pad_ones = 0;
  R.pos = d + o.rpos; R.ang = d + o.rang; R.vel = d + o.rvel; R.pad = d + o.rpad;
  R.lane_ctrs0 = nullptr; R.lane_vecs0 = nullptr; R.travel0 = in->travel0;
  hipLaunchKernelGGL(k_aime_rebase, dim3(1, 1 + RB_FEAT_BLOCKS(a)), dim3(RB_THREADS), 5 * a * sizeof(float), st, R);
  // The lane graph, the root's world-frame histories and the frame read-back go to the side stream: ActorNet only needs k_aime_rebase's
  // features.  "root_head": the predictor call launches them itself, behind ActorNet -- the lane graph in front of LaneNet, the histories
  // (read by k_aime_world and the next round's k_aime_windows, behind the decoder's wait for the side stream) and the read-back behind the
  // target embedding; their launches stood 25 us of host time between the re-basing and ActorNet.  Off: queued here, in front of the call
  const auto lanes = [this, d](hipStream_t rs) {
    const RootLayout &o = ro;
    hipLaunchKernelGGL(k_aime_root_lanes, dim3(l), dim3(64), 0, rs, (const double *)(d + o.lpts), (const int *)(d + o.lfl), (const float *)(d + o.fr),
                       d + o.lc, d + o.lv, d + o.lanes);
    HIPCHK(c, hipGetLastError());
    return (int)MIND_OK;
  };
  const auto hist = [this, d](hipStream_t rs) {
    const RootLayout &o = ro;
    hipLaunchKernelGGL(k_aime_root_hist, dim3(a), dim3(64), 0, rs, (const float *)(d + o.rpos), (const float *)(d + o.rang), (const float *)(d + o.rvel),
                       (const float *)(d + o.fr), (const float *)(d + o.ctrs), (const float *)(d + o.vecs), d + o.wpos, d + o.wang, d + o.wvel, d + o.cov);
    HIPCHK(c, hipGetLastError());
    return pl_frames_back(d + o.fr, 1, rs);      // the root's frame comes back while the first predictor call runs
  };
  if (c->ct.root_head && c->side && !dist) {
    c->enc_pre = lanes; c->enc_post = hist;
    return MIND_OK;
  }
  hipStream_t rs;
  if ((rc = pl_side_hop(rs)) || (rc = lanes(rs))) return rc;
  return hist(rs);
}

// ... host-featurised: everything goes up, the root's frame is the caller's
int PlanRun::pl_root_host() {
  const RootLayout &o = ro;
  const size_t OBS = RB_T;
  float *h = c->pl_pin[0].as<float>();
  memcpy(h + o.actors, in->actors, a * 14 * 48 * sizeof(float));
  memcpy(h + o.ctrs, in->actor_ctrs, a * 2 * sizeof(float));
  memcpy(h + o.vecs, in->actor_vecs, a * 2 * sizeof(float));
  memcpy(h + o.lanes, in->lanes, l * 160 * sizeof(float));
  memcpy(h + o.lc, in->lane_ctrs, l * 2 * sizeof(float));
  memcpy(h + o.lv, in->lane_vecs, l * 2 * sizeof(float));
  memcpy(h + o.tn, in->tgt_nodes, 160 * sizeof(float));
  memcpy(h + o.tr, in->tgt_rpe, 20 * sizeof(float));
  memcpy(h + o.types, in->types, a * OBS * 7 * sizeof(float));
  memcpy(h + o.tl, in->target_lane, P * 2 * sizeof(float));
  memcpy(h + o.ti, in->target_lane_info, P * 12 * sizeof(float));
  for (size_t i = 0; i < a; ++i) {
    h[o.cov + i] = in->hist[(i * OBS + OBS - 1) * 6 + 5];           // TRAJS_COV_HIST[:, -1, 0]
    for (size_t t = 0; t < OBS; ++t) {
      const float *r = in->hist + (i * OBS + t) * 6;
      h[o.wpos + (i * OBS + t) * 2] = r[0]; h[o.wpos + (i * OBS + t) * 2 + 1] = r[1];
      h[o.wvel + (i * OBS + t) * 2] = r[2]; h[o.wvel + (i * OBS + t) * 2 + 1] = r[3];
      h[o.wang + i * OBS + t] = r[4];
    }
  }
  HIPCHK(c, hipMemcpyAsync(c->pl_root.p, h, o.total * sizeof(float), hipMemcpyHostToDevice, st));
  PlScene &s = book.batch[0];
  memcpy(s.rot, in->rot, 4 * sizeof(float)); memcpy(s.orig, in->orig, 2 * sizeof(float)); memcpy(s.tgt, in->tgt_pts, 22 * sizeof(float));
  return MIND_OK;
}

int PlanRun::pl_root() {
  int rc;
  if ((rc = ensure(c, c->pl_root, ro.total * sizeof(float)))) return rc;
  if ((rc = pl_pin(c, 0, ro.total * sizeof(float)))) return rc;
  droot = (const float *)c->pl_root.p;
  if ((rc = raw ? pl_root_raw() : pl_root_host())) return rc;
  if ((rc = ensure(c, c->pl_lf, (size_t)l * 128 * sizeof(float)))) return rc;
  // the lane-distance field of the contingency solves this plan will begin: everything it depends on is known now (il_solve adopts it)
  if (solves_asked()) {
    const auto field = [this]() { return il_field_prepare(c, in->solve_cfg_full, in->solve_x0, in->solve_lane, in->solve_n_lane_pts, c->pl_copy); };
    if (c->enc_post) {      // ("root_head": behind ActorNet's launch with the rest)
      const std::function<int(hipStream_t)> hist = std::move(c->enc_post);
      c->enc_post = [hist, field](hipStream_t rs) { const int rc_ = hist(rs); return rc_ ? rc_ : field(); };
    } else if ((rc = field())) return rc;
  }
  prev_pos = droot + ro.wpos; prev_ang = droot + ro.wang; prev_vel = droot + ro.wvel;
  cov_last_dev = droot + ro.cov;
  return MIND_OK;
}

// ---- the buffers of a round.  Its scenes go through predictor -> k_aime_world -> k_aime_select -> k_aime_branch in chunks of scenes when the
//      round's edge tensor would not fit the budget (mind_set_tuning "plan_chunk_mb"): the scenes are independent, a chunk is a smaller launch
int PlanRun::pl_round_buffers(int round) {
  const int Bk = g.Bk, Bmax = g.Bmax, A = Bk * a;      // this rank's scenes of the round, their agent rows
  int rc;
  // small outputs: topo [A,6] | ego_end [Bk,6,4] | decisions laid out for Bmax scenes: sel [Bmax,6] | sel_prob [Bmax,6] | hit [Bmax,6,2]
  const size_t n_topo = ((size_t)A * 6 + 3) & ~(size_t)3, n_ego = (size_t)Bk * 24;
  n_back = (size_t)Bmax * 6 * 4;
  if ((rc = ensure(c, c->pl_small, (n_topo + n_ego + n_back) * sizeof(float)))) return rc;
  d_topo = (float *)c->pl_small.p; d_ego = d_topo + n_topo; d_sel = d_ego + n_ego; d_selp = d_sel + (size_t)Bmax * 6;
  d_hit = (unsigned *)(d_selp + (size_t)Bmax * 6);
  // unsharded: the round's last kernel writes the decisions where the host reads them (same layout as the device buffer)
  h_mirror = nullptr; h_gen = nullptr;
  round_no = round;
  if (!dist && c->ct.dec_mirror) {
    if ((rc = pl_pin(c, 2, n_back * sizeof(float) + 64))) return rc;      // (+ the generation word of the polled decisions)
    h_mirror = c->pl_pin[2].as<float>();
  }
  tabb = &c->pl_tab[round & 1];
  bS = ((size_t)Bk * sizeof(AimeScene) + 15) & ~(size_t)15; bI = ((size_t)A * sizeof(int) + 15) & ~(size_t)15;
  bP = ((size_t)Bk * sizeof(float) + 15) & ~(size_t)15;
  tab_bytes = bS + bI + bP;
  // (two table buffers, by round parity: the stream may still hold the previous round's windows kernel, which reads the index lists behind
  // that round's tables)
  if ((rc = ensure(c, *tabb, tab_bytes + 3 * (size_t)6 * Bmax * sizeof(int) + 64))) return rc;
  if ((rc = pl_pin(c, 1, tab_bytes + 3 * (size_t)6 * Bmax * sizeof(int) + 64))) return rc;
  if ((int)c->pl_world.size() <= round) c->pl_world.resize(round + 1);
  d_world = nullptr;
  chunk = pl_chunk(a + l + 1, pred_edge_pair_bytes(c->pt, c->pair_prec), c->ct.plan_chunk_mb, Bk);
  if (Bk > 0) {
    if ((rc = ensure(c, c->pl_world[round], (size_t)A * 6 * AIME_T * 6 * sizeof(float)))) return rc;
    d_world = (float *)c->pl_world[round].p;
    const int cbm = std::min(chunk, Bk);
    const size_t n_cls = ((size_t)cbm * 6 + 3) & ~(size_t)3;
    if ((rc = ensure(c, c->pl_pred, (n_cls + (size_t)cbm * a * 6 * AIME_T * 7) * sizeof(float)))) return rc;
  }
  tables_done = false;
  all_small = c->ct.tab_small && std::min(chunk, std::max(Bk, 1)) <= AIME_SMALL;
  // a round of one launch whose decisions are mirrored: its last kernel marks them complete and the host polls (pl_round_decisions).  The word
  // is cleared here, before the launch: slot 2's last writer (the previous round's kernel, the previous plan's read-back) has been waited for
  if (h_mirror && c->ct.dec_poll && Bk > 0 && chunk >= Bk) {
    if (!c->pl_cnt.p) {
      if ((rc = ensure(c, c->pl_cnt, 64))) return rc;
      HIPCHK(c, hipMemsetAsync(c->pl_cnt.p, 0, 64, st));      // (once: the block that arrives last re-arms the counter)
    }
    h_gen = (unsigned *)(h_mirror + n_back);
    if (++c->dec_gen == 0u) c->dec_gen = 1u;
    want_gen = c->dec_gen;
    __atomic_store_n(h_gen, 0u, __ATOMIC_RELEASE);
  }
  return MIND_OK;
}

// ---- the frames of the re-based scenes + the scene tables of the block: prepared BEHIND the launch of the round's first predictor call (which
//      needs neither): waiting for the frames first put a host round trip between k_aime_rebase and the predictor
int PlanRun::pl_round_tables() {
  std::vector<PlScene> &batch = book.batch;
  const int Bk = g.Bk;
  tables_done = true;
  // ---- the frames of the re-based scenes (ROT, ORIG, TGT_PTS; queued behind k_aime_rebase / the unpacking): needed by the scene tables
  if (frames_pending) {
    HIPCHK(c, hipEventSynchronize(c->ev_pl));
    const float *fr = c->pl_pin[3].as<float>();
    for (int b = 0; b < g.B; ++b) {
      memcpy(batch[b].rot, fr + (size_t)b * 28, 4 * sizeof(float));
      memcpy(batch[b].orig, fr + (size_t)b * 28 + 4, 2 * sizeof(float));
      memcpy(batch[b].tgt, fr + (size_t)b * 28 + 6, 22 * sizeof(float));
    }
    frames_pending = false;
  }
  if (Bk <= 0) return MIND_OK;
  // the scene tables of the whole block, one upload; agent rows are counted from the start of a scene's chunk
  char *h = c->pl_pin[1].as<char>();
  AimeScene *hs = (AimeScene *)h;
  int *as = (int *)(h + bS);
  float *sp = (float *)(h + bS + bI);
  for (int b = 0; b < Bk; ++b) {
    AimeScene &S = hs[b];
    const PlScene &q = batch[g.lo + b];
    const int bc = b % chunk;
    S.a0 = a * bc; S.a1 = a * (bc + 1); S.last = HZ - 1;     /* seq_len - 1 - history length */ S.cmp = q.cur_t == 0 ? 1 : q.cur_t; S.pad2 = 0.f;
    S.r00 = q.rot[0]; S.r01 = q.rot[1]; S.r10 = q.rot[2]; S.r11 = q.rot[3];
    S.ox = q.orig[0]; S.oy = q.orig[1];
    S.theta_g = atan2f(S.r10, S.r00);
    for (int i = 0; i < a; ++i) as[(size_t)b * a + i] = bc;
    sp[b] = q.prob;
  }
  if (all_small) {
    // (the glue kernels take these tables by value: AimeSmall)
  } else if (c->ct.pl_tab_side) {
    HIPCHK(c, hipMemcpyAsync(tabb->p, h, tab_bytes, hipMemcpyHostToDevice, c->pl_copy));
    HIPCHK(c, hipEventRecord(c->ev_tab, c->pl_copy));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_tab, 0));
  } else {
    HIPCHK(c, hipMemcpyAsync(tabb->p, h, tab_bytes, hipMemcpyHostToDevice, st));
  }
  return MIND_OK;
}

// the predictor call of the scenes [g0, g0 + cb) of the round, from the root upload or the current re-based input set
int PlanRun::pl_predict_chunk(int g0, int cb, float *d_cls, float *d_reg, float *d_vel, const float *&d_ctrs, const float *&d_vecs) {
  std::vector<int32_t> ao(cb + 1), lof(cb + 1);
  for (int b = 0; b <= cb; ++b) { ao[b] = a * b; lof[b] = l * b; }
  mind_scene_batch sb;
  memset(&sb, 0, sizeof(sb));
  mind_pred_out po;
  memset(&po, 0, sizeof(po));
  sb.n_scenes = cb; sb.actor_off = ao.data(); sb.lane_off = lof.data();
  if (cur_in < 0) {
    const RootLayout &o = ro;
    sb.actors = droot + o.actors; sb.lanes = droot + o.lanes; sb.actor_ctrs = d_ctrs = droot + o.ctrs; sb.actor_vecs = d_vecs = droot + o.vecs;
    sb.lane_ctrs = droot + o.lc; sb.lane_vecs = droot + o.lv; sb.tgt_nodes = droot + o.tn; sb.tgt_rpe = droot + o.tr;
    po.lane_feat = (float *)c->pl_lf.p;
  } else {
    const InLayout q(g.B, a, l);
    const float *d = (const float *)c->pl_in[cur_in].p;
    sb.actors = d + q.actors + (size_t)g0 * a * 14 * 48; sb.actor_ctrs = d_ctrs = d + q.ctrs + (size_t)g0 * a * 2; sb.actor_vecs = d_vecs = d + q.vecs + (size_t)g0 * a * 2;
    sb.lane_ctrs = d + q.lc + (size_t)g0 * l * 2; sb.lane_vecs = d + q.lv + (size_t)g0 * l * 2;
    sb.tgt_nodes = d + q.tn + (size_t)g0 * 160; sb.tgt_rpe = d + q.tr + (size_t)g0 * 20;
    sb.lane_feat = cb == 1 ? (const float *)c->pl_lf.p : (const float *)c->pl_lrep.p;
  }
  po.cls = d_cls; po.reg = d_reg; po.vel = d_vel;
  TR("round: predictor launch begins");
  const int rc = mind_predict_batch(c, &sb, &po);
  if (!rc) TR("round: predictor launched");
  return rc;
}

// ---- this rank's scenes of the round, chunk by chunk: predictor, scripted modes, world rows, pruning decisions + branch-time bits
int PlanRun::pl_round_launch() {
  const int T = AIME_T, Bk = g.Bk, Bmax = g.Bmax;
  const char *dtab = (const char *)tabb->p;
  int rc;
  for (int c0 = 0; c0 < Bk; c0 += chunk) {
    const int cb = std::min(chunk, Bk - c0), g0 = g.lo + c0, Ac = cb * a;      // scenes [g0, g0 + cb) of the round
    const size_t n_cls = ((size_t)cb * 6 + 3) & ~(size_t)3;
    float *d_cls = (float *)c->pl_pred.p, *d_reg = d_cls + n_cls, *d_vel = d_reg + (size_t)Ac * 6 * T * 5;
    const float *d_ctrs, *d_vecs;
    if ((rc = pl_predict_chunk(g0, cb, d_cls, d_reg, d_vel, d_ctrs, d_vecs))) return rc;
    if (!tables_done && (rc = pl_round_tables())) return rc;
    TR("round: tables prepared");
    n_expanded += cb;
    if (c->profiling) pair_launches += c->n_pair_launch;
    if (in->script_cls) {
      // scripted modes (benchmark hook): the forward above was the timed work, its outputs are replaced scene by scene
      const size_t nr = (size_t)a * 6 * T * 5, nv = (size_t)a * 6 * T * 2;
      hipLaunchKernelGGL(k_repeat_rows, dim3((unsigned)((6 * (size_t)cb + 255) / 256)), dim3(256), 0, st, in->script_cls, (size_t)6, cb, d_cls);
      hipLaunchKernelGGL(k_repeat_rows, dim3((unsigned)((nr * cb + 255) / 256)), dim3(256), 0, st, in->script_reg, nr, cb, d_reg);
      hipLaunchKernelGGL(k_repeat_rows, dim3((unsigned)((nv * cb + 255) / 256)), dim3(256), 0, st, in->script_vel, nv, cb, d_vel);
    }
    // prune_merge arithmetic + decisions + branch-time bits of the chunk, written at the chunk's place in the block's buffers
    const AimeScene *t_sc = (const AimeScene *)dtab + c0;
    const float *t_prob = (const float *)(dtab + bS + bI) + c0;
    float *w_c = d_world + (size_t)c0 * a * 6 * T * 6, *topo_c = d_topo + (size_t)c0 * a * 6, *ego_c = d_ego + (size_t)c0 * 24;
    float *sel_c = d_sel + (size_t)c0 * 6, *selp_c = d_selp + (size_t)c0 * 6;
    unsigned *hit_c = d_hit + (size_t)c0 * 12;
    AimeSmall sm;
    memset(&sm, 0, sizeof(sm));
    if (all_small) {
      const char *h = c->pl_pin[1].as<char>();
      memcpy(sm.s, (const AimeScene *)h + c0, (size_t)cb * sizeof(AimeScene));
      memcpy(sm.prob, (const float *)(h + bS + bI) + c0, (size_t)cb * sizeof(float));
      sm.n = cb; sm.a = a;
    }
    hipLaunchKernelGGL(k_aime_world, dim3(Ac * AIME_K), dim3(64), 0, st, t_sc, (const int *)(dtab + bS) + (size_t)c0 * a, d_reg, d_vel, d_ctrs, d_vecs,
                       cov_last_dev + (size_t)g0 * a, w_c, topo_c, ego_c, droot + ro.tl, P, sm);
    float *hs_ = h_mirror ? h_mirror + (size_t)c0 * 6 : nullptr, *hp_ = h_mirror ? h_mirror + (size_t)Bmax * 6 + (size_t)c0 * 6 : nullptr;
    unsigned *hh_ = h_mirror ? (unsigned *)(h_mirror + (size_t)Bmax * 12) + (size_t)c0 * 12 : nullptr;
    const float pf_ = in->prob_floor > 0.f ? in->prob_floor : 0.001f;
    const AimeDone dn{h_gen ? (unsigned *)c->pl_cnt.p : nullptr, h_gen, want_gen};
    if (c->ct.glue_fused) {
      // pruning decisions + branch-time bits in one launch (every block derives its scene's decisions itself)
      hipLaunchKernelGGL(k_aime_select_branch, dim3(cb * AIME_K), dim3(64), 0, st, t_sc, d_cls, t_prob, topo_c, ego_c, 1, in->dist_thres, pf_, w_c, sel_c, selp_c,
                         hit_c, hs_, hp_, hh_, sm, dn);
    } else {
      hipLaunchKernelGGL(k_aime_select, dim3(cb), dim3(64), 0, st, t_sc, d_cls, t_prob, topo_c, ego_c, 1, in->dist_thres, sel_c, selp_c, pf_, sm);
      hipLaunchKernelGGL(k_aime_branch, dim3(cb * AIME_K), dim3(64), 0, st, t_sc, sel_c, w_c, hit_c, (const float *)selp_c, hs_, hp_, hh_, sm, dn);
    }
    HIPCHK(c, hipGetLastError());
  }
  if (!tables_done && (rc = pl_round_tables())) return rc;      // (a rank without scenes in this round still needs the frames)
  return MIND_OK;
}

// ---- the round's decisions on the host: this rank's block, or (sharded) every rank's through one all-gather.  -> [ranks][Bmax x 24 floats]
int PlanRun::pl_round_decisions(const float *&h_dec) {
  int rc;
  if (dist) {
    if ((rc = ensure(c, c->x_recv, (size_t)XW * n_back * sizeof(float)))) return rc;
    if ((rc = pl_exchange(c, MIND_XCHG_ALLGATHER, d_sel, c->x_recv.p, n_back * sizeof(float)))) return rc;
    if ((rc = pl_pin(c, 2, (size_t)XW * n_back * sizeof(float)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pl_pin[2], c->x_recv.p, (size_t)XW * n_back * sizeof(float), hipMemcpyDeviceToHost, st));
  } else if (!h_mirror) {
    if ((rc = pl_pin(c, 2, n_back * sizeof(float)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->pl_pin[2], d_sel, n_back * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  TR("round: glue launched, waiting for the decisions");
  if (h_gen) {
    // what the next round needs whatever is decided, while the device works; then the word -- bounded: past the time-out (a round of many
    // scenes, a launch that failed) the stream is drained as before and the same bytes are read
    if ((rc = pl_presize_next())) return rc;
    if (!pl_wait_word(h_gen, want_gen, 0.25, pl_steady_now, nullptr, 1024)) {
      HIPCHK(c, hipStreamSynchronize(st));
      HIPCHK(c, hipMemsetAsync(c->pl_cnt.p, 0, 64, st));      // (whatever a failed launch left in the counter)
    }
  } else {
    HIPCHK(c, hipStreamSynchronize(st));
  }
  TR("round: decisions on the host");
  h_dec = c->pl_pin[2].as<float>();
  return MIND_OK;
}

// ---- the next round's inputs, windows, repeated lane features and frame staging at the largest branch set this round can produce (every kept
//      mode of every scene branches), in front of the wait for the decisions instead of behind it.  Only while that bound stays in the
//      doubling regime of ensure (64 MB): a big round's buffers are sized from its real branch set (pl_rebase_next), not from six times it.
//      (pl_lrep may be what this round's token kernels are reading: before a buffer grows the stream is drained, as it was before the old
//      place of these calls -- in the first plans of a process only)
int PlanRun::pl_presize_next() {
  if (round_no + 1 >= in->max_rounds) return MIND_OK;
  const size_t OBS = RB_T, S = (size_t)g.B * AIME_K;
  const int n = cur_in < 0 ? 0 : cur_in ^ 1;
  const size_t b_in = InLayout(S, a, l).total * sizeof(float), b_win = S * a * OBS * 5 * sizeof(float), b_rep = S * l * 128 * sizeof(float);
  if (std::max(b_in, std::max(b_win, b_rep)) >= ((size_t)64 << 20)) return MIND_OK;
  int rc;
  if (b_in > c->pl_in[n].cap || b_win > c->pl_win[n].cap || b_rep > c->pl_lrep.cap) HIPCHK(c, hipStreamSynchronize(st));
  if ((rc = ensure(c, c->pl_in[n], b_in)) || (rc = ensure(c, c->pl_win[n], b_win)) || (rc = ensure(c, c->pl_lrep, b_rep))) return rc;
  return pl_pin(c, 3, S * 28 * sizeof(float));
}

// ---- update_obser (:467-567) of the branching nodes: windows + predictor inputs of the next round, on the device; a rank re-bases the
//      children of ITS scenes (PlRound)
int PlanRun::pl_rebase_next() {
  const PlRound &r = book.rec;
  const size_t OBS = RB_T, S = r.S, s0 = r.s0;
  const int Sm = r.Sm;
  int rc;
  nxt = cur_in < 0 ? 0 : cur_in ^ 1;
  q = InLayout(S, a, l);
  if ((rc = ensure(c, c->pl_in[nxt], q.total * sizeof(float)))) return rc;
  const size_t n_wpos = S * a * OBS * 2, n_wang = S * a * OBS;
  if ((rc = ensure(c, c->pl_win[nxt], (2 * n_wpos + n_wang) * sizeof(float)))) return rc;
  w_pos = (float *)c->pl_win[nxt].p; w_ang = w_pos + n_wpos; w_vel = w_ang + n_wang;
  d_in = (float *)c->pl_in[nxt].p;
  if (Sm <= 0) return MIND_OK;
  int *hi_ = (int *)(c->pl_pin[1].as<char>() + tab_bytes);
  memcpy(hi_, r.win.data(), 3 * (size_t)Sm * sizeof(int));
  // (a small branch set: k_aime_windows reads its three ints per scene from the page-locked staging itself -- no copy in front of it)
  const bool tab_host = c->ct.tab_host_max > 0 && (size_t)Sm * a <= (size_t)c->ct.tab_host_max;
  if (!tab_host) HIPCHK(c, hipMemcpyAsync((char *)tabb->p + tab_bytes, hi_, 3 * (size_t)Sm * sizeof(int), hipMemcpyHostToDevice, st));
  const int *d_idx = tab_host ? (const int *)hi_ : (const int *)((const char *)tabb->p + tab_bytes);
  float *pos0 = w_pos + s0 * a * OBS * 2, *ang0 = w_ang + s0 * a * OBS, *vel0 = w_vel + s0 * a * OBS * 2;
  hipLaunchKernelGGL(k_aime_windows, dim3((unsigned)(Sm * a)), dim3(64), 0, st, prev_pos, prev_ang, prev_vel, (const float *)d_world, d_idx, d_idx + Sm,
                     d_idx + 2 * Sm, a, pos0, ang0, vel0, AIME_K, d_in + q.cov + s0 * a);
  RebaseArgs R = pl_rebase_args(d_in, q, s0, l);
  R.pad_ones = 1;
  R.pos = pos0; R.ang = ang0; R.vel = vel0; R.pad = nullptr;
  R.lane_ctrs0 = droot + ro.lc; R.lane_vecs0 = droot + ro.lv; R.travel0 = -1.f;
  hipLaunchKernelGGL(k_aime_rebase, dim3((unsigned)Sm, 1 + RB_FEAT_BLOCKS(a)), dim3(RB_THREADS), 5 * a * sizeof(float), st, R);
  HIPCHK(c, hipGetLastError());
  return MIND_OK;
}

// ---- sharded: the next round's inputs + windows go where they are NEEDED: scene s of the next round was re-based by the rank that predicted its
//      parent and is predicted -- and later branched from -- by the rank whose block of the next round holds it.  On a full tree the two ranges
//      coincide up to the block boundaries, so only the boundary scenes travel (all-to-all with per-pair sizes; round 4 handed every rank ALL
//      scenes: 52 MB per cfg4 round, 3.7 GB on the deepest stress tree).  What every rank does need of every scene is small: its frame (ROT / ORIG /
//      TGT_PTS, 28 floats: the replicated tree's node records) and, after the root round, LaneNet's output -- one all-gather.
int PlanRun::pl_exchange_next(int round) {
  const PlRound &r = book.rec;
  const size_t OBS = RB_T;
  float *fr_base = d_in + q.fr;
  int rc;
  struct Arr { float *base; size_t per; };
  const size_t na = a, nl = l;
  const Arr arrs[11] = {{d_in + q.actors, na * 14 * 48}, {d_in + q.ctrs, na * 2}, {d_in + q.vecs, na * 2}, {d_in + q.lc, nl * 2}, {d_in + q.lv, nl * 2}, {d_in + q.tn, 160},
                        {d_in + q.tr, 20}, {d_in + q.cov, na}, {w_pos, na * OBS * 2}, {w_ang, na * OBS}, {w_vel, na * OBS * 2}};
  std::vector<CopySeg> segs;
  // (1) all-gather: [LaneNet output (root round, from rank 0) | the frames of this rank's children, laid out for the largest child count]
  {
    int cmax = 0;
    for (int k = 0; k < XW; ++k) cmax = std::max(cmax, r.cnt_r[k]);
    const size_t n_hdr = round == 0 ? nl * 128 : 0;
    const size_t n_pay = (n_hdr + (size_t)cmax * 28 + 3) & ~(size_t)3;
    if ((rc = ensure(c, c->x_send, n_pay * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->x_recv, (size_t)XW * n_pay * sizeof(float)))) return rc;
    float *snd = (float *)c->x_send.p, *rcv = (float *)c->x_recv.p;
    if (n_hdr && XR == 0) segs.push_back({(const float *)c->pl_lf.p, snd, (long long)n_hdr});
    if (r.Sm > 0) segs.push_back({fr_base + (size_t)r.s0 * 28, snd + n_hdr, (long long)r.Sm * 28});
    if ((rc = pl_copy_segs(c, segs))) return rc;
    if ((rc = pl_exchange(c, MIND_XCHG_ALLGATHER, snd, rcv, n_pay * sizeof(float)))) return rc;
    segs.clear();
    if (n_hdr && XR != 0) segs.push_back({rcv, (float *)c->pl_lf.p, (long long)n_hdr});
    for (int k = 0; k < XW; ++k) {
      if (k == XR || r.cnt_r[k] == 0) continue;
      segs.push_back({rcv + (size_t)k * n_pay + n_hdr, fr_base + (size_t)r.s0_r[k] * 28, (long long)r.cnt_r[k] * 28});
    }
    if ((rc = pl_copy_segs(c, segs))) return rc;
  }
  // (2) all-to-all (pl_route): per pair the eleven array slices one behind the other.  Every rank computes the same table, so a round whose
  //     ranges coincide everywhere is skipped by all of them.  (A forced group -- tests, overhead measurements: mind_set_exchange(force) --
  //     also sends a rank's own scenes to itself through the transport: the same values land where they are, and the all-to-all is exercised
  //     with real data even in a one-rank RCCL group)
  size_t per_scene = 0;
  for (int k = 0; k < 11; ++k) per_scene += arrs[k].per;
  PlRoute rt;
  pl_route(r.S, XW, XR, r.cnt_r, r.s0_r, per_scene, c->xforce != 0, rt);
  if (rt.any <= 0) return MIND_OK;
  size_t n_snd = 0, n_rcv = 0;
  for (int k = 0; k < XW; ++k) { n_snd += (size_t)rt.tab[k] / sizeof(float); n_rcv += (size_t)rt.tab[(size_t)XW + k] / sizeof(float); }
  if ((rc = ensure(c, c->x_send, (n_snd + 4) * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->x_recv, (n_rcv + 4) * sizeof(float)))) return rc;
  float *snd = (float *)c->x_send.p, *rcv = (float *)c->x_recv.p;
  // the segments of one direction: the scenes [i0, i1) of every peer's range, packed in rank order
  const auto pair_segs = [&](const std::vector<int> &range, float *packed, bool unpack) {
    segs.clear();
    size_t o = 0;
    for (int k = 0; k < XW; ++k) {
      const size_t i0 = range[2 * k], n = range[2 * k + 1] - range[2 * k];
      for (int e = 0; e < 11 && n > 0; ++e) {
        float *arr = arrs[e].base + arrs[e].per * i0;
        segs.push_back(unpack ? CopySeg{packed + o, arr, (long long)(arrs[e].per * n)} : CopySeg{arr, packed + o, (long long)(arrs[e].per * n)});
        o += arrs[e].per * n;
      }
    }
  };
  pair_segs(rt.snd, snd, false);
  if ((rc = pl_copy_segs(c, segs))) return rc;
  if ((rc = pl_exchange_v(c, snd, rcv, rt.tab.data()))) return rc;
  pair_segs(rt.rcv, rcv, true);
  return pl_copy_segs(c, segs);
}

// ---- LaneNet's output repeated for this rank's scenes of the next round + the read-back of their frames; the next round's inputs become the current ones
int PlanRun::pl_next_inputs() {
  const int S = book.rec.S;
  int nlo, nhi, rc;
  pl_block(S, XR, XW, nlo, nhi);
  // (unsharded: the repeated lane features -- read by the token kernels, behind the predictor's side-stream work -- and the frames' read-back
  // go to the side stream; ActorNet follows the re-basing directly.  "round_head": the predictor call launches them itself, behind ActorNet --
  // the lane features in front of the token positions, the read-back behind the target embedding.  Off: queued here, in front of the call)
  const int n_rep = nhi - nlo;
  if (n_rep > 1 && (rc = ensure(c, c->pl_lrep, (size_t)n_rep * l * 128 * sizeof(float)))) return rc;
  const auto rep = [this, n_rep](hipStream_t rs) {
    if (n_rep > 1) {
      const size_t n = (size_t)l * 128;
      hipLaunchKernelGGL(k_repeat_rows, dim3((unsigned)((n * n_rep + 255) / 256)), dim3(256), 0, rs, (const float *)c->pl_lf.p, n, n_rep, (float *)c->pl_lrep.p);
      HIPCHK(c, hipGetLastError());
    }
    return (int)MIND_OK;
  };
  const float *d_fr = d_in + q.fr;
  const auto back = [this, d_fr, S](hipStream_t rs) { return pl_frames_back(d_fr, (size_t)S, rs); };
  if (c->ct.round_head && c->side && !dist) {
    c->enc_pre = rep; c->enc_post = back;
  } else {
    hipStream_t rs;
    if ((rc = pl_side_hop(rs)) || (rc = rep(rs)) || (rc = back(rs))) return rc;
  }
  prev_pos = w_pos; prev_ang = w_ang; prev_vel = w_vel;
  cov_last_dev = d_in + q.cov;
  cur_in = nxt;
  return MIND_OK;
}

// the contingency solves of the plan, begun by the plan itself: results stay in the library until mind_ilqr_finish_plan
void PlanRun::pl_begin_solves() {
  const size_t Mtot = (size_t)book.tree_off.back(), nt = book.tree_top.size();
  c->pl_sol_xs.resize(Mtot * 6); c->pl_sol_us.resize(Mtot * 2);
  c->pl_sol_stw.resize(nt); c->pl_sol_stf.resize(nt);
  solves_tried = true;
  solves_rc = mind_ilqr_contingency_begin_plan(c, in->solve_cfg_warm, in->solve_cfg_full, in->solve_x0, in->solve_lane, in->solve_n_lane_pts,
                                               in->solve_target_vel, c->pl_sol_xs.data(), c->pl_sol_us.data(), c->pl_sol_stw.data(), c->pl_sol_stf.data());
  c->il_finish_owned = solves_rc == MIND_OK;
}

// ---- the finished branches' rows and the flattened cost trees: one upload (both job tables), the two packing kernels, one read-back (rows |
//      flat means | flat covariances); the plan's own solves right behind k_aime_flat
int PlanRun::pl_pack_results() {
  const size_t Mtot = (size_t)book.tree_off.back(), n_rows = (size_t)book.n_rows, n_flat = Mtot * a * 3, n_res = n_rows + n_flat;
  want_solves = solves_asked() && !book.tree_top.empty();
  lc_n = lc_on(c) ? (int)c->lc.pending.size() : 0;      // (before the plan's own solves take a block)
  int rc;
  c->plan.agents = a;
  c->plan.rows_p = c->plan.fmean_p = c->plan.fcov_p = nullptr;
  c->plan.dev_fmean = c->plan.dev_fcov = nullptr;
  if (n_res > 0) {
    const JobTable &F = book.flat, &G = book.gather;
    const size_t o_g = F.bytes(), n_tab = o_g + G.bytes();
    const size_t o_rows = (n_tab + 255) & ~(size_t)255;
    if ((rc = ensure(c, c->pl_flat, o_rows + n_res * sizeof(float)))) return rc;
    if ((rc = pl_pin(c, 0, n_tab))) return rc;          // (the root upload of this plan completed rounds ago)
    char *h = c->pl_pin[0].as<char>();
    const float *world_of_round[32];
    for (size_t i = 0; i < c->pl_world.size() && i < 32; ++i) world_of_round[i] = (const float *)c->pl_world[i].p;
    F.pack(h, world_of_round);
    G.pack(h + o_g, world_of_round);
    TR("end: trees flattened on the host");
    // (few jobs: the two packing kernels read their tables from the page-locked staging themselves)
    const bool tab_host = !dist && c->ct.tab_host_max > 0 && F.job_of_block.size() + G.job_of_block.size() <= (size_t)c->ct.tab_host_max;
    if (n_tab && !tab_host) HIPCHK(c, hipMemcpyAsync(c->pl_flat.p, h, n_tab, hipMemcpyHostToDevice, st));
    char *d = tab_host ? h : (char *)c->pl_flat.p;
    float *d_rows = (float *)((char *)c->pl_flat.p + o_rows), *d_fmean = d_rows + n_rows, *d_fcov = d_fmean + Mtot * a * 2;
    if (dist) HIPCHK(c, hipMemsetAsync(d_rows, 0, n_res * sizeof(float), st));      // every entry is written by exactly one rank: the sum completes it
    if (!F.jobs.empty())
      hipLaunchKernelGGL(k_aime_flat, dim3((unsigned)F.job_of_block.size()), dim3(64), 0, st, (const AimeFlat *)d, (const int *)(d + F.off_job()),
                         (const int *)(d + F.off_agent()), (const float *const *)(d + F.off_world()), d_fmean, d_fcov);
    const auto gather = [&](hipStream_t gs) {
      if (!G.jobs.empty())
        hipLaunchKernelGGL(k_aime_gather, dim3((unsigned)G.job_of_block.size()), dim3(64), 0, gs, (const AimeGather *)(d + o_g), (const int *)(d + o_g + G.off_job()),
                           (const int *)(d + o_g + G.off_agent()), (const float *const *)(d + o_g + G.off_world()), d_rows);
    };
    if (!want_solves) gather(st);
    HIPCHK(c, hipGetLastError());
    if (dist && (rc = pl_exchange(c, MIND_XCHG_ALLREDUCE, d_rows, d_rows, n_res * sizeof(float)))) return rc;
    c->plan.dev_fmean = d_fmean; c->plan.dev_fcov = d_fcov;
    if ((rc = pl_pin(c, 2, n_res * sizeof(float)))) return rc;
    float *hp = c->pl_pin[2].as<float>();
    if (want_solves) {
      // k_ilqr right behind k_aime_flat: the cost trees' agent arrays stay where that kernel wrote them (il_solve reads them on the device)
      // and the host builds the solver's tables while it runs.  What only the CALLER wants -- the finished branches' rows (k_aime_gather) and the
      // plan's read-back (rows | flat means | sigmas: the tree objects, the candidate evaluation) -- is queued on the copy stream AFTER the
      // solves have been launched: beside k_ilqr on the device, and behind its launch on the host (the five calls stood 10 us in front of it).
      if (!c->ev_rows) HIPCHK(c, c->ev_rows.create(hipEventDisableTiming));
      HIPCHK(c, hipEventRecord(c->ev_tab, st));          // (the job tables are up, the flat arrays written)
      TR("end: flat kernel queued");
      pl_begin_solves();
      TR("end: solves begun");
      HIPCHK(c, hipStreamWaitEvent(c->pl_copy, c->ev_tab, 0));
      gather(c->pl_copy);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(hp, d_rows, n_res * sizeof(float), hipMemcpyDeviceToHost, c->pl_copy));
      if (lc_n > 0 && (rc = lc_copy_async(c, c->pl_copy, 0, lc_n))) return rc;
      HIPCHK(c, hipEventRecord(c->ev_rows, c->pl_copy));
      HIPCHK(c, hipEventSynchronize(c->ev_rows));
      TR("end: read-back on the host");
    } else {
      HIPCHK(c, hipMemcpyAsync(hp, d_rows, n_res * sizeof(float), hipMemcpyDeviceToHost, st));
      if (lc_n > 0 && (rc = lc_copy_async(c, st, 0, lc_n))) return rc;
      HIPCHK(c, hipStreamSynchronize(st));
    }
    // the plan's rows and flattened cost trees are handed out where the read-back put them (page-locked slot 2: nothing touches it before
    // the context's next plan, the lifetime mind_aime_plan_out promises); the deep stress trees return 0.9 GB here
    c->plan.rows_p = hp; c->plan.fmean_p = hp + n_rows; c->plan.fcov_p = hp + n_rows + Mtot * a * 2;
  } else {
    if (lc_n > 0 && (rc = lc_copy_async(c, st, 0, lc_n))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
  }
  return MIND_OK;
}

int PlanRun::pl_hand_out() {
  float pair_ms = 0.f;
  int rc;
  out->nodes = book.table.data(); out->n_nodes = (int)book.table.size();
  out->rows = c->plan.rows_p; out->n_row_floats = book.n_rows;
  out->n_expanded = n_expanded; out->n_rounds = book.n_rounds;
  out->root_flags = book.root_flags();
  if (c->profiling && (rc = mind_pair_events_resolve(c, &pair_ms))) return rc;      // (the plan's kernels have completed: every exit above waited for the read-back behind them)
  if (lc_on(c)) {
    // the launch clock's figure is the one handed out (with "prof_clock" 2 the events above were read too: mind_debug_launch_times)
    double ms[LC_KINDS];
    int n[LC_KINDS];
    if ((rc = lc_resolve(c, lc_n, 1u << LC_PAIR, ms, n))) return rc;
    pair_ms = (float)ms[LC_PAIR];
  }
  out->pair_ms = pair_ms; out->pair_launches = pair_launches;
  out->n_trees = (int)book.tree_top.size(); out->tree_top = book.tree_top.data(); out->tree_off = book.tree_off.data();
  out->flat_parent = book.flat_parent.data(); out->flat_prob = book.flat_prob.data();
  out->flat_mean = c->plan.fmean_p; out->flat_cov = c->plan.fcov_p;
  // ---- the contingency solves of the plan, begun here when the caller handed their inputs in (no host round trip between the plan's
  //      read-back and k_ilqr); results stay in the library until mind_ilqr_finish_plan
  if (want_solves) {
    if (!solves_tried) pl_begin_solves();
    out->solves_begun = solves_rc == MIND_OK ? 1 : 0;      // (a failed begin is not the plan's failure: the caller then solves the usual way)
  }
  TR("end: result handed out");
  return MIND_OK;
}

}  // namespace

extern "C" int mind_aime_plan(mind_ctx *c, const mind_aime_plan_in *in, mind_aime_plan_out *out) {
  if (!c || !in || !out) return MIND_EINVAL;
  int rc;
  if ((rc = pl_check(c, in))) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  PlanRun p(c, in, out);
  c->plan.agents = 0;
  c->plan.gen += 1;
  p.book.reset(in->pred_len, in->max_depth, p.a, p.XW, p.XR, p.dist);      // (the previous plan's cost trees are gone whatever happens below)
  if (!c->ev_pl) HIPCHK(c, c->ev_pl.create(hipEventDisableTiming));
  if (!c->ev_tab) HIPCHK(c, c->ev_tab.create(hipEventDisableTiming));
  if (!c->pl_copy) HIPCHK(c, c->pl_copy.create());
  struct HookGuard { mind_ctx *c; ~HookGuard() { c->enc_pre = nullptr; c->enc_post = nullptr; } } hook_guard{c};      // (they capture this call's PlanRun)
  if ((rc = p.pl_root())) return rc;
  memset(out, 0, sizeof(*out));
  p.TR.t0 = std::chrono::steady_clock::now();      // (the stamps count from here, behind the root upload)
  // profiling (bench.py's live pair-kernel durations): the predictor calls of the plan record into an event pool that is read once at
  // the end, instead of draining the stream after every call
  struct DeferGuard { mind_ctx *c; ~DeferGuard() { c->ev_defer = false; c->ev_pending.clear(); c->ev_pool_used = 0; } } defer_guard{c};
  c->ev_defer = c->profiling;
  c->ev_pending.clear(); c->ev_pool_used = 0;
  // (launch-clock records a failed call left behind are dropped, behind a drained stream)
  if (!c->lc.pending.empty() && (rc = lc_flush(c, false))) return rc;
  for (int k = 0; k < LC_KINDS; ++k) { c->lc_carry_ms[k] = 0.0; c->lc_carry_n[k] = 0; }
  for (int round = 0;; ++round) {
    PlErr e = p.book.begin_round(in->max_rounds, p.g);
    if (e) return p.fail_book(e);
    out->round_scenes[round] = p.g.Bk;
    const float *h_dec;
    if ((rc = p.pl_round_buffers(round)) || (rc = p.pl_round_launch()) || (rc = p.pl_round_decisions(h_dec))) return rc;
    if ((e = p.book.round(h_dec, p.g.Bmax))) return p.fail_book(e);
    if (p.book.rec.todo.empty()) break;
    if ((rc = p.pl_rebase_next())) return rc;
    if (p.dist && (rc = p.pl_exchange_next(round))) return rc;
    if ((rc = p.pl_next_inputs())) return rc;
  }
  p.TR("rounds done");
  const PlErr e = p.book.finish();
  if (e) return p.fail_book(e);
  if ((rc = p.pl_pack_results())) return rc;
  return p.pl_hand_out();
}

extern "C" int mind_ilqr_finish_plan(mind_ctx *c, int n_nodes, int n_trees, double *xs, double *us, mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full) {
  if (!c || !xs || !us || !stats_full) return MIND_EINVAL;
  if (!c->il_finish || !c->il_finish_owned) return fail(c, MIND_ESTATE, "mind_ilqr_finish_plan: no plan-begun tree-iLQR call is pending on this context");
  const int rc = mind_ilqr_finish(c);
  if (rc) return rc;
  // the caller sized xs / us / stats_* from ITS plan's tree table: refuse to copy another plan's results into them
  if ((size_t)n_nodes * 6 != c->pl_sol_xs.size() || (size_t)n_trees != c->pl_sol_stf.size() || (size_t)n_trees + 1 != c->plan.book.tree_off.size() ||
      c->plan.book.tree_off[(size_t)n_trees] != n_nodes)
    return fail(c, MIND_EINVAL, "mind_ilqr_finish_plan: the caller expects %d nodes in %d trees, the pending solves hold %zu in %zu", n_nodes, n_trees,
                c->pl_sol_xs.size() / 6, c->pl_sol_stf.size());
  memcpy(xs, c->pl_sol_xs.data(), c->pl_sol_xs.size() * sizeof(double));
  memcpy(us, c->pl_sol_us.data(), c->pl_sol_us.size() * sizeof(double));
  if (stats_warm) memcpy(stats_warm, c->pl_sol_stw.data(), c->pl_sol_stw.size() * sizeof(mind_ilqr_stats));
  memcpy(stats_full, c->pl_sol_stf.data(), c->pl_sol_stf.size() * sizeof(mind_ilqr_stats));
  return MIND_OK;
}


// ---- mind_aime_plan in two halves (a host thread that plans several scenes, one context each: mind_amd/pipelined.py)
extern "C" int mind_aime_plan_begin(mind_ctx *c, const mind_aime_plan_in *in) {
  if (!c || !in) return MIND_EINVAL;
  // a plan that is still RUNNING must be collected first; one that finished and was never collected (its caller gave it up) is dropped
  if (c->pa_state.load(std::memory_order_acquire) == 1) return fail(c, MIND_ESTATE, "mind_aime_plan_begin: a plan is running on this context");
  if (c->pa_thread.joinable()) c->pa_thread.join();
  c->pa_in = *in;
  memset(&c->pa_out, 0, sizeof(c->pa_out));
  c->pa_state.store(1, std::memory_order_release);
  try {
    c->pa_thread = std::thread([c] {
      c->pa_rc = mind_aime_plan(c, &c->pa_in, &c->pa_out);
      c->pa_state.store(2, std::memory_order_release);
    });
  } catch (...) {
    c->pa_state.store(0, std::memory_order_release);
    return fail(c, MIND_ESTATE, "mind_aime_plan_begin: no thread");
  }
  return MIND_OK;
}

extern "C" int mind_aime_plan_poll(mind_ctx *c) {
  if (!c) return MIND_EINVAL;
  return c->pa_state.load(std::memory_order_acquire) == 1 ? 1 : 0;
}

extern "C" int mind_aime_plan_finish(mind_ctx *c, mind_aime_plan_out *out) {
  if (!c || !out) return MIND_EINVAL;
  if (c->pa_state.load(std::memory_order_acquire) == 0) return fail(c, MIND_ESTATE, "mind_aime_plan_finish: no plan was begun");
  if (c->pa_thread.joinable()) c->pa_thread.join();
  *out = c->pa_out;
  c->pa_state.store(0, std::memory_order_release);
  return c->pa_rc;
}

extern "C" int mind_ctx_busy(mind_ctx *c) {
  if (!c) return MIND_EINVAL;
  if (c->pa_state.load(std::memory_order_acquire) == 1) return 1;
  (void)hipSetDevice(c->device);
  const hipError_t e = hipStreamQuery(c->stream);
  if (e == hipErrorNotReady) return 1;
  if (e != hipSuccess) return fail(c, MIND_EHIP, "mind_ctx_busy: %s", hipGetErrorString(e));
  return 0;
}

// pl_wait_word, the bounded wait of the polled decisions, over the caller's word and clock (clock null: the steady clock)
extern "C" int mind_debug_wait_word(const unsigned *word, unsigned want, double timeout_s, double (*clock)(void *), void *user, int spins_per_look) {
  if (!word || !(timeout_s >= 0.0) || spins_per_look <= 0) return MIND_EINVAL;
  return pl_wait_word(word, want, timeout_s, clock ? clock : pl_steady_now, user, (unsigned)spins_per_look) ? 1 : 0;
}

// AimeBook's records, pl_route's tables and pl_chunk for a stream of decision words (layout: include/mind_hip.h)
constexpr int PL_BOOK_HEADER = 16;
extern "C" int mind_debug_aime_book(int pred_len, int max_depth, int max_rounds, int n_agents, int world, int rank, int force, int n_rounds, const int *dec_len,
                                    const float *dec, int n_tokens, int bytes_per_pair, int plan_chunk_mb, int per_scene, long long *out, int cap, char *msg,
                                    int msg_cap) {
  if (pred_len < 2 || pred_len > AIME_T || max_depth < 0 || max_rounds <= 0 || max_rounds > 32 || n_agents <= 0 || world < 1 || rank < 0 || rank >= world ||
      n_rounds < 0 || (n_rounds > 0 && (!dec_len || !dec)) || n_tokens < 0 || (n_tokens > 0 && (bytes_per_pair <= 0 || plan_chunk_mb <= 0)) || per_scene < 0 ||
      cap < 0 || (cap > 0 && !out) || msg_cap < 0 || (msg_cap > 0 && !msg))
    return MIND_EINVAL;
  const bool dist = pl_exchanges(true, world, force != 0);
  const auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (long long)u; };
  AimeBook book(pred_len, max_depth, n_agents, world, rank, dist);
  std::vector<long long> rec(PL_BOOK_HEADER, 0);
  const auto put = [&rec](const auto &v) { rec.insert(rec.end(), v.begin(), v.end()); };
  PlErr e;
  PlGeom g;
  PlRoute rt;
  int rounds = 0;
  for (const float *d = dec; rounds < n_rounds; d += dec_len[rounds++]) {
    if ((e = book.begin_round(max_rounds, g))) break;
    if (dec_len[rounds] != (dist ? world : 1) * g.Bmax * 24) return MIND_EINVAL;
    if ((e = book.round(d, g.Bmax))) break;
    const PlRound &q = book.rec;
    pl_route(q.S, world, rank, q.cnt_r, q.s0_r, (size_t)per_scene, force != 0, rt);
    rec.insert(rec.end(), {g.B, g.lo, g.hi, g.Bmax, n_tokens ? pl_chunk(n_tokens, bytes_per_pair, plan_chunk_mb, g.Bk) : 0, q.S, q.s0, q.Sm, rt.any});
    put(q.todo); put(q.cnt_r); put(q.s0_r); put(q.win); put(rt.tab); put(rt.snd); put(rt.rcv);
  }
  if (!e) e = book.finish();
  if (msg_cap > 0) snprintf(msg, (size_t)msg_cap, pl_err_format(e.code), e.a0, e.a1);
  if (!e) {
    for (size_t i = 0; i < book.table.size(); ++i) {
      const mind_aime_node &n = book.table[i];
      const PlNode &m = book.nodes[i + 1];
      rec.insert(rec.end(), {n.round, n.scene, n.mode, n.parent, bits(n.prob), n.cur_t, n.end_t, n.flags, n.dur, n.row_off, m.owner, m.lscene});
    }
    for (const JobTable *t : {&book.gather, &book.flat}) {
      rec.insert(rec.end(), {(long long)t->jobs.size(), (long long)t->job_of_block.size(), (long long)t->bytes()});
      for (size_t i = 0; i < t->jobs.size(); ++i) rec.insert(rec.end(), {t->jobs[i].row0, t->jobs[i].n, t->jobs[i].dst, t->jobs[i].a, t->world[i]});
      put(t->job_of_block); put(t->agent_of_block);
    }
    put(book.tree_top); put(book.tree_off); put(book.flat_parent);
    for (float f : book.flat_prob) rec.push_back(bits(f));
  }
  const long long hdr[12] = {PL_BOOK_HEADER, e.code, e.a0, e.a1, rounds, e ? 0 : (long long)book.table.size(), e ? 0 : (long long)book.tree_top.size(),
                             e ? 0 : (long long)book.flat_parent.size(), e ? 0 : book.n_rows, book.root_flags(), dist, world};
  std::copy(hdr, hdr + 12, rec.begin());
  for (size_t i = 0; i < rec.size() && (int)i < cap; ++i) out[i] = rec[i];
  return (int)rec.size();
}
