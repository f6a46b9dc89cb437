// mind_loop_*: the closed loop of one scene in native code (include/mind_hip.h, "The closed loop of one scene behind ONE call").
// Host code only: the device work is what mind_aime_plan / the plan-begun contingency solves already do; this file is the part of the
// cycle the interpreter used to run between them (reference: simulator.py:51-107, agent.py:255-331, planner.py:50-145, utils.py:245-342,
// kinematics.py:22-36; this repo's Python form of the same steps: mind_amd/closed_loop.py, planners/mind/planner.py).
// mind_planner_*: the same planning cycle for a caller that keeps the simulator and pushes one observation frame at a time
// ("MINDPlanner.plan() behind ONE call").  Both objects own a mind_cycle: the windows, the scene tables, the last plan and the speculation
// state; cycle_plan / cycle_speculate / cycle_solve_speculated below are the one body of the cycle.
// Included at the end of mind_hip.hip (needs mind_ctx, fail, mind_aime_plan, mind_ilqr_finish, np_pairwise / eval_nodes).
#pragma once
#pragma STDC FP_CONTRACT OFF
#include <chrono>
#include <unordered_map>

namespace {

constexpr int LOOP_OBS = 50;        // MINDPlanner.obs_len (planner.py:14)
constexpr int LOOP_ROW = 7;         // observed, x, y, heading, vx, vy, timestep

struct LoopTrack {
  int track = 0;                    // mind_loop: index into the world's tracks
  long long key = 0;                // mind_planner: the caller's key of the track (mind_loop: the track index again)
  int slot = 6;                     // one-hot slot of the track's object type
  int count = 0, head = 0;          // rows in the window, position of the oldest
  double rows[LOOP_OBS][LOOP_ROW];
  const double *last() const { return rows[(head + count - 1) % LOOP_OBS]; }
  void push(const double *r) {
    double *dst;
    if (count < LOOP_OBS) dst = rows[(head + count++) % LOOP_OBS];
    else { dst = rows[head]; head = (head + 1) % LOOP_OBS; }            // object_states.pop(0)
    memcpy(dst, r, LOOP_ROW * sizeof(double));
  }
  void push_observed(const double *v, double timestep) {       // v: x, y, heading, vx, vy
    double row[LOOP_ROW];
    row[0] = 1.0; memcpy(row + 1, v, 5 * sizeof(double)); row[6] = timestep;
    push(row);
  }
};

}  // namespace

// what a planning cycle reads that does not change with the frame (mind_loop_desc / mind_planner_desc + the sizes of the tables below)
struct CycleParams {
  int n_lanes = 0, n_lane_pts = 0;
  double time_ahead = 0.0; float min_vel = 0.f, dist_thres = 0.f; int max_depth = 0, max_rounds = 0, pred_len = 0; float prob_floor = 0.f;
  int solve_n_lane_pts = 0; double target_vel = 0.0;
  int eval_n_lane_pts = 0, eval_lane_is_f32 = 0;
  int speculative = 0;
};

// the state of one planner's cycles: shared by mind_loop (windows fed from its tables) and mind_planner (windows fed by the caller)
struct mind_cycle {
  mind_ctx *c = nullptr;
  const char *who = "mind_loop";    // prefix of the error messages
  CycleParams p;
  // copies of the caller's scene tables
  std::vector<double> lane_pts, solve_lane, eval_lane_f64;
  std::vector<int32_t> lane_flags;
  std::vector<float> target_lane, target_lane_info, eval_lane_f32;
  mind_ilqr_cfg cfg_warm, cfg_full;
  double state[4] = {0, 0, 0, 0}, ctrl[2] = {0, 0};      // ego plant state the plan starts from, control in force / chosen by the plan
  // observation windows (MINDPlanner.agent_obs): tracks in first-appearance order, AV first
  std::vector<LoopTrack> obs;
  // per-plan scratch + the last plan
  std::vector<double> raw, eval_st, eval_ct, costs, per;
  std::vector<char> early_seen;      // candidate trees priced while the solves of the others still ran
  std::vector<float> f_pos, f_ang, f_vel, f_pad, f_types;
  std::vector<int16_t> i_typ, i_have;
  std::vector<int32_t> kept, kept_obs, slots, counts;        // kept: world track of every agent of the plan, kept_obs: its index in obs
  std::vector<long long> kept_keys;
  mind_aime_plan_out po;
  bool have_plan = false;
  long long plan_gen = -1;          // mind_ctx::plan.gen of the last plan
  std::chrono::steady_clock::time_point t_plan_end;
  // speculative warm start (TrajectoryTreeOptimizer.speculate_warm / _take_speculation, this repo's trajectory_tree.py): the warm-start fits of the
  // PREVIOUS plan's tree shapes run on a second context beside the AIME rounds; a tree whose shape recurs takes its warm-start controls from there
  mind_ctx *side = nullptr;
  hipStream_t side_stream = nullptr;
  struct Shape { std::vector<int32_t> parent; std::vector<float> prob; };
  std::vector<Shape> last_shapes, spec_shapes;
  bool spec_pending = false;
  int spec_skip = 0, spec_backoff = 4, spec_last = -1;
  std::vector<double> spec_xs, spec_us, sol_xs, sol_us, hit_ui, miss_xs, miss_us;
  std::vector<mind_ilqr_stats> spec_st, sol_stw, sol_stf, miss_stw, miss_stf;
  std::vector<float> zero_mean, zero_cov;
  long long warm_speculated = 0, warm_hits = 0;
  double plan_x0[6];
  int last_agents = 0, last_nodes = 0, best = -1, last_agents_plan = 0;
  bool sol_owned = false;           // the last plan's solve results are the cycle's own arrays (a speculated cycle), not the context's
  double aime_s = 0, ilqr_s = 0, total_s = 0;
  mind_loop_totals tot;
  mind_cycle() { memset(&po, 0, sizeof(po)); memset(&tot, 0, sizeof(tot)); }
  // a track seen for the first time joins the table behind the others; returns its index in obs
  int add_track(int track, long long key, int slot) {
    obs.emplace_back();
    obs.back().track = track; obs.back().key = key; obs.back().slot = slot;
    return (int)obs.size() - 1;
  }
};

struct mind_loop : mind_cycle {
  mind_loop_desc d;
  // copies of the caller's tables
  std::vector<double> ego_state, ego_obs, exo_obs;
  std::vector<uint8_t> exo_valid;
  std::vector<int32_t> timestep, type_slot;
  std::vector<float> ego_trig32;
  // simulator state (ClosedLoopSim)
  double sim_time = 0.0, last_trigger = -1.0;
  bool have_trigger = false, enabled = false;
  bool state_recorded = false;      // the plant state is the recorded one of row state_row (taken over in this step, not propagated yet)
  int state_row = 0;
  bool tan_valid = false;
  double tan_arg = 0.0, tan_val = 0.0;
  long long n_steps = 0, n_plans = 0, ep_steps = 0;
  std::vector<int> slot_of_track;       // world track -> index in obs, -1 = not seen yet
  bool half_step = false;
  bool planned_last = false;
};

struct mind_planner : mind_cycle {
  std::unordered_map<long long, int> slot_of_key;       // caller's key -> index in obs
  std::vector<long long> frame_keys;                    // (scratch: the duplicate check of a frame)
  std::vector<char> frame_seen;
  bool have_lanes = false, have_target = false, have_solve = false, have_eval = false;
  long long n_plans = 0, n_uploads = 0;                 // n_uploads: set_* calls that really changed a table
};

namespace {

// the cycle's fields of mind_loop_desc / mind_planner_desc
template <class Desc> void cycle_params_from(CycleParams &cp, const Desc &d) {
  cp.time_ahead = d.time_ahead; cp.min_vel = d.min_vel; cp.dist_thres = d.dist_thres; cp.max_depth = d.max_depth; cp.max_rounds = d.max_rounds;
  cp.pred_len = d.pred_len; cp.prob_floor = d.prob_floor; cp.speculative = d.speculative;
}

// the last plan's fields and the running totals of mind_loop_out / mind_planner_out
template <class Out> void cycle_fill_plan_out(const mind_cycle *L, Out *o) {
  if (L->have_plan) {
    o->n_agents = L->last_agents; o->n_trees = L->po.n_trees; o->best = L->best;
    o->n_expanded = L->po.n_expanded; o->n_rounds = L->po.n_rounds;
    o->n_traj_nodes = L->last_nodes;        // (kept by value: the plan's tables are the context's and may be another plan's by now)
    o->costs = L->costs.data();
    o->aime_s = L->aime_s; o->ilqr_s = L->ilqr_s; o->total_s = L->total_s;
  }
  o->tot = L->tot;
}

// a reset finishes a speculation that is still running on the side context (mind_loop_reset keeps have_plan, mind_planner_reset clears it: ADVICE.md item 3)
void cycle_drop_speculation(mind_cycle *L) {
  if (L->spec_pending && L->side) { (void)mind_ilqr_finish(L->side); L->spec_pending = false; }
}

// tracks not reported in this frame (seen(s, track) false): their last state again, unobserved (planner.py:58-62)
template <class Seen> void cycle_repeat_unseen(mind_cycle *L, size_t known_before, Seen seen) {
  double row[LOOP_ROW];
  for (size_t s = 1; s < known_before; ++s) {
    LoopTrack &t = L->obs[s];
    if (seen(s, t)) continue;
    memcpy(row, t.last(), sizeof(row));
    row[0] = 0.0;
    t.push(row);
  }
}

// *_last_plan: `idents` names the plan's agents the way the owner's callers do (world tracks / caller's keys)
template <class Id> int cycle_last_plan(mind_cycle *L, const std::vector<Id> &idents, mind_aime_plan_out *plan, const double **xs, const double **us,
                                        const mind_ilqr_stats **stats_warm, const mind_ilqr_stats **stats_full, const Id **agents, const float **types, double *x0) {
  if (!L->have_plan) return fail(L->c, MIND_ESTATE, "%s_last_plan: no plan is held", L->who);
  if (L->plan_gen != L->c->plan.gen) return fail(L->c, MIND_ESTATE, "%s_last_plan: the context has planned again since (another planner shares it): the plan's tables are gone", L->who);
  *plan = L->po;
  if (xs) *xs = L->sol_owned ? L->sol_xs.data() : L->c->pl_sol_xs.data();
  if (us) *us = L->sol_owned ? L->sol_us.data() : L->c->pl_sol_us.data();
  if (stats_warm) *stats_warm = L->sol_owned ? L->sol_stw.data() : L->c->pl_sol_stw.data();
  if (stats_full) *stats_full = L->sol_owned ? L->sol_stf.data() : L->c->pl_sol_stf.data();
  if (agents) *agents = idents.data();
  if (types) *types = L->f_types.data();
  if (x0) memcpy(x0, L->plan_x0, 6 * sizeof(double));
  return MIND_OK;
}

// *_export: the windows obs[first .. first + n), oldest row first, each named by the member `id` of its track
template <class M, class Id> void cycle_export_rows(const mind_cycle *L, int first, int n, M LoopTrack::*id, Id *ident, int32_t *count, double *rows) {
  for (int s = 0; s < n; ++s) {
    const LoopTrack &t = L->obs[s + first];
    ident[s] = t.*id; count[s] = t.count;
    for (int k = 0; k < t.count; ++k)
      memcpy(rows + ((size_t)s * LOOP_OBS + k) * LOOP_ROW, t.rows[(t.head + k) % LOOP_OBS], LOOP_ROW * sizeof(double));
  }
}

// one candidate of mind_eval_traj_trees at node `o` of eval_st / eval_ct: the root (x0, zero control) + the tree's m trajectory nodes
void cycle_stage_candidate(mind_cycle *L, size_t o, const double *x0, const double *xs, const double *us, int m) {
  memcpy(L->eval_st.data() + o * 6, x0, 6 * sizeof(double));
  L->eval_ct[o * 2] = 0.0; L->eval_ct[o * 2 + 1] = 0.0;
  memcpy(L->eval_st.data() + (o + 1) * 6, xs, (size_t)m * 6 * sizeof(double));
  memcpy(L->eval_ct.data() + (o + 1) * 2, us, (size_t)m * 2 * sizeof(double));
}

int loop_row(const mind_loop *L, long long n) {
  if (n < L->d.n_steps) return (int)n;
  return L->d.clamp_last ? L->d.n_steps - 1 : -1;
}

void loop_fill_out(const mind_loop *L, mind_loop_out *o) {
  memset(o, 0, sizeof(*o));
  o->planned = L->planned_last ? 1 : 0;
  o->enabled = L->enabled ? 1 : 0;
  o->n_steps = L->n_steps; o->n_plans = L->n_plans; o->episode_steps = L->ep_steps;
  o->sim_time = L->sim_time; o->last_trigger = L->have_trigger ? L->last_trigger : -1.0;
  memcpy(o->state, L->state, sizeof(o->state));
  memcpy(o->ctrl, L->ctrl, sizeof(o->ctrl));
  cycle_fill_plan_out(L, o);
}

void loop_sincos(const mind_loop *L, double x, double *sc) {
  if (L->d.sincos_fn) L->d.sincos_fn(x, sc);
  else { sc[0] = sin(x); sc[1] = cos(x); }
}

// MINDPlanner.update_observation (planner.py:50-64) on the tables' row `r`
void loop_observe(mind_loop *L, int r) {
  const int nt = L->d.n_tracks;
  const double ts = (double)L->timestep[r];
  if (L->obs.empty()) L->slot_of_track[0] = L->add_track(0, 0, L->type_slot[0]);
  const size_t known_before = L->obs.size();
  // ego: its plant state once enabled, the recording before (ClosedLoopSim._observation); to_object_state (planner.py:61-64).  The recorded
  // ego's entry -- before the take-over and at the take-over step, when the plant state IS the recorded one -- comes from the caller's table
  // (a float32 recording makes numpy evaluate it with its float32 cosine: only the driver's own code reproduces that)
  if (!L->enabled || L->state_recorded) L->obs[0].push_observed(L->ego_obs.data() + (size_t)r * 5, ts);
  else {
    const double *es = L->state;
    double sc[2];
    loop_sincos(L, es[3], sc);
    const double v[5] = {es[0], es[1], es[3], es[2] * sc[1], es[2] * sc[0]};
    L->obs[0].push_observed(v, ts);
  }
  // exo agents reported at this step, in the world's order; a track seen for the first time joins the table behind the others
  const uint8_t *val = L->exo_valid.data() + (size_t)r * nt;
  for (int i = 1; i < nt; ++i) {
    if (!val[i]) continue;
    int s = L->slot_of_track[i];
    if (s < 0) s = L->slot_of_track[i] = L->add_track(i, i, L->type_slot[i]);
    L->obs[s].push_observed(L->exo_obs.data() + ((size_t)r * nt + i) * 5, ts);
  }
  cycle_repeat_unseen(L, known_before, [&](size_t, const LoopTrack &t) { return val[t.track] != 0; });
}

// kine_propagate (common/kinematics.py:22-36) with the simulator's plant constants (agent.py:298-299)
void loop_propagate(mind_loop *L) {
  const mind_loop_desc &d = L->d;
  const double x = L->state[0], y = L->state[1], v = L->state[2], yaw = L->state[3];
  double a = L->ctrl[0], delta = L->ctrl[1];
  a = fmin(fmax(a, d.max_dec), d.max_acc);
  delta = fmin(fmax(delta, -d.max_steer), d.max_steer);
  const double dt = d.sim_step;
  double o0, o1, o2, o3;
  if (!(L->tan_valid && L->tan_arg == delta)) {        // (the control holds for the steps between two plans)
    L->tan_val = d.tan_fn ? d.tan_fn(delta) : tan(delta);
    L->tan_arg = delta; L->tan_valid = true;
  }
  const double tn = L->tan_val;
  if (L->state_recorded && d.ego_state_is_f32) {
    // the state taken over from a float32 recording is a float32 array: numpy evaluates x + v cos(yaw) dt and y + v sin(yaw) dt in float32 (its
    // float32 cosine / sine of the recorded yaw: the caller's table; the Python float dt is a weak operand), v + a dt in float64 (a is a float64
    // scalar) and yaw + v / wb tan(delta) dt with v / wb in float32 and the rest in float64 (np.tan of a float64 scalar is one); the result
    // array is float64, and so is every later step
    const float *cs = L->ego_trig32.data() + (size_t)L->state_row * 2;
    const float xf = (float)x, yf = (float)y, vf = (float)v, wf = (float)yaw, dtf = (float)dt;
    const float c0 = vf * cs[0], s0 = vf * cs[1];
    const float c1 = c0 * dtf, s1 = s0 * dtf;
    const float q0 = vf / (float)d.wheelbase;
    o0 = (double)(float)(xf + c1); o1 = (double)(float)(yf + s1); o2 = v + a * dt;
    o3 = (double)wf + ((double)q0 * tn) * dt;
  } else {
    double sc[2];
    loop_sincos(L, yaw, sc);
    o0 = x + v * sc[1] * dt; o1 = y + v * sc[0] * dt; o2 = v + a * dt; o3 = yaw + v / d.wheelbase * tn * dt;
  }
  L->state_recorded = false;
  o2 = fmin(fmax(o2, -d.max_speed), d.max_speed);
  L->state[0] = o0; L->state[1] = o1; L->state[2] = o2; L->state[3] = o3;
}

// TrajectoryTreeOptimizer.speculate_warm: the warm-start fit (lane term only: it sees the cost tree's shape, the ego state, the target lane and
// velocity -- no prediction) of every shape of the previous plan, begun on the side context; returns at once
int cycle_speculate(mind_cycle *L, const double *x0) {
  mind_ctx *c = L->c;
  const CycleParams &d = L->p;
  L->spec_pending = false;
  if (!d.speculative || L->last_shapes.empty()) return MIND_OK;
  if (L->spec_skip > 0) { L->spec_skip -= 1; L->spec_last = -1; return MIND_OK; }
  if (!L->side) {
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&L->side_stream, hipStreamNonBlocking) != hipSuccess) { L->side_stream = nullptr; return MIND_OK; }
    if (mind_ctx_create(c->device, (void *)L->side_stream, &L->side) != MIND_OK) {
      // no side context on this device: this object plans without speculation from here on (and does not create a stream per plan)
      (void)hipStreamDestroy(L->side_stream);
      L->side = nullptr; L->side_stream = nullptr; L->p.speculative = 0; L->last_shapes.clear();
      return MIND_OK;
    }
  }
  mind_ctx *sc = L->side;
  if (sc->il_finish) (void)mind_ilqr_finish(sc);
  (void)mind_set_tuning(sc, "ilqr_wgs", 1);          // (a fit beside the predictor stays on one workgroup per tree: IlqrCall background)
  L->spec_shapes = L->last_shapes;
  const int n = (int)L->spec_shapes.size();
  size_t M = 0, maxM = 0;
  for (const auto &sh : L->spec_shapes) { M += sh.parent.size(); maxM = std::max(maxM, sh.parent.size()); }
  L->zero_mean.assign(maxM * 2, 0.f); L->zero_cov.assign(maxM, 0.f);        // the warm-start cost has no agent term: one dummy agent per node
  std::vector<mind_cost_tree> trees(n);
  for (int t = 0; t < n; ++t) {
    mind_cost_tree &T = trees[t];
    memset(&T, 0, sizeof(T));
    T.n_nodes = (int)L->spec_shapes[t].parent.size(); T.parent = L->spec_shapes[t].parent.data(); T.prob = L->spec_shapes[t].prob.data();
    T.n_agents = 1; T.agent_mean = L->zero_mean.data(); T.agent_cov = L->zero_cov.data();
  }
  L->spec_xs.resize(M * 6); L->spec_us.resize(M * 2); L->spec_st.resize(n);
  IlqrCall q;
  q.cfg = &L->cfg_warm; q.trees = trees.data(); q.n_trees = n; q.x0 = x0; q.lane = L->solve_lane.data(); q.n_lane_pts = d.solve_n_lane_pts;
  q.target_vel = d.target_vel; q.xs = L->spec_xs.data(); q.us = L->spec_us.data(); q.stats = L->spec_st.data();
  q.begin_only = true;
  const int rc = il_solve(sc, q);
  if (rc != MIND_OK) return MIND_OK;                 // (the in-line path then computes -- or reports -- the same thing)
  L->spec_pending = true;
  L->warm_speculated += n;
  L->spec_last = n;
  return MIND_OK;
}

// TrajectoryTreeOptimizer.solve_batch with a speculation in flight: trees whose shape was guessed right run the full fit only (from the
// speculated warm-start controls), the others both fits on the side context beside them.  Results into L->sol_* (tree order).
int cycle_solve_speculated(mind_cycle *L, const double *x0) {
  mind_ctx *c = L->c, *sc = L->side;
  const CycleParams &d = L->p;
  const int nt = L->po.n_trees, a = L->last_agents_plan;
  const int32_t *off = L->po.tree_off;
  const int M = off[nt];
  // ---- _take_speculation
  bool have = mind_ilqr_finish(sc) == MIND_OK;
  L->spec_pending = false;
  std::vector<int> hit_of(nt, -1);
  std::vector<size_t> spec_off(L->spec_shapes.size() + 1, 0);
  for (size_t j = 0; j < L->spec_shapes.size(); ++j) spec_off[j + 1] = spec_off[j] + L->spec_shapes[j].parent.size();
  int n_hits = 0;
  for (int t = 0; t < nt && have; ++t) {
    const int m = off[t + 1] - off[t];
    for (size_t j = 0; j < L->spec_shapes.size(); ++j) {
      const auto &sh = L->spec_shapes[j];
      if ((int)sh.parent.size() == m && memcmp(sh.parent.data(), L->po.flat_parent + off[t], (size_t)m * 4) == 0 &&
          memcmp(sh.prob.data(), L->po.flat_prob + off[t], (size_t)m * 4) == 0) { hit_of[t] = (int)j; ++n_hits; break; }
    }
  }
  L->warm_hits += n_hits;
  if (L->spec_last >= 0) {
    // a speculated fit only pays when the shape recurs: after a cycle in which fewer than half of the guesses were used, skip the next
    // spec_backoff cycles (doubling after every failed probe, 4 .. 256), then probe again
    if (2 * n_hits < L->spec_last) { L->spec_skip = L->spec_backoff; L->spec_backoff = std::min(2 * L->spec_backoff, 256); }
    else L->spec_backoff = 4;
  }
  L->spec_last = -1;
  L->sol_xs.assign((size_t)M * 6, 0.0); L->sol_us.assign((size_t)M * 2, 0.0); L->sol_stw.assign(nt, mind_ilqr_stats()); L->sol_stf.assign(nt, mind_ilqr_stats());
  auto tree_of = [&](int t) {
    mind_cost_tree T;
    memset(&T, 0, sizeof(T));
    T.n_nodes = off[t + 1] - off[t]; T.parent = L->po.flat_parent + off[t]; T.prob = L->po.flat_prob + off[t];
    T.n_agents = a; T.agent_mean = L->po.flat_mean + (size_t)off[t] * a * 2; T.agent_cov = L->po.flat_cov + (size_t)off[t] * a;
    return T;
  };
  std::vector<mind_cost_tree> hits, misses;
  std::vector<int> hit_idx, miss_idx;
  for (int t = 0; t < nt; ++t) { if (hit_of[t] >= 0) { hit_idx.push_back(t); hits.push_back(tree_of(t)); } else { miss_idx.push_back(t); misses.push_back(tree_of(t)); } }
  int rc = MIND_OK;
  size_t Mm = 0, Mh = 0;
  for (const auto &T : misses) Mm += T.n_nodes;
  for (const auto &T : hits) Mh += T.n_nodes;
  bool miss_on_side = false;
  if (!misses.empty()) {          // both fits, as without speculation: beside the hits' full fits when there are any
    L->miss_xs.resize(Mm * 6); L->miss_us.resize(Mm * 2); L->miss_stw.resize(misses.size()); L->miss_stf.resize(misses.size());
    if (!hits.empty()) {
      (void)mind_set_tuning(sc, "ilqr_wgs", c->it.ilqr_wgs);
      rc = mind_ilqr_contingency_begin(sc, &L->cfg_warm, &L->cfg_full, misses.data(), (int)misses.size(), x0, L->solve_lane.data(), d.solve_n_lane_pts, d.target_vel,
                                       L->miss_xs.data(), L->miss_us.data(), L->miss_stw.data(), L->miss_stf.data());
      if (rc) return fail(c, rc, "%s: %s", L->who, sc->err.c_str());
      miss_on_side = true;
    } else {
      if ((rc = mind_ilqr_contingency(c, &L->cfg_warm, &L->cfg_full, misses.data(), (int)misses.size(), x0, L->solve_lane.data(), d.solve_n_lane_pts, d.target_vel,
                                      L->miss_xs.data(), L->miss_us.data(), L->miss_stw.data(), L->miss_stf.data())))
        return rc;
    }
  }
  if (!hits.empty()) {            // warm-start controls are there already: full fit only
    L->hit_ui.resize(Mh * 2);
    size_t o = 0;
    for (int t : hit_idx) {
      const int m = off[t + 1] - off[t];
      memcpy(L->hit_ui.data() + o * 2, L->spec_us.data() + spec_off[hit_of[t]] * 2, (size_t)m * 2 * sizeof(double));
      o += m;
    }
    std::vector<double> hx(Mh * 6), hu(Mh * 2);
    std::vector<mind_ilqr_stats> hs(hits.size());
    if ((rc = mind_ilqr_solve_trees(c, &L->cfg_full, hits.data(), (int)hits.size(), x0, L->solve_lane.data(), d.solve_n_lane_pts, d.target_vel, 1, L->hit_ui.data(),
                                    hx.data(), hu.data(), hs.data()))) {
      if (miss_on_side) (void)mind_ilqr_finish(sc);
      return rc;
    }
    o = 0;
    for (size_t k = 0; k < hit_idx.size(); ++k) {
      const int t = hit_idx[k], m = off[t + 1] - off[t];
      memcpy(L->sol_xs.data() + (size_t)off[t] * 6, hx.data() + o * 6, (size_t)m * 6 * sizeof(double));
      memcpy(L->sol_us.data() + (size_t)off[t] * 2, hu.data() + o * 2, (size_t)m * 2 * sizeof(double));
      L->sol_stw[t] = L->spec_st[hit_of[t]]; L->sol_stf[t] = hs[k];
      o += m;
    }
  }
  if (miss_on_side && (rc = mind_ilqr_finish(sc))) return fail(c, rc, "%s: %s", L->who, sc->err.c_str());
  size_t o = 0;
  for (size_t k = 0; k < miss_idx.size(); ++k) {
    const int t = miss_idx[k], m = off[t + 1] - off[t];
    memcpy(L->sol_xs.data() + (size_t)off[t] * 6, L->miss_xs.data() + o * 6, (size_t)m * 6 * sizeof(double));
    memcpy(L->sol_us.data() + (size_t)off[t] * 2, L->miss_us.data() + o * 2, (size_t)m * 2 * sizeof(double));
    L->sol_stw[t] = L->miss_stw[k]; L->sol_stf[t] = L->miss_stf[k];
    o += m;
  }
  return MIND_OK;
}

// MINDPlanner.plan (planner.py:66-145) on the windows L->obs, from the ego state L->state and the control in force L->ctrl; the chosen control
// replaces L->ctrl
int cycle_plan(mind_cycle *L) {
  mind_ctx *c = L->c;
  const CycleParams &d = L->p;
  const auto t0 = std::chrono::steady_clock::now();
  // MIND_LOOP_TRACE=1: host time stamps of the cycle's sections on stderr (diagnostic, as MIND_PLAN_TRACE inside the plan)
  static const bool loop_trace = getenv("MIND_LOOP_TRACE") != nullptr;
  auto TRL = [&](const char *what) {
    if (loop_trace) fprintf(stderr, "[loop] %8.1f us  %s\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what);
  };
  if (loop_trace && L->have_plan) fprintf(stderr, "[loop] %8.1f us since the last plan's end (evaluation excluded: steps, observation)\n",
                                          std::chrono::duration<double, std::micro>(t0 - L->t_plan_end).count());
  // ---- get_agent_trajectories (utils.py:245-342): AV first, tracks whose last state is unobserved are dropped, windows left-padded
  L->kept.clear(); L->kept_keys.clear(); L->kept_obs.clear(); L->slots.clear();
  for (size_t s = 0; s < L->obs.size(); ++s) {
    const LoopTrack &t = L->obs[s];
    if (t.last()[0] == 0.0) continue;
    L->kept.push_back(t.track); L->kept_keys.push_back(t.key); L->kept_obs.push_back((int32_t)s);
    L->slots.push_back(t.slot);
  }
  const int a = (int)L->kept.size(), T = LOOP_OBS;
  L->raw.assign((size_t)a * T * 6, 0.0);
  for (int i = 0; i < a; ++i) {
    const LoopTrack &t = L->obs[L->kept_obs[i]];
    for (int k = 0; k < t.count; ++k)
      memcpy(L->raw.data() + ((size_t)i * T + (T - t.count + k)) * 6, t.rows[(t.head + k) % LOOP_OBS], 6 * sizeof(double));
  }
  L->f_pos.resize((size_t)a * T * 2); L->f_ang.resize((size_t)a * T); L->f_vel.resize((size_t)a * T * 2);
  L->i_typ.resize((size_t)a * T * 7); L->i_have.resize((size_t)a * T);
  int rc = mind_fill_tracks(L->raw.data(), a, T, L->slots.data(), L->f_pos.data(), L->f_ang.data(), L->f_vel.data(), L->i_typ.data(), L->i_have.data());
  if (rc) return fail(c, rc, "%s: mind_fill_tracks failed", L->who);
  TRL("tracks filled");
  L->f_pad.resize((size_t)a * T); L->f_types.resize((size_t)a * T * 7);
  for (size_t i = 0; i < L->f_pad.size(); ++i) L->f_pad[i] = (float)L->i_have[i];
  for (size_t i = 0; i < L->f_types.size(); ++i) L->f_types[i] = (float)L->i_typ[i];
  // ---- mind_aime_plan, device-built root, the contingency solves begun behind it (scenario_tree.py:38-58, planner.py:174-178)
  mind_aime_plan_in pi;
  memset(&pi, 0, sizeof(pi));
  pi.n_agents = a; pi.n_lanes = d.n_lanes; pi.n_lane_pts = d.n_lane_pts;
  pi.raw_pos = L->f_pos.data(); pi.raw_ang = L->f_ang.data(); pi.raw_vel = L->f_vel.data(); pi.raw_pad = L->f_pad.data();
  pi.types = L->f_types.data();
  pi.target_lane = L->target_lane.data(); pi.target_lane_info = L->target_lane_info.data();
  pi.lane_pts = L->lane_pts.data(); pi.lane_flags = L->lane_flags.data();
  const double cur_vel = L->state[2];
  pi.travel0 = (float)((cur_vel >= (double)d.min_vel ? cur_vel : (double)d.min_vel) * d.time_ahead);      // F32(max(cur_vel, 0.5) * tar_time_ahead)
  pi.time_ahead = (float)d.time_ahead; pi.min_vel = d.min_vel; pi.dist_thres = d.dist_thres;
  pi.max_depth = d.max_depth; pi.max_rounds = d.max_rounds; pi.pred_len = d.pred_len; pi.prob_floor = d.prob_floor;
  double *x0 = L->plan_x0;
  x0[0] = L->state[0]; x0[1] = L->state[1]; x0[2] = L->state[2]; x0[3] = L->state[3]; x0[4] = L->ctrl[0]; x0[5] = L->ctrl[1];
  // warm-start fits of the previous plan's tree shapes start now, beside the predictor; with one in flight the plan does not begin the
  // solves itself (TrajectoryTreeOptimizer.plan_solve_args returns None then)
  if ((rc = cycle_speculate(L, x0))) return rc;
  if (!L->spec_pending) {
    pi.solve_cfg_warm = &L->cfg_warm; pi.solve_cfg_full = &L->cfg_full;
    pi.solve_x0 = x0; pi.solve_lane = L->solve_lane.data(); pi.solve_n_lane_pts = d.solve_n_lane_pts; pi.solve_target_vel = d.target_vel;
  }
  L->have_plan = false;
  TRL("plan call begins");
  rc = mind_aime_plan(c, &pi, &L->po);
  if (rc) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  TRL("plan returned (solves begun)");
  const int nt = L->po.n_trees;
  if (nt <= 0) return fail(c, MIND_ESTATE, "%s: the plan returned no scenario tree", L->who);
  const int32_t *off = L->po.tree_off;
  const int M = off[nt];
  bool early_done = false;        // the candidates were priced while the solves ran (below)
  const double *xs, *us;
  const mind_ilqr_stats *stw, *stf;
  L->last_agents_plan = a;
  if (L->spec_pending) {
    if ((rc = cycle_solve_speculated(L, x0))) return rc;
    xs = L->sol_xs.data(); us = L->sol_us.data(); stw = L->sol_stw.data(); stf = L->sol_stf.data();
    L->sol_owned = true;
  } else {
    if (!L->po.solves_begun) return fail(c, MIND_ESTATE, "%s: the plan could not begin its contingency solves (%s)", L->who, c->err.c_str());
    // ---- collect the solves (mind_ilqr_finish_plan without the copy: the results stay in the context until its next plan)
    if (!c->il_finish || !c->il_finish_owned) return fail(c, MIND_ESTATE, "%s: no plan-begun tree-iLQR call is pending", L->who);
    // ---- a launch of small trees writes every tree's results to the host and marks it when they are complete: price the candidates as they
    //      arrive (evaluate_traj_tree of one tree is independent of the others), beside the trees the device is still solving -- only the
    //      last one's evaluation stays between the kernel's end and the chosen control
    const mind_ctx::IlEarly E = c->il_early;
    if (c->ct.early_eval && E.done && E.n_trees == nt && E.nodes == (long)M) {
      L->costs.assign(nt, 0.0);
      L->early_seen.assign(nt, 0);
      const void *elane_e = d.eval_lane_is_f32 ? (const void *)L->eval_lane_f32.data() : (const void *)L->eval_lane_f64.data();
      int left = nt;
      const auto te0 = std::chrono::steady_clock::now();
      unsigned spins = 0;
      while (left > 0) {
        bool any = false;
        for (int t = 0; t < nt; ++t) {
          if (L->early_seen[t] || __atomic_load_n((const unsigned *)&E.done[t], __ATOMIC_ACQUIRE) != E.gen) continue;
          const int m = off[t + 1] - off[t];
          L->eval_st.resize((size_t)(m + 1) * 6); L->eval_ct.resize((size_t)(m + 1) * 2);
          cycle_stage_candidate(L, 0, x0, E.xs + (size_t)off[t] * 6, E.us + (size_t)off[t] * 2, m);
          const int32_t cnt1 = m + 1;
          if ((rc = mind_eval_traj_trees(L->eval_st.data(), L->eval_ct.data(), &cnt1, 1, elane_e, d.eval_lane_is_f32, d.eval_n_lane_pts, d.target_vel, &L->costs[t])))
            return fail(c, rc, "%s: mind_eval_traj_trees failed", L->who);
          L->early_seen[t] = 1; --left; any = true;
        }
        if (!any && (++spins & 0x3ffu) == 0u &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - te0).count() > 0.25) break;      // (never hang on a word: the usual path below)
      }
      early_done = left == 0;
    }
    if ((rc = mind_ilqr_finish(c))) return rc;
    if ((size_t)M * 6 != c->pl_sol_xs.size() || (size_t)nt != c->pl_sol_stf.size()) return fail(c, MIND_ESTATE, "%s: the solves' results do not fit the plan", L->who);
    xs = c->pl_sol_xs.data(); us = c->pl_sol_us.data(); stw = c->pl_sol_stw.data(); stf = c->pl_sol_stf.data();
    L->sol_owned = false;
  }
  const auto t2 = std::chrono::steady_clock::now();
  TRL("solves collected");
  if (d.speculative) {           // the shapes the next cycle speculates on (_last_structs)
    L->last_shapes.resize(nt);
    for (int t = 0; t < nt; ++t) {
      L->last_shapes[t].parent.assign(L->po.flat_parent + off[t], L->po.flat_parent + off[t + 1]);
      L->last_shapes[t].prob.assign(L->po.flat_prob + off[t], L->po.flat_prob + off[t + 1]);
    }
  }
  // ---- evaluate_traj_tree of every candidate (planner.py:180-198): the tree's nodes = the root (x0, zero control) + its trajectory nodes
  L->counts.resize(nt);
  if (early_done) { for (int t = 0; t < nt; ++t) L->counts[t] = off[t + 1] - off[t] + 1; }
  else {
  L->eval_st.resize((size_t)(M + nt) * 6); L->eval_ct.resize((size_t)(M + nt) * 2); L->costs.resize(nt);
  size_t o = 0;
  for (int t = 0; t < nt; ++t) {
    const int m = off[t + 1] - off[t];
    cycle_stage_candidate(L, o, x0, xs + (size_t)off[t] * 6, us + (size_t)off[t] * 2, m);
    L->counts[t] = m + 1;
    o += (size_t)m + 1;
  }
  const void *elane = d.eval_lane_is_f32 ? (const void *)L->eval_lane_f32.data() : (const void *)L->eval_lane_f64.data();
  if ((rc = mind_eval_traj_trees(L->eval_st.data(), L->eval_ct.data(), L->counts.data(), nt, elane, d.eval_lane_is_f32, d.eval_n_lane_pts, d.target_vel, L->costs.data())))
    return fail(c, rc, "%s: mind_eval_traj_trees failed", L->who);
  }
  // ---- the reference's strict `<` scan (planner.py:131-136): the first minimum, a NaN never wins
  int best = -1;
  double min_cost = INFINITY;
  for (int t = 0; t < nt; ++t)
    if (L->costs[t] < min_cost) { min_cost = L->costs[t]; best = t; }
  if (best < 0) return fail(c, MIND_ESTATE, "%s: no candidate tree has a finite cost", L->who);
  // first control: (a, delta) of the state of the root's first child (planner.py:138-141, Q15)
  int first = -1;
  for (int k = off[best]; k < off[best + 1]; ++k)
    if (L->po.flat_parent[k] == -1) { first = k; break; }
  if (first < 0) return fail(c, MIND_ESTATE, "%s: the chosen tree has no root child", L->who);
  L->ctrl[0] = xs[(size_t)first * 6 + 4]; L->ctrl[1] = xs[(size_t)first * 6 + 5];
  L->best = best; L->last_agents = a; L->last_nodes = M; L->have_plan = true; L->plan_gen = c->plan.gen;
  // accounting (TrajectoryTreeOptimizer.counters, MINDPlanner.timing_sum; bench.py's live kernel durations when profiling is on)
  mind_loop_totals &S = L->tot;
  for (int t = 0; t < nt; ++t) {
    const long long m = off[t + 1] - off[t], iw = stw[t].iterations, jf = stf[t].iterations;
    S.iterations += iw + jf; S.node_iterations += m * (iw + jf); S.node_iterations_exo += m * jf * a;
  }
  S.warm_speculated = L->warm_speculated; S.warm_hits = L->warm_hits;
  S.plans += 1; S.expansions += L->po.n_expanded; S.scen_trees += nt; S.rounds += L->po.n_rounds;
  const double N = (double)(a + d.n_lanes + 1);
  S.scene_n2 += (double)L->po.n_expanded * N * N; S.scene_n_a1 += (double)L->po.n_expanded * N * (double)(a + 1);
  if (c->profiling) {
    S.pair_ms += L->po.pair_ms; S.pair_launches += L->po.pair_launches;
    if (c->ilqr_ms > 0.f) {
      S.ilqr_ms += c->ilqr_ms; S.ilqr_launches += 1; S.ilqr_trees += c->ilqr_trees; S.ilqr_workgroups_per_tree = c->ilqr_multi;
      for (int q = 0; q < 9; ++q) S.ilqr_prof[q] += c->il_prof[q];
      S.ilqr_node_steps += c->il_prof[2] * c->il_prof[1];
    }
  }
  const auto t3 = std::chrono::steady_clock::now();
  TRL("evaluated, control chosen");
  L->t_plan_end = t3;
  L->aime_s = std::chrono::duration<double>(t1 - t0).count();
  L->ilqr_s = std::chrono::duration<double>(t2 - t1).count();
  L->total_s = std::chrono::duration<double>(t3 - t0).count();
  S.aime_s += L->aime_s; S.ilqr_s += L->ilqr_s; S.total_s += L->total_s;
  return MIND_OK;
}

// ClosedLoopSim.step: returns MIND_OK, *planned set
int loop_step(mind_loop *L) {
  mind_ctx *c = L->c;
  const mind_loop_desc &d = L->d;
  L->planned_last = false;
  const int r = loop_row(L, L->ep_steps);
  if (r < 0) return fail(c, MIND_EINVAL, "mind_loop: the scene tables end at step %d (episode step %lld)", d.n_steps, L->ep_steps);
  if (L->half_step) return fail(c, MIND_ESTATE, "mind_loop: the plan of the last step failed after its observation update: take the loop over (mind_loop_export) or reset it");
  {
    if (L->sim_time >= d.enable_time && !L->enabled) {            // check_enable: take over from the recording
      L->enabled = true;
      memcpy(L->state, L->ego_state.data() + (size_t)r * 4, 4 * sizeof(double));
      L->state_recorded = true; L->state_row = r;
      L->ctrl[0] = 0.0; L->ctrl[1] = 0.0;
    }
    if (!L->have_trigger || (L->sim_time - L->last_trigger) >= d.plan_step) {
      L->have_trigger = true; L->last_trigger = L->sim_time;
      loop_observe(L, r);
      if (L->enabled) {
        const int rc = cycle_plan(L);
        if (rc) {
          // the observation update of this step is done and must not be repeated: a caller that takes the loop over finishes the step itself
          L->half_step = true;
          return rc;
        }
        L->n_plans += 1;
        L->planned_last = true;
      }
    }
  }
  if (L->enabled) loop_propagate(L);
  L->sim_time += d.sim_step;
  L->n_steps += 1; L->ep_steps += 1;
  return MIND_OK;
}

}  // namespace

extern "C" int mind_loop_reset(mind_loop *L);
extern "C" int mind_loop_create(mind_ctx *c, const mind_loop_desc *d, mind_loop **out) {
  if (!c || !d || !out) return MIND_EINVAL;
  if (!c->have_weights) return fail(c, MIND_ESTATE, "weights not loaded");
  if (d->n_tracks <= 0 || d->n_steps <= 0 || !d->ego_state || !d->ego_obs || (d->ego_state_is_f32 && !d->ego_trig32) || !d->exo_obs || !d->exo_valid || !d->timestep || !d->type_slot || !(d->sim_step > 0.0) ||
      !(d->plan_step > 0.0) || !(d->wheelbase > 0.0) || d->n_lanes <= 0 || !d->lane_pts || !d->lane_flags || d->n_lane_pts < 12 || !d->target_lane ||
      !d->target_lane_info || !d->cfg_warm || !d->cfg_full || d->solve_n_lane_pts < 2 || !d->solve_lane || d->eval_n_lane_pts < 2 || !d->eval_lane ||
      d->max_rounds <= 0 || d->max_rounds > 32 || d->pred_len < 2 || d->pred_len > 60)
    return fail(c, MIND_EINVAL, "mind_loop_create: bad argument");
  mind_loop *L = new (std::nothrow) mind_loop();
  if (!L) return fail(c, MIND_ENOMEM, "mind_loop_create: out of memory");
  L->c = c; L->d = *d;
  CycleParams &cp = L->p;
  cycle_params_from(cp, *d);
  cp.n_lanes = d->n_lanes; cp.n_lane_pts = d->n_lane_pts;
  cp.solve_n_lane_pts = d->solve_n_lane_pts; cp.target_vel = d->target_vel;
  cp.eval_n_lane_pts = d->eval_n_lane_pts; cp.eval_lane_is_f32 = d->eval_lane_is_f32;
  const size_t S = (size_t)d->n_steps, nt = (size_t)d->n_tracks;
  L->ego_state.assign(d->ego_state, d->ego_state + S * 4);
  L->ego_obs.assign(d->ego_obs, d->ego_obs + S * 5);
  if (d->ego_trig32) L->ego_trig32.assign(d->ego_trig32, d->ego_trig32 + S * 2);
  L->exo_obs.assign(d->exo_obs, d->exo_obs + S * nt * 5);
  L->exo_valid.assign(d->exo_valid, d->exo_valid + S * nt);
  L->timestep.assign(d->timestep, d->timestep + S);
  L->type_slot.assign(d->type_slot, d->type_slot + nt);
  L->lane_pts.assign(d->lane_pts, d->lane_pts + (size_t)d->n_lanes * 22);
  L->lane_flags.assign(d->lane_flags, d->lane_flags + (size_t)d->n_lanes * 6);
  L->target_lane.assign(d->target_lane, d->target_lane + (size_t)d->n_lane_pts * 2);
  L->target_lane_info.assign(d->target_lane_info, d->target_lane_info + (size_t)d->n_lane_pts * 12);
  L->solve_lane.assign(d->solve_lane, d->solve_lane + (size_t)d->solve_n_lane_pts * 2);
  if (d->eval_lane_is_f32) L->eval_lane_f32.assign((const float *)d->eval_lane, (const float *)d->eval_lane + (size_t)d->eval_n_lane_pts * 2);
  else L->eval_lane_f64.assign((const double *)d->eval_lane, (const double *)d->eval_lane + (size_t)d->eval_n_lane_pts * 2);
  L->cfg_warm = *d->cfg_warm; L->cfg_full = *d->cfg_full;
  // (the descriptor's pointers are not used after this call)
  L->d.ego_state = nullptr; L->d.ego_obs = nullptr; L->d.ego_trig32 = nullptr; L->d.exo_obs = nullptr; L->d.exo_valid = nullptr; L->d.timestep = nullptr; L->d.type_slot = nullptr; L->d.lane_pts = nullptr;
  L->d.lane_flags = nullptr; L->d.target_lane = nullptr; L->d.target_lane_info = nullptr; L->d.cfg_warm = nullptr; L->d.cfg_full = nullptr;
  L->d.solve_lane = nullptr; L->d.eval_lane = nullptr;
  L->slot_of_track.assign(nt, -1);
  (void)mind_loop_reset(L);
  *out = L;
  return MIND_OK;
}

static void cycle_release(mind_cycle *L) {
  if (L && L->side) {
    (void)mind_ctx_destroy(L->side);
    if (L->side_stream) (void)hipStreamDestroy(L->side_stream);
    L->side = nullptr; L->side_stream = nullptr;
  }
}

extern "C" int mind_loop_destroy(mind_loop *L) {
  cycle_release(L);
  delete L;
  return MIND_OK;
}

extern "C" int mind_loop_reset(mind_loop *L) {
  if (!L) return MIND_EINVAL;
  L->sim_time = 0.0; L->have_trigger = false; L->last_trigger = -1.0; L->enabled = false; L->half_step = false;
  memcpy(L->state, L->ego_state.data(), 4 * sizeof(double));        // world.agent_state(0, 0.0)
  L->state_recorded = false; L->tan_valid = false;
  cycle_drop_speculation(L);
  L->ctrl[0] = 0.0; L->ctrl[1] = 0.0;
  L->ep_steps = 0;
  L->obs.clear();
  std::fill(L->slot_of_track.begin(), L->slot_of_track.end(), -1);
  L->planned_last = false;
  return MIND_OK;
}

extern "C" int mind_loop_advance(mind_loop *L, int until_plans, double until_time, long long max_steps, mind_loop_out *out) {
  if (!L || !out || max_steps < 0) return MIND_EINVAL;
  if (L->c->xfn) return fail(L->c, MIND_ESTATE, "mind_loop_advance: the context is sharded (mind_set_exchange): the native loop plans on one GPU");
  int done = 0, rc = MIND_OK;
  bool planned_any = false;
  for (long long s = 0; s < max_steps; ++s) {
    if (until_time >= 0.0 && !(L->sim_time < until_time - 1e-9)) break;
    if ((rc = loop_step(L))) break;
    if (L->planned_last) {
      planned_any = true;
      if (until_plans > 0 && ++done >= until_plans) break;
    }
  }
  L->planned_last = planned_any;
  loop_fill_out(L, out);
  return rc;
}

extern "C" int mind_loop_state(mind_loop *L, mind_loop_out *out) {
  if (!L || !out) return MIND_EINVAL;
  loop_fill_out(L, out);
  return MIND_OK;
}

extern "C" int mind_loop_last_plan(mind_loop *L, mind_aime_plan_out *plan, const double **xs, const double **us, const mind_ilqr_stats **stats_warm,
                                   const mind_ilqr_stats **stats_full, const int32_t **agent_tracks, const float **types, double *x0) {
  if (!L || !plan) return MIND_EINVAL;
  return cycle_last_plan(L, L->kept, plan, xs, us, stats_warm, stats_full, agent_tracks, types, x0);
}

extern "C" int mind_loop_export(mind_loop *L, int cap, int *n, int32_t *track, int32_t *count, double *rows) {
  if (!L || !n) return MIND_EINVAL;
  *n = (int)L->obs.size();
  if (*n > cap || !track || !count || !rows) return MIND_EINVAL;
  cycle_export_rows(L, 0, *n, &LoopTrack::track, track, count, rows);
  return MIND_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// mind_planner_*: MINDPlanner.update_observation / plan (planner.py:50-145) of a caller that keeps the simulator itself
// ---------------------------------------------------------------------------------------------------------------------------------------
namespace {

void planner_fill_out(const mind_planner *P, mind_planner_out *o) {
  memset(o, 0, sizeof(*o));
  o->n_plans = P->n_plans;
  if (P->have_plan) memcpy(o->ctrl, P->ctrl, sizeof(o->ctrl));
  cycle_fill_plan_out(P, o);
}

// copies a table when it differs from the planner's copy; returns whether it did
template <class T> bool planner_take(std::vector<T> &dst, const T *src, size_t n) {
  if (dst.size() == n && (n == 0 || memcmp(dst.data(), src, n * sizeof(T)) == 0)) return false;
  dst.assign(src, src + n);
  return true;
}

}  // namespace

extern "C" int mind_planner_reset(mind_planner *P);
extern "C" int mind_planner_create(mind_ctx *c, const mind_planner_desc *d, mind_planner **out) {
  if (!d || !out) return MIND_EINVAL;
  if (c && !c->have_weights) return fail(c, MIND_ESTATE, "weights not loaded");
  if (!d->cfg_warm || !d->cfg_full || d->max_rounds <= 0 || d->max_rounds > 32 || d->pred_len < 2 || d->pred_len > 60 || d->ego_type_slot < 0 || d->ego_type_slot > 6)
    return fail(c, MIND_EINVAL, "mind_planner_create: bad argument");
  mind_planner *P = new (std::nothrow) mind_planner();
  if (!P) return fail(c, MIND_ENOMEM, "mind_planner_create: out of memory");
  P->c = c; P->who = "mind_planner";
  cycle_params_from(P->p, *d);
  P->cfg_warm = *d->cfg_warm; P->cfg_full = *d->cfg_full;
  P->add_track(0, MIND_PLANNER_EGO_KEY, d->ego_type_slot);      // the ego's window: always the first track
  *out = P;
  return MIND_OK;
}

extern "C" int mind_planner_destroy(mind_planner *P) {
  cycle_release(P);
  delete P;
  return MIND_OK;
}

extern "C" int mind_planner_reset(mind_planner *P) {
  if (!P) return MIND_EINVAL;
  cycle_drop_speculation(P);
  const int ego_slot = P->obs.empty() ? 6 : P->obs[0].slot;
  P->obs.clear();
  P->add_track(0, MIND_PLANNER_EGO_KEY, ego_slot);
  P->slot_of_key.clear();
  P->have_plan = false;                       // (the last plan belongs to the episode that ended)
  return MIND_OK;
}

extern "C" int mind_planner_observe(mind_planner *P, int timestep, const double *ego, int n, const long long *track_key, const int32_t *type_slot, const double *rows) {
  if (!P || !ego || n < 0 || (n > 0 && (!track_key || !type_slot || !rows))) return P ? fail(P->c, MIND_EINVAL, "mind_planner_observe: bad argument") : MIND_EINVAL;
  // nothing is changed by a frame that is refused
  P->frame_keys.assign(track_key, track_key + n);
  std::sort(P->frame_keys.begin(), P->frame_keys.end());
  for (int i = 0; i < n; ++i) {
    if (P->frame_keys[i] == MIND_PLANNER_EGO_KEY) return fail(P->c, MIND_EINVAL, "mind_planner_observe: MIND_PLANNER_EGO_KEY names the ego's own track");
    if (i > 0 && P->frame_keys[i] == P->frame_keys[i - 1]) return fail(P->c, MIND_EINVAL, "mind_planner_observe: track key %lld twice in one frame", P->frame_keys[i]);
    if (type_slot[i] < 0 || type_slot[i] > 6) return fail(P->c, MIND_EINVAL, "mind_planner_observe: type slot %d of track %d", (int)type_slot[i], i);
  }
  const size_t known_before = P->obs.size();
  P->obs[0].push_observed(ego, (double)timestep);
  P->frame_seen.assign(known_before, 0);
  // agents reported in this frame, in the caller's order
  for (int i = 0; i < n; ++i) {
    int s;
    auto it = P->slot_of_key.find(track_key[i]);
    if (it == P->slot_of_key.end()) {
      s = P->add_track((int)P->obs.size(), track_key[i], type_slot[i]);
      P->slot_of_key.emplace(track_key[i], s);
    } else {
      s = it->second;
      P->frame_seen[s] = 1;
    }
    P->obs[s].push_observed(rows + (size_t)i * 5, (double)timestep);
  }
  cycle_repeat_unseen(P, known_before, [&](size_t s, const LoopTrack &) { return P->frame_seen[s] != 0; });
  return MIND_OK;
}

extern "C" int mind_planner_set_lanes(mind_planner *P, int n_lanes, const double *lane_pts, const int32_t *lane_flags) {
  if (!P) return MIND_EINVAL;
  if (!P->c) return MIND_ESTATE;
  if (n_lanes <= 0 || !lane_pts || !lane_flags) return fail(P->c, MIND_EINVAL, "mind_planner_set_lanes: bad argument");
  bool ch = planner_take(P->lane_pts, lane_pts, (size_t)n_lanes * 22);
  ch = planner_take(P->lane_flags, lane_flags, (size_t)n_lanes * 6) || ch;
  P->p.n_lanes = n_lanes; P->have_lanes = true; P->n_uploads += ch;
  return MIND_OK;
}

extern "C" int mind_planner_set_target_lane(mind_planner *P, int n, const float *lane, const float *info) {
  if (!P) return MIND_EINVAL;
  if (!P->c) return MIND_ESTATE;
  if (!lane || !info) return fail(P->c, MIND_EINVAL, "mind_planner_set_target_lane: bad argument");
  if (n < 12) return fail(P->c, MIND_EINVAL, "mind_planner_set_target_lane: a target lane of %d points (the plan needs 12)", n);
  bool ch = planner_take(P->target_lane, lane, (size_t)n * 2);
  ch = planner_take(P->target_lane_info, info, (size_t)n * 12) || ch;
  P->p.n_lane_pts = n; P->have_target = true; P->n_uploads += ch;
  return MIND_OK;
}

extern "C" int mind_planner_set_solve_lane(mind_planner *P, int n, const double *lane, double target_vel) {
  if (!P) return MIND_EINVAL;
  if (!P->c) return MIND_ESTATE;
  if (n < 2 || !lane) return fail(P->c, MIND_EINVAL, "mind_planner_set_solve_lane: bad argument");
  const bool ch = planner_take(P->solve_lane, lane, (size_t)n * 2);
  P->p.solve_n_lane_pts = n; P->p.target_vel = target_vel; P->have_solve = true; P->n_uploads += ch;
  return MIND_OK;
}

extern "C" int mind_planner_set_eval_lane(mind_planner *P, int n, const void *lane, int is_f32) {
  if (!P) return MIND_EINVAL;
  if (!P->c) return MIND_ESTATE;
  if (n < 2 || !lane) return fail(P->c, MIND_EINVAL, "mind_planner_set_eval_lane: bad argument");
  bool ch;
  if (is_f32) { ch = planner_take(P->eval_lane_f32, (const float *)lane, (size_t)n * 2); P->eval_lane_f64.clear(); }
  else { ch = planner_take(P->eval_lane_f64, (const double *)lane, (size_t)n * 2); P->eval_lane_f32.clear(); }
  P->p.eval_n_lane_pts = n; P->p.eval_lane_is_f32 = is_f32 ? 1 : 0; P->have_eval = true; P->n_uploads += ch;
  return MIND_OK;
}

extern "C" int mind_planner_plan(mind_planner *P, const double *state, const double *ctrl, mind_planner_out *out) {
  if (!P || !state || !ctrl || !out) return MIND_EINVAL;
  if (!P->c) return MIND_ESTATE;
  mind_ctx *c = P->c;
  if (c->xfn) return fail(c, MIND_ESTATE, "mind_planner_plan: the context is sharded (mind_set_exchange): the native cycle plans on one GPU");
  if (P->obs[0].count == 0) return fail(c, MIND_ESTATE, "mind_planner_plan: no observation yet (mind_planner_observe)");
  if (!P->have_lanes) return fail(c, MIND_ESTATE, "mind_planner_plan: the lane tables are not set (mind_planner_set_lanes)");
  if (!P->have_target || !P->have_solve || !P->have_eval)
    return fail(c, MIND_ESTATE, "mind_planner_plan: the target lane is not set (mind_planner_set_target_lane / _set_solve_lane / _set_eval_lane)");
  memcpy(P->state, state, 4 * sizeof(double));
  memcpy(P->ctrl, ctrl, 2 * sizeof(double));
  const int rc = cycle_plan(P);
  if (rc == MIND_OK) P->n_plans += 1;
  planner_fill_out(P, out);
  return rc;
}

extern "C" int mind_planner_last_plan(mind_planner *P, mind_aime_plan_out *plan, const double **xs, const double **us, const mind_ilqr_stats **stats_warm,
                                      const mind_ilqr_stats **stats_full, const long long **agent_keys, const float **types, double *x0) {
  if (!P || !plan) return MIND_EINVAL;
  if (!P->c) return MIND_ESTATE;
  return cycle_last_plan(P, P->kept_keys, plan, xs, us, stats_warm, stats_full, agent_keys, types, x0);
}

extern "C" int mind_planner_export(mind_planner *P, int cap, int *n, long long *key, int32_t *count, double *rows) {
  if (!P || !n) return MIND_EINVAL;
  const int first = P->obs[0].count ? 0 : 1;      // (the ego's window exists from creation on: it is a track once it has a frame)
  *n = (int)P->obs.size() - first;
  if (*n > cap || (*n > 0 && (!key || !count || !rows))) return MIND_EINVAL;
  cycle_export_rows(P, first, *n, &LoopTrack::key, key, count, rows);
  return MIND_OK;
}
