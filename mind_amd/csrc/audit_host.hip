// Host side of the clearance audit (kernels: audit_kernels.hip; geometry: box_geom.h): mind_audit_plan, mind_audit_episode and the host-only
// mind_debug_box_clearance -- and the scaffold the five synchronous "upload, launch, read back" entries share (these two, mind_forecast_score,
// mind_audit_road_plan, mind_audit_road_episode): the arena's head, upload and tail over audit_arena.h, and the cost trees of a plan audit.
// Included by mind_hip.hip behind loop.hip.
#pragma clang fp contract(off)

// mind_trig.h once more, as plain host functions (the text the C oracle compiles): mind_debug_box_clearance with trig == NULL runs the
// kernels' own sin / cos on the CPU
namespace au_host {
#pragma push_macro("__HIPCC__")
#pragma push_macro("MT_FN")
#pragma push_macro("MT_ALL_ZERO")
#undef __HIPCC__
#undef MIND_TRIG_H
#undef MT_FN
#undef MT_ALL_ZERO
#include "mind_trig.h"
#pragma pop_macro("MT_ALL_ZERO")
#pragma pop_macro("MT_FN")
#pragma pop_macro("__HIPCC__")
}  // namespace au_host

#define AU_PLAN_MAX_ROWS (1L << 20)       // n_cand x sum M a plan audit admits, clearance or road (48 MB of states)
#define AU_EPISODE_MAX_ROWS (1L << 22)    // n_ego x n_steps an episode audit admits, clearance or road (128 MB of ego states)
#define AU_SCENE_MAX_ROWS (1L << 24)      // n_steps x n_tracks of the replayed scene

static bool au_fin(double v) { return std::isfinite(v); }
static bool au_box_ok(const mind_audit_box *b) {
  return b && au_fin(b->length) && au_fin(b->width) && au_fin(b->center_offset) && b->length >= 0.0 && b->width >= 0.0;
}
static int au_busy(mind_ctx *c, const char *who) {
  if (c->pa_state.load(std::memory_order_acquire) == 1) return fail(c, MIND_ESTATE, "%s: a plan is running on this context", who);
  if (c->il_finish) return fail(c, MIND_ESTATE, "%s: a tree-iLQR call begun on this context has not been finished (mind_ilqr_finish)", who);
  return MIND_OK;
}

// ---- the arena on the device.  A call carves its fields, uploads every input a kernel will read and reads back only what it wrote: nothing
// in c->audit_dev outlives the call that put it there
// head: the context's device, room for the whole arena -> its base
static int ar_begin(mind_ctx *c, const Arena &ar, char **d) {
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->audit_dev, ar.top))) return rc;
  *d = (char *)c->audit_dev.p;
  return MIND_OK;
}
template <class T>
static int ar_put(mind_ctx *c, char *d, const ArField<T> &f, const T *src) {
  HIPCHK(c, hipMemcpyAsync(f.at(d), src, f.bytes(), hipMemcpyHostToDevice, c->stream));
  return MIND_OK;
}
// tail: copy back every field whose host pointer is non-null, then synchronise
static int ar_finish(mind_ctx *c, const char *d, std::initializer_list<ArBack> back) {
  for (const ArBack &b : back)
    if (b.h) HIPCHK(c, hipMemcpyAsync(b.h, d + b.off, b.bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MIND_OK;
}

// the cost trees of a plan audit, clearance or road: the rules both read (n_nodes, prob, the two row caps), then the AuTree table and the
// probabilities, carved from `ar` and filled into the image `img` (which then spans the arena so far)
struct AuPlanTrees { ArField<AuTree> trees; ArField<float> prob; long Mtot = 0; };
static int au_plan_trees(mind_ctx *c, const char *who, const mind_cost_tree *trees, int n_trees, int n_cand, Arena &ar, std::vector<char> &img, AuPlanTrees &pt) {
  for (int t = 0; t < n_trees; ++t) {
    if (trees[t].n_nodes <= 0 || !trees[t].prob) return fail(c, MIND_EINVAL, "%s: tree %d: bad n_nodes or null prob", who, t);
    pt.Mtot += trees[t].n_nodes;
    if (pt.Mtot > AU_PLAN_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: more than %ld nodes", who, AU_PLAN_MAX_ROWS);
  }
  if ((long)n_cand * pt.Mtot > AU_PLAN_MAX_ROWS)
    return fail(c, MIND_EINVAL, "%s: %d candidates x %ld nodes > %ld rows supported", who, n_cand, pt.Mtot, AU_PLAN_MAX_ROWS);
  pt.trees = ar.take<AuTree>(n_trees);
  pt.prob = ar.take<float>(pt.Mtot);
  img.resize(ar.top, 0);
  long moff = 0;
  for (int t = 0; t < n_trees; ++t) {
    pt.trees.at(img.data())[t] = AuTree{(int)moff, trees[t].n_nodes};
    std::copy_n(trees[t].prob, trees[t].n_nodes, pt.prob.at(img.data()) + moff);
    moff += trees[t].n_nodes;
  }
  return MIND_OK;
}

extern "C" int mind_audit_plan(mind_ctx *c, const mind_audit_box *ego, double exo_margin, const mind_cost_tree *trees, int n_trees, int n_cand,
                               const double *xs, const mind_audit_plan_out *out) {
  const char *who = "mind_audit_plan";
  if (!c) return MIND_EINVAL;
  if (!ego || !out || n_trees < 0 || n_cand < 0 || (n_trees > 0 && !trees)) return fail(c, MIND_EINVAL, "%s: null ego / trees / out or a negative count", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  if (!au_fin(exo_margin) || exo_margin < 0.0) return fail(c, MIND_EINVAL, "%s: exo_margin = %g, a finite value >= 0 is needed", who, exo_margin);
  if (!out->node_clear && !out->node_agent && !out->tree_min && !out->tree_node && !out->tree_agent && !out->tree_hits && !out->tree_first && !out->tree_mass)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  int rc;
  Arena ar;
  std::vector<char> img;
  AuPlanTrees pt;
  if ((rc = au_plan_trees(c, who, trees, n_trees, n_cand, ar, img, pt))) return rc;
  const long Mtot = pt.Mtot;
  long Atot = 0;
  for (int t = 0; t < n_trees; ++t) {
    const mind_cost_tree &tr = trees[t];
    if (tr.n_agents <= 0 || (tr.n_agents > 1 && (!tr.agent_mean || !tr.agent_cov)))
      return fail(c, MIND_EINVAL, "%s: tree %d: bad n_agents or null agent_mean / agent_cov", who, t);
    Atot += (long)tr.n_nodes * tr.n_agents;
    if (Atot > (1L << 30)) return fail(c, MIND_EINVAL, "%s: more than 2^30 (node, agent) rows", who);
    const size_t na = (size_t)tr.n_nodes * tr.n_agents;
    for (size_t i = 0; i < na; ++i) {
      if (i % tr.n_agents == 0) continue;           // (agent 0 is the ego: not read)
      const float mx = tr.agent_mean[i * 2], my = tr.agent_mean[i * 2 + 1], cv = tr.agent_cov[i];
      if (!std::isfinite(mx) || !std::isfinite(my) || !std::isfinite(cv) || cv < 0.f)
        return fail(c, MIND_EINVAL, "%s: tree %d node %ld agent %ld: non-finite mean or non-finite / negative cov", who, t, (long)(i / tr.n_agents),
                    (long)(i % tr.n_agents));
    }
  }
  if (n_cand > 0 && Mtot > 0 && !xs) return fail(c, MIND_EINVAL, "%s: null xs", who);
  if ((rc = au_busy(c, who))) return rc;
  if (n_cand == 0 || Mtot == 0) return MIND_OK;

  // the arena: the image (tree table, prob, node table, mean, cov), xs, then the outputs.  A tree without exo agents (n_agents == 1) leaves
  // its mean / cov rows of the image zero: k_audit_plan reads no agent of such a node
  const size_t R = (size_t)n_cand * (size_t)Mtot, RT = (size_t)n_cand * (size_t)n_trees;
  const auto f_nodes = ar.take<AuNode>(Mtot);
  const auto f_mean = ar.take<float>((size_t)Atot * 2), f_cov = ar.take<float>(Atot);
  img.resize(ar.top, 0);
  const auto f_xs = ar.take<double>(R * 6), f_clear = ar.take<double>(R);
  const auto f_agent = ar.take<int>(R);
  const auto f_tmin = ar.take<double>(RT), f_tmass = ar.take<double>(RT);
  const auto f_tnode = ar.take<int>(RT), f_tagent = ar.take<int>(RT), f_thits = ar.take<int>(RT), f_tfirst = ar.take<int>(RT);
  {
    long moff = 0, aoff = 0;
    for (int t = 0; t < n_trees; ++t) {
      const mind_cost_tree &tr = trees[t];
      const size_t M = tr.n_nodes, a = tr.n_agents;
      for (size_t i = 0; i < M; ++i) f_nodes.at(img.data())[moff + i] = AuNode{(int)(aoff + (long)(i * a)), tr.n_agents};
      if (a > 1) {
        std::copy_n(tr.agent_mean, M * a * 2, f_mean.at(img.data()) + aoff * 2);
        std::copy_n(tr.agent_cov, M * a, f_cov.at(img.data()) + aoff);
      }
      moff += (long)M; aoff += (long)(M * a);
    }
  }
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(d, img.data(), img.size(), hipMemcpyHostToDevice, s));
  if ((rc = ar_put(c, d, f_xs, xs))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_audit_plan, dim3((unsigned)((Mtot + AU_NB - 1) / AU_NB), (unsigned)((n_cand + AU_CB - 1) / AU_CB)), dim3(AU_CB), 0, s, eb, exo_margin,
                     (int)Mtot, n_cand, f_nodes.at(d), f_mean.at(d), f_cov.at(d), f_xs.at(d), f_clear.at(d), f_agent.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_plan_trees, dim3((unsigned)((RT + 255) / 256)), dim3(256), 0, s, (int)Mtot, n_cand, n_trees, pt.trees.at(d), pt.prob.at(d),
                     f_clear.at(d), f_agent.at(d), f_tmin.at(d), f_tnode.at(d), f_tagent.at(d), f_thits.at(d), f_tfirst.at(d), f_tmass.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->node_clear, f_clear}, {out->node_agent, f_agent}, {out->tree_min, f_tmin}, {out->tree_node, f_tnode},
                          {out->tree_agent, f_tagent}, {out->tree_hits, f_thits}, {out->tree_first, f_tfirst}, {out->tree_mass, f_tmass}});
}

extern "C" int mind_audit_episode(mind_ctx *c, const mind_audit_box *ego, int n_ego, int n_steps, int n_tracks, const double *ego_states, const double *exo,
                                  const uint8_t *valid, const double *boxes, const mind_audit_episode_out *out) {
  const char *who = "mind_audit_episode";
  if (!c) return MIND_EINVAL;
  if (!ego || !out || n_ego < 0 || n_steps < 0 || n_tracks < 1) return fail(c, MIND_EINVAL, "%s: null ego / out, a negative count or no track row", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  if (!out->step_clear && !out->step_track && !out->ego_min && !out->ego_step && !out->ego_track && !out->ego_hits && !out->ego_first)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  const size_t R = (size_t)n_ego * (size_t)n_steps, RS = (size_t)n_steps * (size_t)n_tracks;
  if ((long)R > AU_EPISODE_MAX_ROWS || n_ego > 65535 * AU_EB) return fail(c, MIND_EINVAL, "%s: %d egos x %d steps > %ld rows supported", who, n_ego, n_steps, AU_EPISODE_MAX_ROWS);
  if ((long)RS > AU_SCENE_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d steps x %d tracks > %ld rows supported", who, n_steps, n_tracks, AU_SCENE_MAX_ROWS);
  if (R > 0 && (!ego_states || (n_tracks > 1 && (!exo || !valid || !boxes)))) return fail(c, MIND_EINVAL, "%s: null ego_states / exo / valid / boxes", who);
  if (R > 0) {
    for (int j = 1; j < n_tracks; ++j)
      if (!au_fin(boxes[j * 2]) || !au_fin(boxes[j * 2 + 1]) || boxes[j * 2] < 0.0 || boxes[j * 2 + 1] < 0.0)
        return fail(c, MIND_EINVAL, "%s: track %d: non-finite or negative box dimension", who, j);
    for (size_t i = 0; i < R; ++i)
      if (!au_fin(ego_states[i * 4]) || !au_fin(ego_states[i * 4 + 1]) || !au_fin(ego_states[i * 4 + 3]))
        return fail(c, MIND_EINVAL, "%s: ego %ld step %ld: non-finite state", who, (long)(i / n_steps), (long)(i % n_steps));
    for (size_t i = 0; i < RS; ++i)
      if (i % n_tracks != 0 && valid[i] && (!au_fin(exo[i * 5]) || !au_fin(exo[i * 5 + 1]) || !au_fin(exo[i * 5 + 2])))
        return fail(c, MIND_EINVAL, "%s: step %ld track %ld: valid but not finite", who, (long)(i / n_tracks), (long)(i % n_tracks));
  }
  int rc;
  if ((rc = au_busy(c, who))) return rc;
  if (R == 0) return MIND_OK;

  const size_t ne = (size_t)n_ego;
  Arena ar;
  const auto f_ego = ar.take<double>(R * 4), f_exo = ar.take<double>(RS * 5), f_box = ar.take<double>((size_t)n_tracks * 2);
  const auto f_val = ar.take<uint8_t>(RS);
  const auto f_clear = ar.take<double>(R);
  const auto f_track = ar.take<int>(R);
  const auto f_emin = ar.take<double>(ne);
  const auto f_estep = ar.take<int>(ne), f_etrack = ar.take<int>(ne), f_ehits = ar.take<int>(ne), f_efirst = ar.take<int>(ne);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  if ((rc = ar_put(c, d, f_ego, ego_states))) return rc;
  // without a track beside the ego's row the scene is not uploaded: k_audit_episode's loop over the tracks 1..n-1 reads none of it
  if (n_tracks > 1 && ((rc = ar_put(c, d, f_exo, exo)) || (rc = ar_put(c, d, f_box, boxes)) || (rc = ar_put(c, d, f_val, valid)))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_audit_episode, dim3((unsigned)n_steps, (unsigned)((n_ego + AU_EB - 1) / AU_EB)), dim3(AU_EB), 0, s, eb, n_ego, n_steps, n_tracks,
                     f_ego.at(d), f_exo.at(d), f_val.at(d), f_box.at(d), f_clear.at(d), f_track.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_episode_egos<false>, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, 0.0, f_clear.at(d), f_track.at(d),
                     f_emin.at(d), f_estep.at(d), f_etrack.at(d), f_ehits.at(d), f_efirst.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->step_clear, f_clear}, {out->step_track, f_track}, {out->ego_min, f_emin}, {out->ego_step, f_estep},
                          {out->ego_track, f_etrack}, {out->ego_hits, f_ehits}, {out->ego_first, f_efirst}});
}

extern "C" int mind_debug_box_clearance(int kind, int n, const double *a, const double *b, const double *trig, double *out) {
  if ((kind != 0 && kind != 1) || n < 0 || (n > 0 && (!a || !b || !out))) return MIND_EINVAL;
  for (int i = 0; i < n; ++i) {
    const double *A = a + (size_t)i * 5, *B = b + (size_t)i * 5;
    double ca, sa, cb = 1.0, sb = 0.0;
    if (trig) {
      ca = trig[(size_t)i * 4]; sa = trig[(size_t)i * 4 + 1]; cb = trig[(size_t)i * 4 + 2]; sb = trig[(size_t)i * 4 + 3];
    } else {
      au_host::mind_sincos(A[2], &sa, &ca);
      if (kind == 1) au_host::mind_sincos(B[2], &sb, &cb);
    }
    const double dx = B[0] - A[0], dy = B[1] - A[1];
    out[i] = kind == 0 ? bg_point_rect(dx, dy, ca, sa, A[3], A[4]) - B[2] : bg_rect_rect(dx, dy, ca, sa, A[3], A[4], cb, sb, B[3], B[4]);
  }
  return MIND_OK;
}
