// Host side of the clearance audit (kernels: audit_kernels.hip; geometry: box_geom.h): mind_audit_plan, mind_audit_episode and the host-only
// mind_debug_box_clearance.  Both device calls are synchronous on the context's stream and keep their scratch in c->audit_dev.
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

#define AU_PLAN_MAX_ROWS (1L << 20)       // n_cand x sum M a plan audit admits (48 MB of states)
#define AU_EPISODE_MAX_ROWS (1L << 22)    // n_ego x n_steps an episode audit admits (128 MB of ego states)
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
// a carving of the scratch arena: `n` elements of `sz` bytes, 16-byte aligned
static size_t au_take(size_t &top, size_t n, size_t sz) {
  const size_t o = (top + 15) & ~(size_t)15;
  top = o + n * sz;
  return o;
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
  long Mtot = 0, Atot = 0;
  for (int t = 0; t < n_trees; ++t) {
    const mind_cost_tree &tr = trees[t];
    if (tr.n_nodes <= 0 || tr.n_agents <= 0 || !tr.prob || (tr.n_agents > 1 && (!tr.agent_mean || !tr.agent_cov)))
      return fail(c, MIND_EINVAL, "%s: tree %d: bad n_nodes / n_agents or null prob / agent_mean / agent_cov", who, t);
    Mtot += tr.n_nodes; Atot += (long)tr.n_nodes * tr.n_agents;
    if (Mtot > AU_PLAN_MAX_ROWS || Atot > (1L << 30)) return fail(c, MIND_EINVAL, "%s: more than %ld nodes or 2^30 (node, agent) rows", who, AU_PLAN_MAX_ROWS);
    const size_t na = (size_t)tr.n_nodes * tr.n_agents;
    for (size_t i = 0; i < na; ++i) {
      if (i % tr.n_agents == 0) continue;           // (agent 0 is the ego: not read)
      const float mx = tr.agent_mean[i * 2], my = tr.agent_mean[i * 2 + 1], cv = tr.agent_cov[i];
      if (!std::isfinite(mx) || !std::isfinite(my) || !std::isfinite(cv) || cv < 0.f)
        return fail(c, MIND_EINVAL, "%s: tree %d node %ld agent %ld: non-finite mean or non-finite / negative cov", who, t, (long)(i / tr.n_agents),
                    (long)(i % tr.n_agents));
    }
  }
  if ((long)n_cand * Mtot > AU_PLAN_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d candidates x %ld nodes > %ld rows supported", who, n_cand, Mtot, AU_PLAN_MAX_ROWS);
  if (n_cand > 0 && Mtot > 0 && !xs) return fail(c, MIND_EINVAL, "%s: null xs", who);
  int rc;
  if ((rc = au_busy(c, who))) return rc;
  if (n_cand == 0 || Mtot == 0) return MIND_OK;

  // the arena: inputs (node / tree tables, prob, mean, cov, xs), then outputs
  const size_t R = (size_t)n_cand * (size_t)Mtot, RT = (size_t)n_cand * (size_t)n_trees;
  size_t top = 0;
  const size_t o_nodes = au_take(top, Mtot, sizeof(AuNode)), o_trees = au_take(top, n_trees, sizeof(AuTree)), o_prob = au_take(top, Mtot, sizeof(float)),
               o_mean = au_take(top, (size_t)Atot * 2, sizeof(float)), o_cov = au_take(top, Atot, sizeof(float));
  const size_t n_img = top;
  const size_t o_xs = au_take(top, R * 6, sizeof(double)), o_clear = au_take(top, R, sizeof(double)), o_agent = au_take(top, R, sizeof(int)),
               o_tmin = au_take(top, RT, sizeof(double)), o_tmass = au_take(top, RT, sizeof(double)), o_tnode = au_take(top, RT, sizeof(int)),
               o_tagent = au_take(top, RT, sizeof(int)), o_thits = au_take(top, RT, sizeof(int)), o_tfirst = au_take(top, RT, sizeof(int));
  std::vector<char> img(n_img, 0);
  {
    AuNode *hn = (AuNode *)(img.data() + o_nodes);
    AuTree *ht = (AuTree *)(img.data() + o_trees);
    long moff = 0, aoff = 0;
    for (int t = 0; t < n_trees; ++t) {
      const mind_cost_tree &tr = trees[t];
      const size_t M = tr.n_nodes, a = tr.n_agents;
      ht[t] = AuTree{(int)moff, tr.n_nodes};
      for (size_t i = 0; i < M; ++i) hn[moff + i] = AuNode{(int)(aoff + (long)(i * a)), tr.n_agents};
      memcpy(img.data() + o_prob + moff * sizeof(float), tr.prob, M * sizeof(float));
      if (a > 1) {
        memcpy(img.data() + o_mean + (size_t)aoff * 2 * sizeof(float), tr.agent_mean, M * a * 2 * sizeof(float));
        memcpy(img.data() + o_cov + (size_t)aoff * sizeof(float), tr.agent_cov, M * a * sizeof(float));
      }
      moff += (long)M; aoff += (long)(M * a);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->audit_dev, top))) return rc;
  char *d = (char *)c->audit_dev.p;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(d, img.data(), n_img, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(d + o_xs, xs, R * 6 * sizeof(double), hipMemcpyHostToDevice, s));
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_audit_plan, dim3((unsigned)((Mtot + AU_NB - 1) / AU_NB), (unsigned)((n_cand + AU_CB - 1) / AU_CB)), dim3(AU_CB), 0, s, eb, exo_margin,
                     (int)Mtot, n_cand, (const AuNode *)(d + o_nodes), (const float *)(d + o_mean), (const float *)(d + o_cov), (const double *)(d + o_xs),
                     (double *)(d + o_clear), (int *)(d + o_agent));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_plan_trees, dim3((unsigned)((RT + 255) / 256)), dim3(256), 0, s, (int)Mtot, n_cand, n_trees, (const AuTree *)(d + o_trees),
                     (const float *)(d + o_prob), (const double *)(d + o_clear), (const int *)(d + o_agent), (double *)(d + o_tmin), (int *)(d + o_tnode),
                     (int *)(d + o_tagent), (int *)(d + o_thits), (int *)(d + o_tfirst), (double *)(d + o_tmass));
  HIPCHK(c, hipGetLastError());
  const struct { void *h; size_t o, bytes; } back[8] = {
      {out->node_clear, o_clear, R * sizeof(double)}, {out->node_agent, o_agent, R * sizeof(int)}, {out->tree_min, o_tmin, RT * sizeof(double)},
      {out->tree_node, o_tnode, RT * sizeof(int)},    {out->tree_agent, o_tagent, RT * sizeof(int)}, {out->tree_hits, o_thits, RT * sizeof(int)},
      {out->tree_first, o_tfirst, RT * sizeof(int)},  {out->tree_mass, o_tmass, RT * sizeof(double)}};
  for (const auto &b : back)
    if (b.h) HIPCHK(c, hipMemcpyAsync(b.h, d + b.o, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return MIND_OK;
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
  size_t top = 0;
  const size_t o_ego = au_take(top, R * 4, sizeof(double)), o_exo = au_take(top, RS * 5, sizeof(double)), o_box = au_take(top, (size_t)n_tracks * 2, sizeof(double)),
               o_val = au_take(top, RS, 1), o_clear = au_take(top, R, sizeof(double)), o_track = au_take(top, R, sizeof(int)),
               o_emin = au_take(top, ne, sizeof(double)), o_estep = au_take(top, ne, sizeof(int)), o_etrack = au_take(top, ne, sizeof(int)),
               o_ehits = au_take(top, ne, sizeof(int)), o_efirst = au_take(top, ne, sizeof(int));
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->audit_dev, top))) return rc;
  char *d = (char *)c->audit_dev.p;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(d + o_ego, ego_states, R * 4 * sizeof(double), hipMemcpyHostToDevice, s));
  if (n_tracks > 1) {
    HIPCHK(c, hipMemcpyAsync(d + o_exo, exo, RS * 5 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d + o_box, boxes, (size_t)n_tracks * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d + o_val, valid, RS, hipMemcpyHostToDevice, s));
  }
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_audit_episode, dim3((unsigned)n_steps, (unsigned)((n_ego + AU_EB - 1) / AU_EB)), dim3(AU_EB), 0, s, eb, n_ego, n_steps, n_tracks,
                     (const double *)(d + o_ego), (const double *)(d + o_exo), (const unsigned char *)(d + o_val), (const double *)(d + o_box),
                     (double *)(d + o_clear), (int *)(d + o_track));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_episode_egos, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, (const double *)(d + o_clear),
                     (const int *)(d + o_track), (double *)(d + o_emin), (int *)(d + o_estep), (int *)(d + o_etrack), (int *)(d + o_ehits), (int *)(d + o_efirst));
  HIPCHK(c, hipGetLastError());
  const struct { void *h; size_t o, bytes; } back[7] = {
      {out->step_clear, o_clear, R * sizeof(double)}, {out->step_track, o_track, R * sizeof(int)},  {out->ego_min, o_emin, ne * sizeof(double)},
      {out->ego_step, o_estep, ne * sizeof(int)},     {out->ego_track, o_etrack, ne * sizeof(int)}, {out->ego_hits, o_ehits, ne * sizeof(int)},
      {out->ego_first, o_efirst, ne * sizeof(int)}};
  for (const auto &b : back)
    if (b.h) HIPCHK(c, hipMemcpyAsync(b.h, d + b.o, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return MIND_OK;
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
