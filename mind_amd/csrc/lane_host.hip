// Host side of the lane audit (kernels: lane_kernels.hip; geometry: lane_geom.h): mind_audit_lane_plan, mind_audit_lane_episode and the
// host-only mind_debug_lane_project.  Both device calls are synchronous on the context's stream and run on the scaffold of audit_host.hip.
// Included by mind_hip.hip behind ttc_host.hip (au_host::mind_sincos, au_fin, au_box_ok, au_busy, au_plan_trees, ar_*: audit_host.hip;
// RD_MAX_VERTS: road_host.hip).
#pragma clang fp contract(off)

#define LG_MAX_LANES (1 << 16)            // lanes of a map

// The form of k_lane_boxes when the caller leaves it to the library (cfg.form == 0) -- the ONE place that decides it.
// Thread per box (1) launches ceil(rows / 256) workgroups whose threads each walk all V vertices one after the other: its time is the
// latency of that walk for as long as those workgroups leave the device empty.  One wavefront per box (2) launches `rows` wavefronts that
// each stage the map once more and evaluate V / 64 segments per lane: no long walk, but work that grows with every row.
// Measured against the demo_1 lanes (21 lanes, 1 395 vertices; profiles/lane_rate.json -- whole calls: upload, kernels, read-back, median of
// 20): the auditor's 1 x 546 rows take 0.56 ms in (2) against 0.97 ms in (1); (2) stays ahead at 64 x 546 = 34 944 rows (1.16 against
// 1.39 ms) and at 512 candidates x 70 nodes = 35 840 rows (0.95 against 1.19 ms), (1) is ahead at 512 x 546 = 279 552 rows (5.30 against
// 5.62 ms) and at 4 096 x 70 = 286 720 (3.70 against 4.40 ms), and by 3.1 ms at 14 000 x 70.  Between the two measured sides the differences
// cross zero at about 130 000 rows for the traces and 100 000 for the plan, whatever multiplies to it, so the rule is in rows.  A map of far
// more vertices moves both forms alike (each walks or stages every vertex per row); none has been measured.
#define LG_FORM2_MAX_ROWS (1L << 17)      // (2) up to here, (1) above
static int lg_form(long rows) { return rows <= LG_FORM2_MAX_ROWS ? 2 : 1; }

// the lanes' own rules; `c` may be null (the host entry): then only the code is returned
static int lg_lanes_ok(mind_ctx *c, const char *who, const double *verts, const int32_t *lane_off, int P) {
#define LG_FAIL(...) return c ? fail(c, MIND_EINVAL, __VA_ARGS__) : MIND_EINVAL
  if (!verts || !lane_off) LG_FAIL("%s: null verts / lane_off", who);
  if (P < 1 || P > LG_MAX_LANES) LG_FAIL("%s: %d lanes, 1..%d are supported", who, P, LG_MAX_LANES);
  if (lane_off[0] != 0) LG_FAIL("%s: lane_off[0] = %d, 0 is needed", who, (int)lane_off[0]);
  for (int l = 0; l < P; ++l) {
    const long n = (long)lane_off[l + 1] - (long)lane_off[l];
    if (n < 2) LG_FAIL("%s: lane %d: lane_off gives it %ld vertices, a lane needs two (and lane_off must ascend)", who, l, n);
    if (lane_off[l + 1] > RD_MAX_VERTS) LG_FAIL("%s: more than %d vertices", who, RD_MAX_VERTS);
  }
  const long V = lane_off[P];
  for (long i = 0; i < V * 2; ++i)
    if (!au_fin(verts[i])) LG_FAIL("%s: vertex %ld is not finite", who, i / 2);
#undef LG_FAIL
  return MIND_OK;
}
static int lg_cfg_ok(mind_ctx *c, const char *who, const mind_audit_lane_cfg *cfg) {
#define LG_FAIL(...) return c ? fail(c, MIND_EINVAL, __VA_ARGS__) : MIND_EINVAL
  if (!(cfg->cos_flow >= -1.0 && cfg->cos_flow <= 1.0)) LG_FAIL("%s: cos_flow = %g, a value in [-1, 1] is needed", who, cfg->cos_flow);
  if (!au_fin(cfg->bound) || !(cfg->bound > 0.0)) LG_FAIL("%s: bound = %g, a finite value > 0 is needed", who, cfg->bound);
  if (cfg->form < 0 || cfg->form > 2) LG_FAIL("%s: form = %d; 0 (the library's rule), 1 (thread per box) or 2 (one wavefront per box)", who, cfg->form);
#undef LG_FAIL
  return MIND_OK;
}

// the lanes in the arena: verts, lane_off with one entry more (V once again: k_lane_boxes<1> reads one bound past the last lane), cum
struct LgLanes { ArField<double> verts, cum; ArField<int> off; int V, P; std::vector<int> off2; std::vector<double> cum_h; };
static void lg_lanes_take(Arena &ar, LgLanes &r, const double *verts, const int32_t *lane_off, int P) {
  r.V = lane_off[P];
  r.P = P;
  r.verts = ar.take<double>((size_t)r.V * 2);
  r.cum = ar.take<double>((size_t)r.V);
  r.off = ar.take<int>((size_t)P + 2);
  r.off2.assign(lane_off, lane_off + P + 1);
  r.off2.push_back(r.V);
  r.cum_h.resize((size_t)r.V);
  lg_cum(verts, r.off2.data(), P, r.cum_h.data());
}
static int lg_lanes_upload(mind_ctx *c, char *d, const LgLanes &r, const double *verts) {
  int rc;
  if ((rc = ar_put(c, d, r.verts, verts)) || (rc = ar_put(c, d, r.cum, r.cum_h.data()))) return rc;
  return ar_put(c, d, r.off, r.off2.data());
}

// the per-box outputs of k_lane_boxes, [2, R] each (0 = any, 1 = flow), and the margin [R]
struct LgBoxes { ArField<double> lat, s, along, across, margin; ArField<int> lane, edge; };
static LgBoxes lg_boxes_take(Arena &ar, size_t R) {
  LgBoxes b;
  b.lat = ar.take<double>(2 * R); b.s = ar.take<double>(2 * R); b.along = ar.take<double>(2 * R); b.across = ar.take<double>(2 * R);
  b.margin = ar.take<double>(R);
  b.lane = ar.take<int>(2 * R); b.edge = ar.take<int>(2 * R);
  return b;
}
static void lg_boxes_launch(hipStream_t s, char *d, int form, const AuBox &eb, const mind_audit_lane_cfg *cfg, size_t R, const double *states, int stride,
                            int iyaw, const LgLanes &ln, const LgBoxes &b) {
  if (form == 1)
    hipLaunchKernelGGL(k_lane_boxes<1>, dim3((unsigned)((R + LG_BB - 1) / LG_BB)), dim3(LG_BB), 0, s, eb, cfg->cos_flow, cfg->bound, (long)R, states, stride, iyaw,
                       ln.verts.at(d), ln.off.at(d), ln.P, ln.V, ln.cum.at(d), b.lat.at(d), b.s.at(d), b.along.at(d), b.across.at(d), b.lane.at(d), b.edge.at(d),
                       b.margin.at(d));
  else
    hipLaunchKernelGGL(k_lane_boxes<2>, dim3((unsigned)R), dim3(64), 0, s, eb, cfg->cos_flow, cfg->bound, (long)R, states, stride, iyaw, ln.verts.at(d),
                       ln.off.at(d), ln.P, ln.V, ln.cum.at(d), b.lat.at(d), b.s.at(d), b.along.at(d), b.across.at(d), b.lane.at(d), b.edge.at(d), b.margin.at(d));
}

extern "C" int mind_audit_lane_plan(mind_ctx *c, const mind_audit_box *ego, const mind_audit_lane_cfg *cfg, const double *verts, const int32_t *lane_off,
                                    int n_lanes, const mind_cost_tree *trees, int n_trees, int n_cand, const double *xs, const mind_audit_lane_plan_out *out) {
  const char *who = "mind_audit_lane_plan";
  if (!c) return MIND_EINVAL;
  if (!ego || !cfg || !out || n_trees < 0 || n_cand < 0 || (n_trees > 0 && !trees)) return fail(c, MIND_EINVAL, "%s: null ego / cfg / trees / out or a negative count", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  int rc;
  if ((rc = lg_cfg_ok(c, who, cfg)) || (rc = lg_lanes_ok(c, who, verts, lane_off, n_lanes))) return rc;
  if (!out->node_lat && !out->node_s && !out->node_along && !out->node_across && !out->node_lane && !out->node_edge && !out->node_margin && !out->tree_min &&
      !out->tree_node && !out->tree_lane && !out->tree_hits && !out->tree_first && !out->tree_mass && !out->tree_progress)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  Arena ar;
  std::vector<char> img;
  AuPlanTrees pt;
  if ((rc = au_plan_trees(c, who, trees, n_trees, n_cand, ar, img, pt))) return rc;
  const long Mtot = pt.Mtot;
  for (int t = 0; t < n_trees; ++t) {
    if (!trees[t].parent) return fail(c, MIND_EINVAL, "%s: tree %d: null parent", who, t);
    for (int i = 0; i < trees[t].n_nodes; ++i)
      if (trees[t].parent[i] >= trees[t].n_nodes) return fail(c, MIND_EINVAL, "%s: tree %d node %d: parent %d of %d nodes", who, t, i, (int)trees[t].parent[i], trees[t].n_nodes);
  }
  if (n_cand > 0 && Mtot > 0 && !xs) return fail(c, MIND_EINVAL, "%s: null xs", who);
  if ((rc = au_busy(c, who))) return rc;
  if (n_cand == 0 || Mtot == 0) return MIND_OK;

  const size_t R = (size_t)n_cand * (size_t)Mtot, RT = (size_t)n_cand * (size_t)n_trees;
  const auto f_par = ar.take<int>((size_t)Mtot);
  img.resize(ar.top, 0);
  {
    long moff = 0;
    for (int t = 0; t < n_trees; ++t) {
      std::copy_n(trees[t].parent, trees[t].n_nodes, f_par.at(img.data()) + moff);
      moff += trees[t].n_nodes;
    }
  }
  LgLanes ln;
  lg_lanes_take(ar, ln, verts, lane_off, n_lanes);
  const auto f_xs = ar.take<double>(R * 6);
  const LgBoxes b = lg_boxes_take(ar, R);
  const auto f_tmin = ar.take<double>(RT), f_tmass = ar.take<double>(RT), f_tprog = ar.take<double>(RT);
  const auto f_tnode = ar.take<int>(RT), f_tlane = ar.take<int>(RT), f_thits = ar.take<int>(RT), f_tfirst = ar.take<int>(RT);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(d, img.data(), img.size(), hipMemcpyHostToDevice, s));
  if ((rc = lg_lanes_upload(c, d, ln, verts)) || (rc = ar_put(c, d, f_xs, xs))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  lg_boxes_launch(s, d, cfg->form ? cfg->form : lg_form((long)R), eb, cfg, R, f_xs.at(d), 6, 3, ln, b);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_plan_trees, dim3((unsigned)((RT + 255) / 256)), dim3(256), 0, s, (int)Mtot, n_cand, n_trees, pt.trees.at(d), pt.prob.at(d),
                     b.margin.at(d), b.lane.at(d) + R, f_tmin.at(d), f_tnode.at(d), f_tlane.at(d), f_thits.at(d), f_tfirst.at(d), f_tmass.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_lane_progress<true>, dim3((unsigned)((RT + 63) / 64)), dim3(64), 0, s, n_cand, (int)Mtot, n_trees, pt.trees.at(d), f_par.at(d), pt.prob.at(d),
                     b.lane.at(d), b.s.at(d), f_tprog.at(d), (double *)nullptr);
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->node_lat, b.lat}, {out->node_s, b.s}, {out->node_along, b.along}, {out->node_across, b.across}, {out->node_lane, b.lane},
                          {out->node_edge, b.edge}, {out->node_margin, b.margin}, {out->tree_min, f_tmin}, {out->tree_node, f_tnode}, {out->tree_lane, f_tlane},
                          {out->tree_hits, f_thits}, {out->tree_first, f_tfirst}, {out->tree_mass, f_tmass}, {out->tree_progress, f_tprog}});
}

extern "C" int mind_audit_lane_episode(mind_ctx *c, const mind_audit_box *ego, const mind_audit_lane_cfg *cfg, const double *verts, const int32_t *lane_off,
                                       int n_lanes, int n_ego, int n_steps, const double *ego_states, const mind_audit_lane_episode_out *out) {
  const char *who = "mind_audit_lane_episode";
  if (!c) return MIND_EINVAL;
  if (!ego || !cfg || !out || n_ego < 0 || n_steps < 0) return fail(c, MIND_EINVAL, "%s: null ego / cfg / out or a negative count", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  int rc;
  if ((rc = lg_cfg_ok(c, who, cfg)) || (rc = lg_lanes_ok(c, who, verts, lane_off, n_lanes))) return rc;
  if (!out->step_lat && !out->step_s && !out->step_along && !out->step_across && !out->step_lane && !out->step_edge && !out->step_margin && !out->ego_min &&
      !out->ego_step && !out->ego_lane && !out->ego_hits && !out->ego_first && !out->ego_progress && !out->ego_back)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  const size_t R = (size_t)n_ego * (size_t)n_steps, ne = (size_t)n_ego;
  if ((long)R > AU_EPISODE_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d egos x %d steps > %ld rows supported", who, n_ego, n_steps, AU_EPISODE_MAX_ROWS);
  if (R > 0 && !ego_states) return fail(c, MIND_EINVAL, "%s: null ego_states", who);
  if ((rc = au_busy(c, who))) return rc;
  if (R == 0) return MIND_OK;

  Arena ar;
  LgLanes ln;
  lg_lanes_take(ar, ln, verts, lane_off, n_lanes);
  const auto f_ego = ar.take<double>(R * 4);
  const LgBoxes b = lg_boxes_take(ar, R);
  const auto f_emin = ar.take<double>(ne), f_eprog = ar.take<double>(ne), f_eback = ar.take<double>(ne);
  const auto f_estep = ar.take<int>(ne), f_elane = ar.take<int>(ne), f_ehits = ar.take<int>(ne), f_efirst = ar.take<int>(ne);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  if ((rc = lg_lanes_upload(c, d, ln, verts)) || (rc = ar_put(c, d, f_ego, ego_states))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  lg_boxes_launch(s, d, cfg->form ? cfg->form : lg_form((long)R), eb, cfg, R, f_ego.at(d), 4, 3, ln, b);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_episode_egos<true>, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, 0.0, b.margin.at(d), b.lane.at(d) + R,
                     f_emin.at(d), f_estep.at(d), f_elane.at(d), f_ehits.at(d), f_efirst.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_lane_progress<false>, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, 0, (const AuTree *)nullptr, (const int *)nullptr,
                     (const float *)nullptr, b.lane.at(d), b.s.at(d), f_eprog.at(d), f_eback.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->step_lat, b.lat}, {out->step_s, b.s}, {out->step_along, b.along}, {out->step_across, b.across}, {out->step_lane, b.lane},
                          {out->step_edge, b.edge}, {out->step_margin, b.margin}, {out->ego_min, f_emin}, {out->ego_step, f_estep}, {out->ego_lane, f_elane},
                          {out->ego_hits, f_ehits}, {out->ego_first, f_efirst}, {out->ego_progress, f_eprog}, {out->ego_back, f_eback}});
}

extern "C" int mind_debug_lane_project(int n, const double *boxes, const mind_audit_box *ego, const mind_audit_lane_cfg *cfg, const double *verts,
                                       const int32_t *lane_off, int n_lanes, const double *trig, double *lat, double *s, double *along, double *across,
                                       int32_t *lane, int32_t *edge, double *margin) {
  if (n < 0 || !au_box_ok(ego) || !cfg || (n > 0 && !boxes) || (!lat && !s && !along && !across && !lane && !edge && !margin)) return MIND_EINVAL;
  int rc;
  if ((rc = lg_cfg_ok(nullptr, "mind_debug_lane_project", cfg)) || (rc = lg_lanes_ok(nullptr, "mind_debug_lane_project", verts, lane_off, n_lanes))) return rc;
  std::vector<double> cum((size_t)lane_off[n_lanes]);
  lg_cum(verts, lane_off, n_lanes, cum.data());
  for (int i = 0; i < n; ++i) {
    const double *b = boxes + (size_t)i * 3;
    lg_out o[2];
    double mg = NAN;
    lg_out_nan(&o[0]);
    lg_out_nan(&o[1]);
    if (au_fin(b[0]) && au_fin(b[1]) && au_fin(b[2])) {
      double cs, sn;
      if (trig) { cs = trig[(size_t)i * 2]; sn = trig[(size_t)i * 2 + 1]; }
      else au_host::mind_sincos(b[2], &sn, &cs);
      mg = lg_box_lanes(b[0], b[1], cs, sn, ego->center_offset, cfg->cos_flow, cfg->bound, verts, lane_off, n_lanes, cum.data(), o);
    }
    for (int k = 0; k < 2; ++k) {
      const size_t r = (size_t)k * (size_t)n + (size_t)i;
      if (lat) lat[r] = o[k].lat;
      if (s) s[r] = o[k].s;
      if (along) along[r] = o[k].along;
      if (across) across[r] = o[k].across;
      if (lane) lane[r] = o[k].lane;
      if (edge) edge[r] = o[k].edge;
    }
    if (margin) margin[i] = mg;
  }
  return MIND_OK;
}
