// Host side of the road audit (kernels: road_kernels.hip; geometry: road_geom.h): mind_audit_road_plan, mind_audit_road_episode and the
// host-only mind_debug_road_margin.  Both device calls are synchronous on the context's stream and run on the scaffold of audit_host.hip.
// Included by mind_hip.hip behind forecast_host.hip (au_host::mind_sincos, au_fin, au_box_ok, au_busy, au_plan_trees, ar_*: audit_host.hip).
#pragma clang fp contract(off)

#define RD_MAX_VERTS (1 << 20)            // vertices of a road (16 MB)
#define RD_MAX_RINGS (1 << 16)            // rings of a road

// the road's own rules; `c` may be null (the host entry): then only the code is returned
static int rd_road_ok(mind_ctx *c, const char *who, const double *verts, const int32_t *poly_off, int P) {
#define RD_FAIL(...) return c ? fail(c, MIND_EINVAL, __VA_ARGS__) : MIND_EINVAL
  if (!verts || !poly_off) RD_FAIL("%s: null verts / poly_off", who);
  if (P < 1 || P > RD_MAX_RINGS) RD_FAIL("%s: %d rings, 1..%d are supported", who, P, RD_MAX_RINGS);
  if (poly_off[0] != 0) RD_FAIL("%s: poly_off[0] = %d, 0 is needed", who, (int)poly_off[0]);
  for (int r = 0; r < P; ++r) {
    const long n = (long)poly_off[r + 1] - (long)poly_off[r];
    if (n < 3) RD_FAIL("%s: ring %d: poly_off gives it %ld vertices, a ring needs three (and poly_off must ascend)", who, r, n);
    if (poly_off[r + 1] > RD_MAX_VERTS) RD_FAIL("%s: more than %d vertices", who, RD_MAX_VERTS);
  }
  const long V = poly_off[P];
  for (long i = 0; i < V * 2; ++i)
    if (!au_fin(verts[i])) RD_FAIL("%s: vertex %ld is not finite", who, i / 2);
#undef RD_FAIL
  return MIND_OK;
}

// the road in the arena: verts, then poly_off with one entry more (V once again: k_road_boxes reads one bound past the last ring)
struct RdRoad { ArField<double> verts; ArField<int> off; int V; std::vector<int> off2; };
static void rd_road_take(Arena &ar, RdRoad &r, const int32_t *poly_off, int P) {
  r.V = poly_off[P];
  r.verts = ar.take<double>((size_t)r.V * 2);
  r.off = ar.take<int>((size_t)P + 2);
  r.off2.assign(poly_off, poly_off + P + 1);
  r.off2.push_back(r.V);
}
static int rd_road_upload(mind_ctx *c, char *d, const RdRoad &r, const double *verts) {
  int rc;
  if ((rc = ar_put(c, d, r.verts, verts))) return rc;
  return ar_put(c, d, r.off, r.off2.data());
}

extern "C" int mind_audit_road_plan(mind_ctx *c, const mind_audit_box *ego, const double *verts, const int32_t *poly_off, int n_rings,
                                    const mind_cost_tree *trees, int n_trees, int n_cand, const double *xs, const mind_audit_road_plan_out *out) {
  const char *who = "mind_audit_road_plan";
  if (!c) return MIND_EINVAL;
  if (!ego || !out || n_trees < 0 || n_cand < 0 || (n_trees > 0 && !trees)) return fail(c, MIND_EINVAL, "%s: null ego / trees / out or a negative count", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  int rc;
  if ((rc = rd_road_ok(c, who, verts, poly_off, n_rings))) return rc;
  if (!out->node_margin && !out->node_corner && !out->node_ring && !out->node_edge && !out->tree_min && !out->tree_node && !out->tree_corner &&
      !out->tree_hits && !out->tree_first && !out->tree_mass)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  Arena ar;
  std::vector<char> img;
  AuPlanTrees pt;
  if ((rc = au_plan_trees(c, who, trees, n_trees, n_cand, ar, img, pt))) return rc;
  const long Mtot = pt.Mtot;
  if (n_cand > 0 && Mtot > 0 && !xs) return fail(c, MIND_EINVAL, "%s: null xs", who);
  if ((rc = au_busy(c, who))) return rc;
  if (n_cand == 0 || Mtot == 0) return MIND_OK;

  const size_t R = (size_t)n_cand * (size_t)Mtot, RT = (size_t)n_cand * (size_t)n_trees;
  RdRoad road;
  rd_road_take(ar, road, poly_off, n_rings);
  const auto f_xs = ar.take<double>(R * 6), f_m = ar.take<double>(R);
  const auto f_c = ar.take<int>(R), f_r = ar.take<int>(R), f_e = ar.take<int>(R);
  const auto f_tmin = ar.take<double>(RT), f_tmass = ar.take<double>(RT);
  const auto f_tnode = ar.take<int>(RT), f_tcorner = ar.take<int>(RT), f_thits = ar.take<int>(RT), f_tfirst = ar.take<int>(RT);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  HIPCHK(c, hipMemcpyAsync(d, img.data(), img.size(), hipMemcpyHostToDevice, s));
  if ((rc = rd_road_upload(c, d, road, verts)) || (rc = ar_put(c, d, f_xs, xs))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_road_boxes, dim3((unsigned)((R + RD_BB - 1) / RD_BB)), dim3(RD_BB), 0, s, eb, (long)R, f_xs.at(d), 6, 3, road.verts.at(d), road.off.at(d),
                     road.V, f_m.at(d), f_c.at(d), f_r.at(d), f_e.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_plan_trees, dim3((unsigned)((RT + 255) / 256)), dim3(256), 0, s, (int)Mtot, n_cand, n_trees, pt.trees.at(d), pt.prob.at(d),
                     f_m.at(d), f_c.at(d), f_tmin.at(d), f_tnode.at(d), f_tcorner.at(d), f_thits.at(d), f_tfirst.at(d), f_tmass.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->node_margin, f_m}, {out->node_corner, f_c}, {out->node_ring, f_r}, {out->node_edge, f_e}, {out->tree_min, f_tmin},
                          {out->tree_node, f_tnode}, {out->tree_corner, f_tcorner}, {out->tree_hits, f_thits}, {out->tree_first, f_tfirst},
                          {out->tree_mass, f_tmass}});
}

extern "C" int mind_audit_road_episode(mind_ctx *c, const mind_audit_box *ego, const double *verts, const int32_t *poly_off, int n_rings, int n_ego,
                                       int n_steps, const double *ego_states, const mind_audit_road_episode_out *out) {
  const char *who = "mind_audit_road_episode";
  if (!c) return MIND_EINVAL;
  if (!ego || !out || n_ego < 0 || n_steps < 0) return fail(c, MIND_EINVAL, "%s: null ego / out or a negative count", who);
  if (!au_box_ok(ego)) return fail(c, MIND_EINVAL, "%s: the ego box needs finite length, width >= 0 and a finite center_offset", who);
  int rc;
  if ((rc = rd_road_ok(c, who, verts, poly_off, n_rings))) return rc;
  if (!out->step_margin && !out->step_corner && !out->step_ring && !out->step_edge && !out->ego_min && !out->ego_step && !out->ego_corner &&
      !out->ego_hits && !out->ego_first)
    return fail(c, MIND_EINVAL, "%s: every output is null", who);
  const size_t R = (size_t)n_ego * (size_t)n_steps, ne = (size_t)n_ego;
  if ((long)R > AU_EPISODE_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d egos x %d steps > %ld rows supported", who, n_ego, n_steps, AU_EPISODE_MAX_ROWS);
  if (R > 0 && !ego_states) return fail(c, MIND_EINVAL, "%s: null ego_states", who);
  if ((rc = au_busy(c, who))) return rc;
  if (R == 0) return MIND_OK;

  Arena ar;
  RdRoad road;
  rd_road_take(ar, road, poly_off, n_rings);
  const auto f_ego = ar.take<double>(R * 4), f_m = ar.take<double>(R);
  const auto f_c = ar.take<int>(R), f_r = ar.take<int>(R), f_e = ar.take<int>(R);
  const auto f_emin = ar.take<double>(ne);
  const auto f_estep = ar.take<int>(ne), f_ecorner = ar.take<int>(ne), f_ehits = ar.take<int>(ne), f_efirst = ar.take<int>(ne);
  char *d;
  if ((rc = ar_begin(c, ar, &d))) return rc;
  hipStream_t s = c->stream;
  if ((rc = rd_road_upload(c, d, road, verts)) || (rc = ar_put(c, d, f_ego, ego_states))) return rc;
  const AuBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_road_boxes, dim3((unsigned)((R + RD_BB - 1) / RD_BB)), dim3(RD_BB), 0, s, eb, (long)R, f_ego.at(d), 4, 3, road.verts.at(d), road.off.at(d),
                     road.V, f_m.at(d), f_c.at(d), f_r.at(d), f_e.at(d));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_audit_episode_egos<true>, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, 0.0, f_m.at(d), f_c.at(d), f_emin.at(d),
                     f_estep.at(d), f_ecorner.at(d), f_ehits.at(d), f_efirst.at(d));
  HIPCHK(c, hipGetLastError());
  return ar_finish(c, d, {{out->step_margin, f_m}, {out->step_corner, f_c}, {out->step_ring, f_r}, {out->step_edge, f_e}, {out->ego_min, f_emin},
                          {out->ego_step, f_estep}, {out->ego_corner, f_ecorner}, {out->ego_hits, f_ehits}, {out->ego_first, f_efirst}});
}

extern "C" int mind_debug_road_margin(int n, const double *boxes, const mind_audit_box *ego, const double *verts, const int32_t *poly_off, int n_rings,
                                      const double *trig, double *margin, int32_t *corner, int32_t *ring, int32_t *edge) {
  if (n < 0 || !au_box_ok(ego) || (n > 0 && !boxes) || (!margin && !corner && !ring && !edge)) return MIND_EINVAL;
  int rc;
  if ((rc = rd_road_ok(nullptr, "mind_debug_road_margin", verts, poly_off, n_rings))) return rc;
  for (int i = 0; i < n; ++i) {
    const double *b = boxes + (size_t)i * 3;
    double m = NAN;
    int bk = -1, br = -1, be = -1;
    if (au_fin(b[0]) && au_fin(b[1]) && au_fin(b[2])) {
      double cs, sn;
      if (trig) { cs = trig[(size_t)i * 2]; sn = trig[(size_t)i * 2 + 1]; }
      else au_host::mind_sincos(b[2], &sn, &cs);
      m = rg_box_road(b[0], b[1], cs, sn, ego->length, ego->width, ego->center_offset, verts, poly_off, n_rings, &bk, &br, &be);
    }
    if (margin) margin[i] = m;
    if (corner) corner[i] = bk;
    if (ring) ring[i] = br;
    if (edge) edge[i] = be;
  }
  return MIND_OK;
}
