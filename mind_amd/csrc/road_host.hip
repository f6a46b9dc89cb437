// Host side of the road audit (kernels: road_kernels.hip; geometry: road_geom.h): mind_audit_road_plan, mind_audit_road_episode and the
// host-only mind_debug_road_margin.  Both device calls are synchronous on the context's stream and keep their scratch in c->road_dev.
// Included by mind_hip.hip behind forecast_host.hip (au_host::mind_sincos, au_fin, au_box_ok, au_busy, au_take: audit_host.hip).
#pragma clang fp contract(off)

#define RD_MAX_VERTS (1 << 20)            // vertices of a road (16 MB)
#define RD_MAX_RINGS (1 << 16)            // rings of a road
#define RD_PLAN_MAX_ROWS (1L << 20)       // n_cand x sum M a plan audit admits, as mind_audit_plan
#define RD_EPISODE_MAX_ROWS (1L << 22)    // n_ego x n_steps an episode audit admits, as mind_audit_episode

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
struct RdRoadAt { size_t o_verts, o_off; int V; };
static RdRoadAt rd_road_take(size_t &top, const int32_t *poly_off, int P) {
  RdRoadAt a;
  a.V = poly_off[P];
  a.o_verts = au_take(top, (size_t)a.V * 2, sizeof(double));
  a.o_off = au_take(top, (size_t)P + 2, sizeof(int));
  return a;
}
static int rd_road_upload(mind_ctx *c, char *d, const RdRoadAt &a, const double *verts, const int32_t *poly_off, int P, std::vector<int> &off2) {
  off2.assign(poly_off, poly_off + P + 1);
  off2.push_back(a.V);
  HIPCHK(c, hipMemcpyAsync(d + a.o_verts, verts, (size_t)a.V * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + a.o_off, off2.data(), off2.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return MIND_OK;
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
  long Mtot = 0;
  for (int t = 0; t < n_trees; ++t) {
    if (trees[t].n_nodes <= 0 || !trees[t].prob) return fail(c, MIND_EINVAL, "%s: tree %d: bad n_nodes or null prob", who, t);
    Mtot += trees[t].n_nodes;
    if (Mtot > RD_PLAN_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: more than %ld nodes", who, RD_PLAN_MAX_ROWS);
  }
  if ((long)n_cand * Mtot > RD_PLAN_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d candidates x %ld nodes > %ld rows supported", who, n_cand, Mtot, RD_PLAN_MAX_ROWS);
  if (n_cand > 0 && Mtot > 0 && !xs) return fail(c, MIND_EINVAL, "%s: null xs", who);
  if ((rc = au_busy(c, who))) return rc;
  if (n_cand == 0 || Mtot == 0) return MIND_OK;

  const size_t R = (size_t)n_cand * (size_t)Mtot, RT = (size_t)n_cand * (size_t)n_trees;
  size_t top = 0;
  const size_t o_trees = au_take(top, n_trees, sizeof(AuTree)), o_prob = au_take(top, Mtot, sizeof(float));
  const size_t n_img = top;
  const RdRoadAt road = rd_road_take(top, poly_off, n_rings);
  const size_t o_xs = au_take(top, R * 6, sizeof(double)), o_m = au_take(top, R, sizeof(double)), o_c = au_take(top, R, sizeof(int)),
               o_r = au_take(top, R, sizeof(int)), o_e = au_take(top, R, sizeof(int)), o_tmin = au_take(top, RT, sizeof(double)),
               o_tmass = au_take(top, RT, sizeof(double)), o_tnode = au_take(top, RT, sizeof(int)), o_tcorner = au_take(top, RT, sizeof(int)),
               o_thits = au_take(top, RT, sizeof(int)), o_tfirst = au_take(top, RT, sizeof(int));
  std::vector<char> img(n_img, 0);
  {
    AuTree *ht = (AuTree *)(img.data() + o_trees);
    long moff = 0;
    for (int t = 0; t < n_trees; ++t) {
      ht[t] = AuTree{(int)moff, trees[t].n_nodes};
      memcpy(img.data() + o_prob + moff * sizeof(float), trees[t].prob, (size_t)trees[t].n_nodes * sizeof(float));
      moff += trees[t].n_nodes;
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->road_dev, top))) return rc;
  char *d = (char *)c->road_dev.p;
  hipStream_t s = c->stream;
  std::vector<int> off2;
  HIPCHK(c, hipMemcpyAsync(d, img.data(), n_img, hipMemcpyHostToDevice, s));
  if ((rc = rd_road_upload(c, d, road, verts, poly_off, n_rings, off2))) return rc;
  HIPCHK(c, hipMemcpyAsync(d + o_xs, xs, R * 6 * sizeof(double), hipMemcpyHostToDevice, s));
  const RdBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_road_boxes, dim3((unsigned)((R + RD_BB - 1) / RD_BB)), dim3(RD_BB), 0, s, eb, (long)R, (const double *)(d + o_xs), 6, 3,
                     (const double *)(d + road.o_verts), (const int *)(d + road.o_off), road.V, (double *)(d + o_m), (int *)(d + o_c), (int *)(d + o_r),
                     (int *)(d + o_e));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_road_plan_trees, dim3((unsigned)((RT + 255) / 256)), dim3(256), 0, s, (int)Mtot, n_cand, n_trees, (const AuTree *)(d + o_trees),
                     (const float *)(d + o_prob), (const double *)(d + o_m), (const int *)(d + o_c), (double *)(d + o_tmin), (int *)(d + o_tnode),
                     (int *)(d + o_tcorner), (int *)(d + o_thits), (int *)(d + o_tfirst), (double *)(d + o_tmass));
  HIPCHK(c, hipGetLastError());
  const struct { void *h; size_t o, bytes; } back[10] = {
      {out->node_margin, o_m, R * sizeof(double)},   {out->node_corner, o_c, R * sizeof(int)},         {out->node_ring, o_r, R * sizeof(int)},
      {out->node_edge, o_e, R * sizeof(int)},        {out->tree_min, o_tmin, RT * sizeof(double)},     {out->tree_node, o_tnode, RT * sizeof(int)},
      {out->tree_corner, o_tcorner, RT * sizeof(int)}, {out->tree_hits, o_thits, RT * sizeof(int)},    {out->tree_first, o_tfirst, RT * sizeof(int)},
      {out->tree_mass, o_tmass, RT * sizeof(double)}};
  for (const auto &b : back)
    if (b.h) HIPCHK(c, hipMemcpyAsync(b.h, d + b.o, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return MIND_OK;
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
  if ((long)R > RD_EPISODE_MAX_ROWS) return fail(c, MIND_EINVAL, "%s: %d egos x %d steps > %ld rows supported", who, n_ego, n_steps, RD_EPISODE_MAX_ROWS);
  if (R > 0 && !ego_states) return fail(c, MIND_EINVAL, "%s: null ego_states", who);
  if ((rc = au_busy(c, who))) return rc;
  if (R == 0) return MIND_OK;

  size_t top = 0;
  const RdRoadAt road = rd_road_take(top, poly_off, n_rings);
  const size_t o_ego = au_take(top, R * 4, sizeof(double)), o_m = au_take(top, R, sizeof(double)), o_c = au_take(top, R, sizeof(int)),
               o_r = au_take(top, R, sizeof(int)), o_e = au_take(top, R, sizeof(int)), o_emin = au_take(top, ne, sizeof(double)),
               o_estep = au_take(top, ne, sizeof(int)), o_ecorner = au_take(top, ne, sizeof(int)), o_ehits = au_take(top, ne, sizeof(int)),
               o_efirst = au_take(top, ne, sizeof(int));
  HIPCHK(c, hipSetDevice(c->device));
  if ((rc = ensure(c, c->road_dev, top))) return rc;
  char *d = (char *)c->road_dev.p;
  hipStream_t s = c->stream;
  std::vector<int> off2;
  if ((rc = rd_road_upload(c, d, road, verts, poly_off, n_rings, off2))) return rc;
  HIPCHK(c, hipMemcpyAsync(d + o_ego, ego_states, R * 4 * sizeof(double), hipMemcpyHostToDevice, s));
  const RdBox eb{ego->length, ego->width, ego->center_offset};
  hipLaunchKernelGGL(k_road_boxes, dim3((unsigned)((R + RD_BB - 1) / RD_BB)), dim3(RD_BB), 0, s, eb, (long)R, (const double *)(d + o_ego), 4, 3,
                     (const double *)(d + road.o_verts), (const int *)(d + road.o_off), road.V, (double *)(d + o_m), (int *)(d + o_c), (int *)(d + o_r),
                     (int *)(d + o_e));
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_road_episode_egos, dim3((unsigned)((n_ego + 63) / 64)), dim3(64), 0, s, n_ego, n_steps, (const double *)(d + o_m),
                     (const int *)(d + o_c), (double *)(d + o_emin), (int *)(d + o_estep), (int *)(d + o_ecorner), (int *)(d + o_ehits), (int *)(d + o_efirst));
  HIPCHK(c, hipGetLastError());
  const struct { void *h; size_t o, bytes; } back[9] = {
      {out->step_margin, o_m, R * sizeof(double)},  {out->step_corner, o_c, R * sizeof(int)},      {out->step_ring, o_r, R * sizeof(int)},
      {out->step_edge, o_e, R * sizeof(int)},       {out->ego_min, o_emin, ne * sizeof(double)},   {out->ego_step, o_estep, ne * sizeof(int)},
      {out->ego_corner, o_ecorner, ne * sizeof(int)}, {out->ego_hits, o_ehits, ne * sizeof(int)},  {out->ego_first, o_efirst, ne * sizeof(int)}};
  for (const auto &b : back)
    if (b.h) HIPCHK(c, hipMemcpyAsync(b.h, d + b.o, b.bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return MIND_OK;
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
