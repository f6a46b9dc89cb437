// Host side of the predictor forward (included by mind_hip.hip): mind_predict_batch as a sequence of stages.  Which kernels run is decided
// once per call by pred_choose (pred_choice.h); the stages below switch on its record and read no knob.
__global__ void k_tokpos(const TokMeta *__restrict__ meta, int n_tok, const float *__restrict__ actr,
                         const float *__restrict__ avec, const float *__restrict__ lctr,
                         const float *__restrict__ lvec, float *__restrict__ tokpos) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tok) return;
  const TokMeta m = meta[t];
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (m.type == 0 && actr) o = make_float4(actr[m.src * 2], actr[m.src * 2 + 1], avec[m.src * 2], avec[m.src * 2 + 1]);
  if (m.type == 1 && lctr) o = make_float4(lctr[m.src * 2], lctr[m.src * 2 + 1], lvec[m.src * 2], lvec[m.src * 2 + 1]);
  ((float4 *)tokpos)[t] = o;
}

// ---- host tables of one batch shape: tokens, pair jobs, row tables, pair counts -- from the scenes' (actors, lanes)
struct PairTables {
  std::vector<TokMeta> meta;
  std::vector<PairJob> jobs, jobs5;      // jobs5: the columns the last fusion layer consumes (actors + cls)
  std::vector<int> actor_row, actor_scene, cls_row, scene_n;
  long long edge_pairs = 0, edge_pairs_t = 0;
  int ntok = 0, slot = 0;
  double pairs_full = 0, pairs_l5 = 0;
};

static void pair_tables_build(int Bn, const int *scene_actors, const int *scene_lanes, bool xcd_order, int n_cu, PairTables &T) {
  int A = 0;
  for (int b = 0; b < Bn; ++b) A += scene_actors[b];
  T.actor_row.assign(A, 0); T.actor_scene.assign(A, 0); T.cls_row.assign(Bn, 0); T.scene_n.assign(Bn, 0);
  int a0 = 0, l0 = 0;      // first actor / lane of the scene
  for (int b = 0; b < Bn; ++b) {
    const int a = scene_actors[b], l = scene_lanes[b];
    const int N = a + l + 1;
    const int tiles = (N + 15) / 16;
    const int ns = pair_column_splits(N);      // (a function of the scene's own size only: pair_jobs.h)
    for (int j = 0; j < N; ++j) {
      TokMeta m;
      memset(&m, 0, sizeof(m));
      m.type = j < a ? 0 : (j < a + l ? 1 : 2);
      m.src = j < a ? a0 + j : (j < a + l ? l0 + (j - a) : 0);
      m.slot0 = T.slot;
      m.nsplit = ns;
      m.flags = (j < a || j == N - 1) ? 1 : 0;
      T.meta.push_back(m);
      for (int s_ = 0; s_ < ns; ++s_) {
        PairJob J;
        memset(&J, 0, sizeof(J));
        J.edge_base = T.edge_pairs;
        J.edge_base_t = T.edge_pairs_t;
        J.N = N;
        J.j = j;
        pair_job_range(tiles, ns, s_, &J.t0, &J.t1);
        J.tok_base = T.ntok;
        J.slot = T.slot++;
        J.flags = m.flags;
        J.scene = b;
        T.jobs.push_back(J);
      }
      if (j < a) { T.actor_row[a0 + j] = T.ntok + j; T.actor_scene[a0 + j] = b; }
    }
    T.cls_row[b] = T.ntok + N - 1;
    T.scene_n[b] = N;
    T.ntok += N;
    T.edge_pairs += (long long)N * N;
    T.edge_pairs_t += (long long)N * tiles * 16;
    T.pairs_full += (double)N * N;
    T.pairs_l5 += (double)N * (a + 1);
    a0 += a; l0 += l;
  }
  // The order of a job list is its schedule (pair_jobs.h): equal work per wave slot, and for batches of eight scenes or more all column
  // jobs of a scene on one XCD.  The last fusion layer runs the consumed columns only (actors + cls): k_pair_t walks a list of its own
  // instead of skipping the other jobs after a dependent load each.
  for (const PairJob &J : T.jobs)
    if (J.flags & 1) T.jobs5.push_back(J);
  for (std::vector<PairJob> *jl : {&T.jobs, &T.jobs5}) {
    const int grid = pair_grid((long long)jl->size(), n_cu);
    pair_jobs_deal(*jl, grid, PAIR_WAVES, pair_xcd_lanes(xcd_order, Bn, grid));
  }
}

// the pair kernels' job lists as mind_predict_batch builds them (pair_tables_build), for a host-side check of the schedule
extern "C" int mind_debug_pair_schedule(const int *scene_tokens, const int *scene_actors, int n_scenes, int n_cu, int last_layer, int *out_jobs, int cap,
                                        int *out_info) {
  if (!scene_tokens || !scene_actors || n_scenes <= 0 || n_cu <= 0 || !out_jobs || !out_info) return MIND_EINVAL;
  std::vector<int> lanes(n_scenes);
  for (int b = 0; b < n_scenes; ++b) {
    const int N = scene_tokens[b], a = scene_actors[b];
    if (N <= 0 || a < 0 || a >= N) return MIND_EINVAL;
    lanes[b] = N - a - 1;
  }
  PairTables T;
  pair_tables_build(n_scenes, scene_actors, lanes.data(), true, n_cu, T);
  const std::vector<PairJob> &jl = last_layer ? T.jobs5 : T.jobs;
  const int grid = pair_grid((long long)jl.size(), n_cu);      // (a dealt list is a whole number of rounds over all wave slots, or at most one job per slot)
  const int stride = grid * PAIR_WAVES;
  int n = 0;
  for (size_t i = 0; i < jl.size(); ++i) {
    const PairJob &J = jl[i];
    if (J.t1 <= J.t0) continue;
    if (n < cap) {
      int *o = out_jobs + (size_t)6 * n;
      o[0] = J.scene; o[1] = J.j; o[2] = J.t0; o[3] = J.t1; o[4] = J.slot; o[5] = (int)(i % stride);
    }
    ++n;
  }
  out_info[0] = pair_column_splits(scene_tokens[0]); out_info[1] = grid; out_info[2] = (int)jl.size(); out_info[3] = n;
  return n;
}

// pred_choose's record for a call of the given knobs, precision and scene sizes (layout: include/mind_hip.h)
#define PRED_CHOICE_HEADER 32
extern "C" int mind_debug_predict_choice(const char *const *knob_names, const int *knob_values, int n_knobs, int pair_prec, int n_cu, int have_side,
                                         const int *scene_actors, const int *scene_lanes, int n_scenes, long long *out, int cap) {
  if (n_knobs < 0 || (n_knobs > 0 && (!knob_names || !knob_values)) || pair_prec < 0 || pair_prec > 3 || n_cu <= 0 || !scene_actors || !scene_lanes ||
      n_scenes <= 0 || cap < 0 || (cap > 0 && !out))
    return MIND_EINVAL;
  PredTuning t;
  const TnRefs own{&t, nullptr, nullptr};      // (the predictor's knobs alone: any other name is rejected)
  for (int k = 0; k < n_knobs; ++k)
    if (!knob_names[k] || !tn_set(own, knob_names[k], knob_values[k])) return MIND_EINVAL;
  for (int b = 0; b < n_scenes; ++b)
    if (scene_actors[b] <= 0 || scene_lanes[b] < 0) return MIND_EINVAL;
  const PredChoice ch = pred_choose(t, pair_prec, n_cu, have_side != 0, n_scenes, scene_actors, scene_lanes);
  const bool mfma_dec = ch.dec_actor == PRED_DEC_MFMA;
  const long long head[PRED_CHOICE_HEADER] = {
      PRED_CHOICE_HEADER, (long long)ch.tok_runs.size(), ch.np, ch.actor_form, ch.actor_arg, ch.actor_grid, ch.actor_chunk, ch.actor_chunks,
      ch.actor_launches, ch.qsplit, ch.qk_stride, ch.tiled, ch.edge_bf16, pred_edge_pair_bytes(t, pair_prec), ch.tok_chunk, ch.tok_lw,
      ch.last_tok_chunks, ch.pair_family, ch.pair_np, ch.l5_jobs5, ch.xcd_lanes, ch.xcd_lanes5, ch.dec_actor, mfma_dec ? ch.np : 0,
      ch.fp32_dec, ch.split_dec, ch.want_mw, ch.mw_blocks, ch.cls_side && !ch.want_mw, ch.tgt_wait_first, ch.split_dec ? ch.dec_head_ra : 0, ch.dec_chain_g};
  std::vector<long long> rec(head, head + PRED_CHOICE_HEADER);
  for (const PredTokRun &r : ch.tok_runs) rec.insert(rec.end(), {r.t0, r.n, r.kind, r.layerwise, r.small, r.merged});
  for (size_t i = 0; i < rec.size() && (int)i < cap; ++i) out[i] = rec[i];
  return (int)rec.size();
}

// A/B of the small, merged token launches (no knob): `form` 0 the rule (pred_tok_form), 1 k_token_m, 2 / 3 k_token_s on four / two tokens per
// workgroup; a context keeps it for its later calls.  Returns the form (1..3) a small, merged run of n_tok tokens then takes on n_cu CUs -- 0 for
// a run the default knobs do not make small -- or `form` itself with n_tok 0.  ctx may be null (nothing is kept: the rule's table, no GPU).
extern "C" int mind_debug_token_form(mind_ctx *c, int form, int n_tok, int n_cu) {
  if (form < PRED_TOK_RULE || form > PRED_TOK_S2 || n_tok < 0 || (n_tok > 0 && n_cu <= 0)) return MIND_EINVAL;
  if (c) c->debug_tok_form = form;
  if (n_tok == 0) return form;
  const int one = 1, lanes = n_tok - 2;      // a lone scene of n_tok tokens: one actor, the lanes, the cls token (pred_choose reads the sum alone: -1 lanes for one token)
  const PredChoice ch = pred_choose(PredTuning(), 3, n_cu, true, 1, &one, &lanes, form);
  return ch.tok_runs[0].form;
}

// ---- the launch clock's host side (launch_clock.h: the ring's bookkeeping and the reduction): the device ring and its page-locked mirror, the
//      copies, the sums.  With profiling on and "prof_clock" 1 a timed launch takes the next block of the ring and records no HIP event; whoever
//      read event pairs reads slots instead, behind a completed stream or copy -- the device never waits on the host.
static bool lc_on(const mind_ctx *c) { return c->profiling && c->ct.prof_clock != 0 && c->wall_khz > 0; }
static bool lc_events(const mind_ctx *c) { return c->profiling && !(c->ct.prof_clock == 1 && c->wall_khz > 0); }      // 0: events as before; 2 (debug): both

// a record's slots on the host -> its sum and per-launch list
static void lc_account(mind_ctx *c, const LcRecord &r, double (&ms)[LC_KINDS], int (&n)[LC_KINDS]) {
  const double t = lc_ticks_ms(lc_reduce(c->lc_host.as<LcSlot>() + c->lc.slot_of(r.block), r.grid), c->wall_khz);
  ms[r.kind] += t; n[r.kind] += 1;
  c->lc_last[r.kind].push_back((float)t);
}

// everything pending, read behind a drained context stream; kept in the carry sums (keep) or dropped
static int lc_flush(mind_ctx *c, bool keep) {
  const int n = (int)c->lc.pending.size();
  if (n > 0) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->pl_copy) HIPCHK(c, hipStreamSynchronize(c->pl_copy));      // (a queued copy into the mirror)
    int first[2], count[2];
    const int runs = c->lc.pending_runs(0, n, first, count);
    for (int k = 0; k < runs; ++k) {
      const size_t o = c->lc.slot_of(first[k]), b = (size_t)count[k] * c->lc.block_slots * sizeof(LcSlot);
      HIPCHK(c, hipMemcpy(c->lc_host.as<LcSlot>() + o, (const LcSlot *)c->lc_dev.p + o, b, hipMemcpyDeviceToHost));
    }
    if (keep)
      for (const LcRecord &r : c->lc.pending) lc_account(c, r, c->lc_carry_ms, c->lc_carry_n);
    c->lc.drained(n);
  }
  return MIND_OK;
}

// room for `records` launches of at most `grid` workgroups: called outside the timed launches (growing drains the stream; what was pending
// is kept in the carry sums)
static int lc_reserve(mind_ctx *c, int records, int grid) {
  if (c->lc.fits(records, grid)) return MIND_OK;
  int rc, blocks, slots;
  if ((rc = lc_flush(c, true))) return rc;
  c->lc.grown(records, grid, blocks, slots);
  if (blocks != c->lc.n_blocks || slots != c->lc.block_slots) {
    const size_t bytes = (size_t)blocks * slots * sizeof(LcSlot);
    if ((rc = ensure_exact(c, c->lc_dev, bytes, "the launch clock's ring"))) return rc;
    if (c->lc_host.alloc(bytes) != hipSuccess) { c->lc.reset(0, 0); return fail(c, MIND_ENOMEM, "hipHostMalloc(%zu) for the launch clock failed", bytes); }
    c->lc.reset(blocks, slots);
  }
  return MIND_OK;
}

// the next block's slots for a launch of `grid` workgroups, or null (clock off, or no block: the launch then is not timed)
static LcSlot *lc_take(mind_ctx *c, int grid, int kind) {
  if (!lc_on(c)) return nullptr;
  const int b = c->lc.take(grid, kind);
  return b < 0 ? nullptr : (LcSlot *)c->lc_dev.p + c->lc.slot_of(b);
}

// the pending records i0 .. i0 + n - 1 to the mirror, queued on s behind their launches
static int lc_copy_async(mind_ctx *c, hipStream_t s, int i0, int n) {
  int first[2], count[2];
  const int runs = c->lc.pending_runs(i0, n, first, count);
  for (int k = 0; k < runs; ++k) {
    const size_t o = c->lc.slot_of(first[k]), b = (size_t)count[k] * c->lc.block_slots * sizeof(LcSlot);
    HIPCHK(c, hipMemcpyAsync(c->lc_host.as<LcSlot>() + o, (const LcSlot *)c->lc_dev.p + o, b, hipMemcpyDeviceToHost, s));
  }
  if (runs > 0) c->lc.mark_copied(i0, n);
  return MIND_OK;
}

// the oldest n pending records, whose copy has completed (n < 0: all of them), go to the carry sums, and the carry of the kinds in `kinds`
// (bits 1 << LC_*) is handed out and cleared.  Records that no completed copy covers are read behind a drained stream instead
static int lc_resolve(mind_ctx *c, int n, unsigned kinds, double (&ms)[LC_KINDS], int (&cnt)[LC_KINDS]) {
  for (int k = 0; k < LC_KINDS; ++k) {
    ms[k] = 0.0; cnt[k] = 0;
    if (kinds >> k & 1u) c->lc_last[k].clear();
  }
  if (n < 0 || n > (int)c->lc.pending.size()) n = (int)c->lc.pending.size();
  if (!c->lc.copied(n)) {
    int rc;
    if ((rc = lc_flush(c, true))) return rc;
  } else {
    for (int i = 0; i < n; ++i) lc_account(c, c->lc.pending[i], c->lc_carry_ms, c->lc_carry_n);
    c->lc.drained(n);
  }
  for (int k = 0; k < LC_KINDS; ++k)
    if (kinds >> k & 1u) { ms[k] = c->lc_carry_ms[k]; cnt[k] = c->lc_carry_n[k]; c->lc_carry_ms[k] = 0.0; c->lc_carry_n[k] = 0; }
  return MIND_OK;
}

// ---- one mind_predict_batch call: what its stages share
struct PredCall {
  mind_ctx *c;
  const mind_scene_batch *in;
  mind_pred_out *out;
  const mind_pred_aux *aux;             // null: mind_predict_batch
  const PredChoice &ch;
  int Bn, A, Ltot;
  hipStream_t st, ss;                   // the context stream; the side stream (the context stream when there is none)
  TableSet *ts = nullptr;
  const float *lane_feat = nullptr;     // the caller's, or what the lane encoder wrote
  const float *const *rpe_dev = nullptr;
  Event *evs = nullptr;            // profiling: two events per pair layer
  bool tok_timed = false;               // ... and HIP events around every token launch, outside a plan
  bool act_ev = false, pair_ev = false; // this call records the ActorNet's / the pair layers' HIP events (profiling on, and not timed by the launch clock alone)
  bool pair_clk = false;                // the pair layers take blocks of the launch clock's ring
  size_t ev_tok_used = 0;
  float *x() const { return (float *)c->x.p; }
  const int *rows() const { return (const int *)ts->rows.p; }      // actor_row[A], actor_scene[A], cls_row[Bn]
};

// job / token tables, cached by the batch's scene sizes: lookup, or build + upload + synchronise
static int pred_tables(PredCall &p, const int *scene_actors, const int *scene_lanes) {
  mind_ctx *c = p.c;
  const int Bn = p.Bn, A = p.A;
  std::vector<int> key;
  key.reserve(2 * Bn + 3);
  key.push_back(Bn);
  for (int b = 0; b <= Bn; ++b) key.push_back(p.in->actor_off[b]);
  for (int b = 0; b <= Bn; ++b) key.push_back(p.in->lane_off[b]);
  TableSet *ts = nullptr;
  for (TableSet &t : c->tabs)
    if (t.key == key) ts = &t;
  const bool tab_hit = ts != nullptr;
  if (!ts) {
    ts = &c->tabs[0];
    for (TableSet &t : c->tabs)
      if (t.stamp < ts->stamp) ts = &t;         // least recently used (empty sets have stamp 0)
  }
  ts->stamp = ++c->tab_clock;
  p.ts = ts;
  if (tab_hit) {
    c->n_table_hits++;
    return MIND_OK;
  }
  PairTables T;
  pair_tables_build(Bn, scene_actors, scene_lanes, c->pt.xcd_order, c->n_cu, T);
  int rc;
  ts->key.clear();                    // invalid until the upload below has completed
  if ((rc = ensure(c, ts->meta, T.meta.size() * sizeof(TokMeta)))) return rc;
  if ((rc = ensure(c, ts->jobs, T.jobs.size() * sizeof(PairJob)))) return rc;
  if ((rc = ensure(c, ts->jobs5, T.jobs5.size() * sizeof(PairJob)))) return rc;
  if ((rc = ensure(c, ts->rows, (size_t)(2 * A + Bn) * sizeof(int)))) return rc;
  HIPCHK(c, hipMemcpyAsync(ts->meta.p, T.meta.data(), T.meta.size() * sizeof(TokMeta), hipMemcpyHostToDevice, p.st));
  HIPCHK(c, hipMemcpyAsync(ts->jobs.p, T.jobs.data(), T.jobs.size() * sizeof(PairJob), hipMemcpyHostToDevice, p.st));
  HIPCHK(c, hipMemcpyAsync(ts->jobs5.p, T.jobs5.data(), T.jobs5.size() * sizeof(PairJob), hipMemcpyHostToDevice, p.st));
  std::vector<int> rows(2 * A + Bn);
  memcpy(rows.data(), T.actor_row.data(), A * sizeof(int));
  memcpy(rows.data() + A, T.actor_scene.data(), A * sizeof(int));
  memcpy(rows.data() + 2 * A, T.cls_row.data(), Bn * sizeof(int));
  HIPCHK(c, hipMemcpyAsync(ts->rows.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, p.st));
  // the host vectors above must outlive the async copies
  HIPCHK(c, hipStreamSynchronize(p.st));
  ts->actor_row.swap(T.actor_row);
  ts->cls_row.swap(T.cls_row);
  ts->scene_n.swap(T.scene_n);
  ts->edge_pairs = T.edge_pairs; ts->edge_pairs_t = T.edge_pairs_t; ts->ntok = T.ntok; ts->slot = T.slot; ts->njobs = (int)T.jobs.size();
  ts->njobs5 = (int)T.jobs5.size();
  ts->pairs_full = T.pairs_full; ts->pairs_l5 = T.pairs_l5;
  ts->key.swap(key);
  return MIND_OK;
}

static int pred_workspaces(PredCall &p) {
  mind_ctx *c = p.c;
  const TableSet *ts = p.ts;
  const int ntok = ts->ntok, Bn = p.Bn;
  int rc;
  // (k_pair_t<*, 1> keeps the tensor in bf16: the fp32-sized buffer is simply half used)
  if ((rc = ensure(c, c->edge, (size_t)(p.ch.tiled ? ts->edge_pairs_t : ts->edge_pairs) * 128 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->x, (size_t)ntok * 128 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->ST, (size_t)ntok * 256 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->QK, (size_t)(ntok + 1) * p.ch.qk_stride * sizeof(float)))) return rc;      // (+ 1: k_pair_t6's padding rows read past the last record)
  if ((rc = ensure(c, c->part, (size_t)ts->slot * PART_STRIDE * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->tokpos, (size_t)ntok * 4 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->actor_feat, (size_t)p.A * 128 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->lane_feat, (size_t)(p.Ltot > 0 ? p.Ltot : 1) * 128 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->tgt_feat, (size_t)Bn * 128 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->cmode, (size_t)Bn * 768 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->tgt_emb, (size_t)Bn * 128 * sizeof(float)))) return rc;
  if (p.in->rpe) {
    if ((rc = ensure(c, c->rpe_ptrs, (size_t)Bn * sizeof(float *)))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->rpe_ptrs.p, p.in->rpe, (size_t)Bn * sizeof(float *), hipMemcpyHostToDevice, p.st));
    HIPCHK(c, hipStreamSynchronize(p.st));          // in->rpe is the caller's host array
    p.rpe_dev = (const float *const *)c->rpe_ptrs.p;
  }
  return MIND_OK;
}

// the ActorNet in the form pred_choose took, on the context stream (clk: the launch clock's slots of a one-launch form, or null)
static int pred_actor_net(PredCall &p, LcSlot *clk) {
  mind_ctx *c = p.c;
  const PredChoice &ch = p.ch;
  const float *actors = p.in->actors;
  float *actor_feat = (float *)c->actor_feat.p;
  const int A = p.A;
  const dim3 grid(ch.actor_grid);
  switch (ch.actor_form) {
  case PRED_ACTOR_F32:
    if (ch.actor_arg == 2) hipLaunchKernelGGL(k_actor_f32<2>, grid, dim3(AF_T), mind_actor_f32_lds_bytes(2), p.st, actors, A, actor_feat, c->W.actorF, clk);
    else hipLaunchKernelGGL(k_actor_f32<1>, grid, dim3(AF_T), mind_actor_f32_lds_bytes(1), p.st, actors, A, actor_feat, c->W.actorF, clk);
    break;
  case PRED_ACTOR_VALU:
    hipLaunchKernelGGL(k_actor_net, grid, dim3(AT), mind_actor_lds_bytes(), p.st, actors, A, actor_feat, c->W.actor, clk);
    break;
  case PRED_ACTOR_LW: {
    // the weight fragments stationary, one arena of one chunk (allocated at first use)
    int rc;
    if ((rc = ensure_exact(c, c->actor_lw_arena, lw_arena_bytes(ch.actor_chunk), "the layer-wise ActorNet's arena"))) return rc;
    lw_build_plan(A, ch.actor_chunk, c->actor_lw_plan);
    u32 *arena = (u32 *)c->actor_lw_arena.p;
    const int nl = ch.np == 6 ? lw_run<6>(c->actor_lw_plan, p.st, arena, actors, actor_feat, c->W.actorB)
                 : ch.np == 3 ? lw_run<3>(c->actor_lw_plan, p.st, arena, actors, actor_feat, c->W.actorB)
                              : lw_run<1>(c->actor_lw_plan, p.st, arena, actors, actor_feat, c->W.actorB);
    if (nl < 0) return fail(c, MIND_ESTATE, "layer-wise ActorNet: a stage has no kernel");
    c->last_actor_lw = 1; c->last_actor_launches = nl; c->last_actor_chunks = ch.actor_chunks;
    break;
  }
  default:
    if (ch.np == 6) hipLaunchKernelGGL(k_actor_mfma<6>, grid, dim3(AM_T), mind_actor_mfma_lds_bytes(), p.st, actors, A, actor_feat, c->W.actorB, clk);
    else if (ch.np == 3) hipLaunchKernelGGL(k_actor_mfma<3>, grid, dim3(AM_T), mind_actor_mfma_lds_bytes(), p.st, actors, A, actor_feat, c->W.actorB, clk);
    else hipLaunchKernelGGL(k_actor_mfma<1>, grid, dim3(AM_T), mind_actor_mfma_lds_bytes(), p.st, actors, A, actor_feat, c->W.actorB, clk);
  }
  return MIND_OK;
}

// encoders: ActorNet on the context stream, the (independent) lane encoders and token positions beside it on the side stream (everything
// they read was complete at the last synchronisation point), then the target polyline's encoder + embedding
static int pred_encoders(PredCall &p) {
  mind_ctx *c = p.c;
  const mind_scene_batch *in = p.in;
  hipStream_t st = p.st, ss = p.ss;
  const int Bn = p.Bn, Ltot = p.Ltot, ntok = p.ts->ntok;
  if (c->side) {
    // the side stream reads inputs the caller produced on the context stream (uploads, mind_aime_rebase outputs): it starts
    // behind everything queued there so far (a table-cache hit no longer synchronises the stream on the way in)
    HIPCHK(c, hipEventRecord(c->ev_main, st));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
  }
  const bool act_timed = c->profiling && !c->ev_defer;      // (inside a plan nothing drains the stream per call: no ActorNet time there)
  // the one-launch forms by the launch clock; the layer-wise form (a dozen launches per chunk) stays on its two events
  int rc;
  LcSlot *act_clk = nullptr;
  if (act_timed && lc_on(c) && p.ch.actor_form != PRED_ACTOR_LW) {
    if ((rc = lc_reserve(c, 1, p.ch.actor_grid))) return rc;
    act_clk = lc_take(c, p.ch.actor_grid, LC_ACTOR);
  }
  p.act_ev = act_timed && (lc_events(c) || !act_clk);
  if (p.act_ev && !c->ev_act0) {
    HIPCHK(c, c->ev_act0.create());
    HIPCHK(c, c->ev_act1.create());
  }
  c->last_actor_lw = 0; c->last_actor_launches = 1; c->last_actor_chunks = 1; c->actor_ms = 0.f;
  if (p.act_ev) HIPCHK(c, hipEventRecord(c->ev_act0, st));
  if ((rc = pred_actor_net(p, act_clk))) return rc;
  if (p.act_ev) HIPCHK(c, hipEventRecord(c->ev_act1, st));
  // (a plan's own work for the side stream, launched behind ActorNet: in front of the lane encoders here, behind the target embedding below)
  if (c->enc_pre) {
    const std::function<int(hipStream_t)> pre = std::move(c->enc_pre);
    c->enc_pre = nullptr;
    if ((rc = pre(ss))) return rc;
  }
  p.lane_feat = in->lane_feat;
  if (!p.lane_feat) {
    float *lf = p.out->lane_feat ? p.out->lane_feat : (float *)c->lane_feat.p;
    if (Ltot > 0)
      hipLaunchKernelGGL(k_lane_net, dim3((Ltot + PL - 1) / PL), dim3(DT), 0, ss, in->lanes, Ltot, lf, c->W.lane);
    p.lane_feat = lf;
  } else if (p.out->lane_feat && p.out->lane_feat != in->lane_feat && Ltot > 0) {
    HIPCHK(c, hipMemcpyAsync(p.out->lane_feat, in->lane_feat, (size_t)Ltot * 128 * sizeof(float), hipMemcpyDeviceToDevice, ss));
  }
  hipLaunchKernelGGL(k_tokpos, dim3((ntok + 255) / 256), dim3(256), 0, ss, (const TokMeta *)p.ts->meta.p, ntok, in->actor_ctrs, in->actor_vecs,
                     in->lane_ctrs, in->lane_vecs, (float *)c->tokpos.p);
  if (c->side) {
    HIPCHK(c, hipEventRecord(c->ev_side, c->side));
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_side, 0));
  }
  // the target polyline's encoder + embedding feed the decoder only: they stay on the side stream while the fusion layers run
  hipLaunchKernelGGL(k_lane_net, dim3((Bn + PL - 1) / PL), dim3(DT), 0, ss, in->tgt_nodes, Bn, (float *)c->tgt_feat.p, c->W.lane);
  hipLaunchKernelGGL(k_dec_tgt, dim3(Bn), dim3(DT), mind_dec_scene_lds_bytes(), ss, (const float *)c->tgt_feat.p, in->tgt_rpe, (float *)c->tgt_emb.p,
                     c->W.dec);
  if (c->enc_post) {
    const std::function<int(hipStream_t)> post = std::move(c->enc_post);
    c->enc_post = nullptr;
    if ((rc = post(ss))) return rc;
  }
  if (c->side) HIPCHK(c, hipEventRecord(c->ev_tgt, c->side));
  if (p.ch.tgt_wait_first) HIPCHK(c, hipStreamWaitEvent(st, c->ev_tgt, 0));
  return MIND_OK;
}

// timing events are made when first needed: `v` grown to n of them
static hipError_t ev_grow(std::vector<Event> &v, size_t n) {
  hipError_t rc = hipSuccess;
  for (Event e; v.size() < n && (rc = e.create()) == hipSuccess;) v.push_back(std::move(e));
  return rc;
}

// (HIP events around every token launch with profiling on, outside a plan: mind_last_token_stats / mind_last_token_stage_ms)
static hipError_t pred_tok_mark(PredCall &p, int tag) {
  mind_ctx *c = p.c;
  if (!p.tok_timed) return hipSuccess;
  if (p.ev_tok_used == c->ev_tok.size()) {
    const hipError_t rc_ = ev_grow(c->ev_tok, p.ev_tok_used + 1);
    if (rc_ != hipSuccess) return rc_;
    c->ev_tok_tag.push_back(0);
  }
  c->ev_tok_tag[p.ev_tok_used] = tag;
  return hipEventRecord(c->ev_tok[p.ev_tok_used++], p.st);
}

// one token step (init, or the epilogue of fusion layer Lw - 1 + the prologue of layer Lw): every run in its class's kernel
static int pred_token_step(PredCall &p, int mode, int Lw) {
  mind_ctx *c = p.c;
  hipStream_t st = p.st;
  const size_t qk_stride = p.ch.qk_stride, tokm_lds = mind_token_mfma_lds_bytes();
  const float *actor_feat = (const float *)c->actor_feat.p, *lane_feat = p.lane_feat;
  float *part = (float *)c->part.p;
  HIPCHK(c, pred_tok_mark(p, -1));
  for (const PredTokRun &r : p.ch.tok_runs) {
    const TokMeta *m_ = (const TokMeta *)p.ts->meta.p + r.t0;
    float *x_ = p.x() + (size_t)r.t0 * 128, *ST_ = (float *)c->ST.p + (size_t)r.t0 * 256, *QK_ = (float *)c->QK.p + (size_t)r.t0 * qk_stride;
    if (r.layerwise) {
      tl_build_plan(r.n, mode, p.ch.tok_chunk, c->n_cu, c->tok_lw_plan);
      for (const TlLaunch &L : c->tok_lw_plan) {
        if (tl_launch(L, st, mode, m_, actor_feat, lane_feat, x_, part, ST_, QK_, qk_stride, c->W.tok[Lw], c->W.tokM[Lw], (float *)c->tok_lw_arena.p, p.ch.tok_chunk))
          return fail(c, MIND_ESTATE, "layer-wise token stage: a stage has no kernel");
        HIPCHK(c, pred_tok_mark(p, L.stage));
      }
      c->last_tok_launches += (int)c->tok_lw_plan.size();
      continue;
    }
    c->last_tok_launches++;
    if (r.kind == 0) {
      const int tpw = r.form == PRED_TOK_S2 ? 2 : r.small ? TOK_TPW_SMALL : TOK_TPW_BIG;
      auto *kern = r.small ? (r.merged ? k_token_m : k_token<TOK_TPW_SMALL>) : k_token<TOK_TPW_BIG>;
      if (r.form == PRED_TOK_S2 || r.form == PRED_TOK_S4) {
        // the small-launch form is compiled per shape of the step: first (1 | 4), between two layers (2 | 4), last (2)
        const bool two = r.form == PRED_TOK_S2;
        switch (mode & 7) {
          case 5: kern = two ? k_token_s<2, 5> : k_token_s<TOK_TPW_SMALL, 5>; break;
          case 6: kern = two ? k_token_s<2, 6> : k_token_s<TOK_TPW_SMALL, 6>; break;
          case 2: kern = two ? k_token_s<2, 2> : k_token_s<TOK_TPW_SMALL, 2>; break;
          default: return fail(c, MIND_ESTATE, "token step: mode %d has no small-launch kernel", mode);
        }
      }
      hipLaunchKernelGGL(kern, dim3((r.n + tpw - 1) / tpw), dim3(TT_THREADS), 0, st, m_, r.n, mode, actor_feat, lane_feat, x_, part, ST_, QK_, c->W.tok[Lw]);
    } else if (r.kind == 1) {
      hipLaunchKernelGGL(k_token_mfma<0>, dim3((r.n + TM_TOK - 1) / TM_TOK), dim3(TM_THREADS), tokm_lds, st, m_, r.n, mode, actor_feat, lane_feat, x_,
                         part, ST_, QK_, c->W.tok[Lw], c->W.tokM[Lw]);
    } else {
      hipLaunchKernelGGL(k_token_mfma<1>, dim3((r.n + TM_TOK - 1) / TM_TOK), dim3(TM_THREADS), tokm_lds, st, m_, r.n, mode, actor_feat, lane_feat, x_,
                         part, ST_, QK_, c->W.tok[Lw], c->W.tokB[Lw]);
    }
    HIPCHK(c, pred_tok_mark(p, TL_NSTAGE));
  }
  return MIND_OK;
}

// one fusion layer's pair kernel: layer 0 is the MODE 0 instance of its family, the last layer projects with its edge weights
static int pred_pair_layer(PredCall &p, int L) {
  mind_ctx *c = p.c;
  const PredChoice &ch = p.ch;
  const TableSet *ts = p.ts;
  const bool last = L == 5, own5 = last && ch.l5_jobs5;
  const int um = L < 4 ? 0 : (L == 4 ? 1 : 2);
  const PairJob *jl = (const PairJob *)(own5 ? ts->jobs5.p : ts->jobs.p);
  const int nj = own5 ? ts->njobs5 : ts->njobs;
  const dim3 grid(pair_grid(nj, c->n_cu)), block(PAIR_THREADS);
  float *edge = (float *)c->edge.p, *ST = (float *)c->ST.p, *QK = (float *)c->QK.p, *part = (float *)c->part.p, *tokpos = (float *)c->tokpos.p;
  const size_t ldsb = mind_pair_bf_lds_bytes();
  const u32 *we = c->W.pair.WBe[L], *wp = last ? c->W.pair.WBe[L] : c->W.pair.WBp[L];
  LcSlot *clk = p.pair_clk ? lc_take(c, (int)grid.x, LC_PAIR) : nullptr;      // (room was made in pred_fusion)
  if (p.pair_ev) HIPCHK(c, hipEventRecord(p.evs[2 * L], p.st));
#define PAIR_GO(K0, K1, LDS, ...)                                                                                                             \
  do {                                                                                                                                        \
    if (L == 0) hipLaunchKernelGGL(K0, grid, block, LDS, p.st, jl, nj, edge, ST, QK, part, __VA_ARGS__, c->W.pair.vtab[L], c->W.pair.rtab, tokpos, p.rpe_dev, um, clk); \
    else hipLaunchKernelGGL(K1, grid, block, LDS, p.st, jl, nj, edge, ST, QK, part, __VA_ARGS__, c->W.pair.vtab[L], c->W.pair.rtab, tokpos, p.rpe_dev, um, clk);   \
  } while (0)
  switch (ch.pair_family) {
  case PRED_PAIR_F32: PAIR_GO((k_pair<0>), (k_pair<1>), mind_pair_lds_bytes(), c->W.pair.WAe[L], last ? c->W.pair.WAe[L] : c->W.pair.WAp[L]); break;
  case PRED_PAIR_T6: PAIR_GO((k_pair_t6<0>), (k_pair_t6<1>), ldsb, we, wp, c->W.pair.WLe[L], last ? c->W.pair.WLe[L] : c->W.pair.WLp[L]); break;
  case PRED_PAIR_T:
    if (ch.pair_np == 3) PAIR_GO((k_pair_t<0, 3>), (k_pair_t<1, 3>), ldsb, we, wp);
    else PAIR_GO((k_pair_t<0, 1>), (k_pair_t<1, 1>), ldsb, we, wp);
    break;
  default:
    if (ch.pair_np == 3) PAIR_GO((k_pair_bf<0, 3>), (k_pair_bf<1, 3>), ldsb, we, wp);
    else PAIR_GO((k_pair_bf<0, 1>), (k_pair_bf<1, 1>), ldsb, we, wp);
  }
#undef PAIR_GO
  if (p.pair_ev) HIPCHK(c, hipEventRecord(p.evs[2 * L + 1], p.st));
  c->n_pair_launch++;
  c->pairs_done += last ? ts->pairs_l5 : ts->pairs_full;
  return MIND_OK;
}

// fusion: init tokens + 6 x (pair kernel, token kernel)
static int pred_fusion(PredCall &p) {
  mind_ctx *c = p.c;
  const PredChoice &ch = p.ch;
  const TableSet *ts = p.ts;
  int rc;
  c->last_tok_lw = ch.tok_lw; c->last_tok_launches = 0; c->last_tok_chunks = ch.last_tok_chunks; c->tok_ms = 0.f;
  for (float &v : c->tok_stage_ms) v = 0.f;
  if (ch.tok_lw && (rc = ensure_exact(c, c->tok_lw_arena, tl_arena_bytes(ch.tok_chunk), "the layer-wise token stage's arena"))) return rc;
  p.tok_timed = c->profiling && !c->ev_defer;
  if ((rc = pred_token_step(p, 1 | 4 | ch.qsplit, 0))) return rc;
  c->n_pair_launch = 0;
  c->pairs_done = 0;
  // the pair layers' timing: blocks of the launch clock's ring ("prof_clock" 1, 2), HIP events around every launch ("prof_clock" 0, 2)
  p.pair_clk = lc_on(c);
  p.pair_ev = lc_events(c);
  if (p.pair_clk && (rc = lc_reserve(c, c->debug_layers, std::max(pair_grid(ts->njobs, c->n_cu), pair_grid(ts->njobs5, c->n_cu))))) return rc;
  if (p.pair_ev) HIPCHK(c, ev_grow(c->ev, 12));
  p.evs = c->ev.data();
  if (p.pair_ev && c->ev_defer) {
    HIPCHK(c, ev_grow(c->ev_pool, c->ev_pool_used + 12));
    p.evs = c->ev_pool.data() + c->ev_pool_used;
    c->ev_pending.push_back(c->ev_pool_used);
    c->ev_pool_used += 12;
  }
  c->last_ntok = ts->ntok; c->last_edge_pairs = ts->edge_pairs; c->last_slots = ts->slot; c->last_A = p.A; c->last_B = p.Bn;
  c->last_scene_n = ts->scene_n; c->last_edge_tiled = ch.tiled; c->last_edge_bf16 = ch.edge_bf16;
  for (int L = 0; L < c->debug_layers; ++L) {
    if ((rc = pred_pair_layer(p, L))) return rc;
    if ((rc = pred_token_step(p, 2 | (L < 5 ? 4 : 8) | ch.qsplit, L + 1))) return rc;
  }
  return MIND_OK;
}

// the decoder's scene part as the launch chain k_dec_chain1..4 with G workgroups per scene (dec_chain.h), queued on st: x's cls rows -> the mode
// tokens Cout [Bn,6,128] and the mode probabilities cls [Bn,6].  The buffer the kernels hand their intermediate rows through is sized once for
// every call that takes the chain by rule (n_cu / 8 scenes); only mind_debug_dec_scene asks for more.
static int dec_chain_run(mind_ctx *c, int G, int Bn, const float *x, const int *d_cls_row, float *Cout, float *cls, hipStream_t st) {
  if (!dc_valid_g(G) || Bn <= 0) return fail(c, MIND_EINVAL, "decoder chain: %d workgroups per scene, %d scenes", G, Bn);
  int rc;
  if ((rc = ensure(c, c->dec_chain, (size_t)std::max(Bn, c->n_cu / 8) * DC_SCENE_FLOATS * sizeof(float)))) return rc;
  float *buf = (float *)c->dec_chain.p;
  const size_t lds = mind_dec_scene_lds_bytes();
#define DEC_CHAIN(GV)                                                                                                  \
  do {                                                                                                                 \
    hipLaunchKernelGGL(k_dec_chain1<GV>, dim3(Bn * GV), dim3(DT), lds, st, x, d_cls_row, buf, c->W.dec);                \
    hipLaunchKernelGGL(k_dec_chain2<GV>, dim3(Bn * GV), dim3(DT), lds, st, buf, c->W.dec);                              \
    hipLaunchKernelGGL(k_dec_chain3<GV>, dim3(Bn * GV), dim3(DT), lds, st, buf, c->W.dec);                              \
  } while (0)
  if (G == 32) DEC_CHAIN(32);
  else if (G == 16) DEC_CHAIN(16);
  else DEC_CHAIN(8);
#undef DEC_CHAIN
  hipLaunchKernelGGL(k_dec_chain4, dim3(Bn), dim3(DT), lds, st, (const float *)buf, Cout, cls, c->W.dec);
  return MIND_OK;
}

static int pred_decoder(PredCall &p) {
  mind_ctx *c = p.c;
  const PredChoice &ch = p.ch;
  mind_pred_out *out = p.out;
  hipStream_t st = p.st;
  const int A = p.A, Bn = p.Bn;
  const float *x = p.x();
  const int *d_actor_row = p.rows(), *d_actor_scene = d_actor_row + A, *d_cls_row = d_actor_row + 2 * A;
  const float *cmode = (const float *)c->cmode.p, *tgt_emb = (const float *)c->tgt_emb.p;
  const dim3 agrid((A + RA - 1) / RA), mgrid((A + DM_RA - 1) / DM_RA);
  // the aux outputs (mind_predict_batch_aux): the head of every form writes them itself when asked
  float *cov_vel = p.aux ? p.aux->cov_vel : nullptr, *param = p.aux ? p.aux->param : nullptr;
  int rc;
  if (ch.split_dec) {
    if ((rc = ensure(c, c->dec_h2, (size_t)A * 768 * sizeof(float)))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_main, st));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
    hipLaunchKernelGGL(k_dec_actor<1>, agrid, dim3(DT), mind_dec_actor_lds_bytes(), c->side, x, d_actor_row, d_actor_scene, A,
                       (const float *)nullptr, (const float *)nullptr, (float *)nullptr, (float *)nullptr, c->W.dec, (float *)c->dec_h2.p,
                       (float *)nullptr, (float *)nullptr);
    HIPCHK(c, hipEventRecord(c->ev_side, c->side));
  }
  // the scene part
  bool cls_on_side = false;
  bool mw = ch.want_mw;
  if (mw) {
    if (c->dec_abort && *c->dec_abort.as<volatile unsigned>()) return fail(c, MIND_EHIP, "k_dec_scene_mw: a barrier of an earlier launch timed out (launch not resident)");
    if (!c->dec_abort) {
      if (c->dec_abort.alloc(64, hipHostMallocMapped) != hipSuccess) mw = false;
      else *c->dec_abort.as<unsigned>() = 0u;
    }
    const size_t need_x = (size_t)(c->n_cu / DEC_MW_G) * 2 * 6 * 1536 * sizeof(float), need_b = (size_t)(c->n_cu / DEC_MW_G) * 4 * sizeof(unsigned);
    if (mw && c->dec_xbuf.cap < need_x) {
      if ((rc = ensure(c, c->dec_xbuf, need_x))) return rc;
    }
    if (mw && c->dec_bars.cap < need_b) {
      if ((rc = ensure(c, c->dec_bars, need_b))) return rc;
      HIPCHK(c, hipMemsetAsync(c->dec_bars.p, 0, c->dec_bars.cap, st));        // (once: the barrier resets its arrival count itself)
    }
  }
  if (ch.dec_chain_g) {
    if ((rc = dec_chain_run(c, ch.dec_chain_g, Bn, x, d_cls_row, (float *)c->cmode.p, out->cls, st))) return rc;
  } else if (mw)
    hipLaunchKernelGGL(k_dec_scene_mw,dim3(ch.mw_blocks), dim3(DT), mind_dec_scene_lds_bytes(), st, x, d_cls_row, (float *)c->cmode.p, out->cls, c->W.dec, Bn,
                       (float *)c->dec_xbuf.p, (unsigned *)c->dec_bars.p, c->dec_abort.as<unsigned>());
  else if (ch.cls_side) {
    // the mode tokens on the context stream, the mode probabilities (the cls head: ~10 us a launch) on the side stream beside the actor part's
    // head, which needs the tokens only; the caller's next work on the context stream follows both
    hipLaunchKernelGGL(k_dec_scene_c, dim3(Bn), dim3(DT), mind_dec_scene_lds_bytes(), st, x, d_cls_row, (float *)c->cmode.p, c->W.dec);
    HIPCHK(c, hipEventRecord(c->ev_main, st));
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
    hipLaunchKernelGGL(k_dec_cls, dim3(Bn), dim3(DT), mind_dec_scene_lds_bytes(), c->side, (float *)c->cmode.p, out->cls, c->W.dec);
    if (!c->ev_cls) HIPCHK(c, c->ev_cls.create(hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_cls, c->side));
    cls_on_side = true;
  } else
    hipLaunchKernelGGL(k_dec_scene, dim3(Bn), dim3(DT), mind_dec_scene_lds_bytes(), st, x, d_cls_row, (float *)c->cmode.p, out->cls, c->W.dec);
  if (c->side) HIPCHK(c, hipStreamWaitEvent(st, c->ev_tgt, 0));      // the decoder's actor part reads the target embedding
  // the actor part: the K-split fp32 kernel (a handful of workgroups, bound by the latency of one pass over the weights), its head behind the
  // side stream's half in the split form, or the MFMA kernel
  switch (ch.dec_actor) {
  case PRED_DEC_SPLIT:
    HIPCHK(c, hipStreamWaitEvent(st, c->ev_side, 0));
#define DEC_HEAD(RAV)                                                                                                                       \
  hipLaunchKernelGGL((k_dec_actor<2, RAV>), dim3((A + RAV - 1) / RAV), dim3(DT), mind_dec_actor_lds_bytes(), st, x, d_actor_row, d_actor_scene, A, \
                     cmode, tgt_emb, out->reg, out->vel, c->W.dec, (float *)c->dec_h2.p, cov_vel, param)
    if (ch.dec_head_ra == 1) DEC_HEAD(1);
    else if (ch.dec_head_ra == 2) DEC_HEAD(2);
    else DEC_HEAD(RA);
#undef DEC_HEAD
    break;
  case PRED_DEC_ONE:
    hipLaunchKernelGGL(k_dec_actor<0>, agrid, dim3(DT), mind_dec_actor_lds_bytes(), st, x, d_actor_row, d_actor_scene, A, cmode, tgt_emb, out->reg,
                       out->vel, c->W.dec, (float *)nullptr, cov_vel, param);
    break;
  default: {
#define DEC_MFMA(NPV)                                                                                                                     \
  hipLaunchKernelGGL(k_dec_actor_mfma<NPV>, mgrid, dim3(DM_T), mind_dec_actor_mfma_lds_bytes(), st, x, d_actor_row, d_actor_scene, A, cmode, \
                     tgt_emb, out->reg, out->vel, c->W.decB, cov_vel, param)
    if (ch.np == 6) DEC_MFMA(6);
    else if (ch.np == 3) DEC_MFMA(3);
    else DEC_MFMA(1);
#undef DEC_MFMA
  }
  }
  if (cls_on_side) HIPCHK(c, hipStreamWaitEvent(st, c->ev_cls, 0));      // whatever follows on the context stream sees the mode probabilities too
  return MIND_OK;
}

// debug taps (gather fused tokens), the launch errors of the call, and with profiling on outside a plan the events of its stages
static int pred_finish(PredCall &p) {
  mind_ctx *c = p.c;
  mind_pred_out *out = p.out;
  const float *x = p.x();
  for (int a = 0; a < p.A && out->actor_emb; ++a)
    HIPCHK(c, hipMemcpyAsync(out->actor_emb + (size_t)a * 128, x + (size_t)p.ts->actor_row[a] * 128, 128 * sizeof(float), hipMemcpyDeviceToDevice, p.st));
  for (int b = 0; b < p.Bn && out->cls_emb; ++b)
    HIPCHK(c, hipMemcpyAsync(out->cls_emb + (size_t)b * 128, x + (size_t)p.ts->cls_row[b] * 128, 128 * sizeof(float), hipMemcpyDeviceToDevice, p.st));
  HIPCHK(c, hipGetLastError());
  if (c->profiling && c->ev_defer) {
    c->pair_ms = 0.f;         // (read by mind_pair_events_resolve behind the plan's last synchronisation)
  } else if (c->profiling) {
    HIPCHK(c, hipStreamSynchronize(p.st));
    c->pair_ms = 0.f;
    for (int k : {LC_PAIR, LC_ACTOR}) { c->ev_last[k].clear(); c->lc_last[k].clear(); }
    for (int L = 0; L < c->debug_layers && p.pair_ev; ++L) {
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2 * L], c->ev[2 * L + 1]));
      c->pair_ms += ms;
      c->ev_last[LC_PAIR].push_back(ms);
    }
    if (p.act_ev) {
      HIPCHK(c, hipEventElapsedTime(&c->actor_ms, c->ev_act0, c->ev_act1));
      c->ev_last[LC_ACTOR].push_back(c->actor_ms);
    }
    if (lc_on(c)) {
      // the launch clock's records of this call, read behind the drained stream: its figures are the ones handed out
      double ms[LC_KINDS];
      int n[LC_KINDS], rc;
      if ((rc = lc_resolve(c, -1, 1u << LC_PAIR | 1u << LC_ACTOR, ms, n))) return rc;
      if (n[LC_PAIR] > 0) c->pair_ms = (float)ms[LC_PAIR];
      if (n[LC_ACTOR] > 0) c->actor_ms = (float)ms[LC_ACTOR];
    }
    for (size_t i = 1; i < p.ev_tok_used; ++i) {
      if (c->ev_tok_tag[i] < 0) continue;
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev_tok[i - 1], c->ev_tok[i]));
      c->tok_stage_ms[c->ev_tok_tag[i]] += ms;
      c->tok_ms += ms;
    }
  }
  return MIND_OK;
}

extern "C" int mind_predict_batch_aux(mind_ctx *c, const mind_scene_batch *in, mind_pred_out *out, const mind_pred_aux *aux) {
  if (!c || !in || !out) return MIND_EINVAL;
  if (!c->have_weights) return fail(c, MIND_ESTATE, "weights not loaded");
  const int Bn = in->n_scenes;
  if (Bn <= 0 || !in->actor_off || !in->lane_off || !in->actors || !in->tgt_nodes || !in->tgt_rpe || !out->cls ||
      !out->reg || !out->vel)
    return fail(c, MIND_EINVAL, "null input/output pointer");
  if (!in->lanes && !in->lane_feat) return fail(c, MIND_EINVAL, "need lanes or lane_feat");
  if (!in->rpe && !(in->actor_ctrs && in->actor_vecs && in->lane_ctrs && in->lane_vecs))
    return fail(c, MIND_EINVAL, "need rpe or ctrs/vecs");
  HIPCHK(c, hipSetDevice(c->device));
  const int A = in->actor_off[Bn], Ltot = in->lane_off[Bn];
  if (A <= 0 || Ltot < 0) return fail(c, MIND_EINVAL, "empty batch");
  std::vector<int> sa(Bn), sl(Bn);      // actors, lanes per scene
  for (int b = 0; b < Bn; ++b) {
    sa[b] = in->actor_off[b + 1] - in->actor_off[b]; sl[b] = in->lane_off[b + 1] - in->lane_off[b];
    if (sa[b] <= 0 || sl[b] < 0) return fail(c, MIND_EINVAL, "scene %d has %d agents, %d lanes", b, sa[b], sl[b]);
  }
  const PredChoice ch = pred_choose(c->pt, c->pair_prec, c->n_cu, c->side.p != nullptr, Bn, sa.data(), sl.data(), c->debug_tok_form);
  PredCall p{c, in, out, aux, ch, Bn, A, Ltot, c->stream, c->side ? c->side.p : c->stream};
  int rc;
  if ((rc = pred_tables(p, sa.data(), sl.data()))) return rc;
  if ((rc = pred_workspaces(p))) return rc;
  if ((rc = pred_encoders(p))) return rc;
  if ((rc = pred_fusion(p))) return rc;
  if ((rc = pred_decoder(p))) return rc;
  return pred_finish(p);
}

extern "C" int mind_predict_batch(mind_ctx *c, const mind_scene_batch *in, mind_pred_out *out) { return mind_predict_batch_aux(c, in, out, nullptr); }
