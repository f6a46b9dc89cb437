// Every tuning knob of the library, declared once: the three records the hot paths read as plain fields (PredTuning, IlqrTuning, CtxTuning)
// and one table with a row per knob -- its mind_set_tuning name, its environment variable (or none), its record and field, the rule that
// turns an int into the stored value and the rule that reads the variable's text (both plain functions).  tn_set, tn_get and tn_apply_env are the only code that
// looks a knob up by name: mind_set_tuning, mind_get_tuning, mind_ctx_create and the two debug entries that take knob lists call them.
// Defaults are the field initialisers.  No HIP call, no context: compiles alone with the host compiler; tests read it through mind_debug_tuning.
#pragma once
#include <cstdlib>
#include <cstring>

#define TN_RA 4           // RA (encdec_kernels.hip) and IL_SLOTS (ilqr_kernels.hip), which two clamps need: mind_hip.hip static_asserts them
#define TN_IL_SLOTS 12

struct PredTuning {
  // bf16 arithmetics: k_pair_t (tile-native edge tensor, pair_tile_kernels.hip; default) or the row-major k_pair_bf of rounds 2-3
  // (mind_set_tuning("pair_tile", 0) / MIND_PAIR_TILE=0, kept for same-box A/B measurements)
  bool pair_tile = true;
  bool xcd_order = true;        // XCD-aware job order for big batches (MIND_XCD_ORDER=0 switches it off, for A/B measurements)
  bool enc_mfma = true;         // MFMA ActorNet under the bf16x3 / bf16 settings (MIND_ENC_MFMA=0: the fp32 VALU kernel, for A/B)
  int actor_np = 6;             // partial products per term of the MFMA ActorNet under bf16x3: 6 (three-way split, fp32-class) or 3 (MIND_ACTOR_SPLIT=3)
  // fp32-MFMA ActorNet (k_actor_f32): "actor_f32" 1 (default) = the ActorNet of the exact-fp32 setting (0: the fp32 VALU kernel, for A/B);
  // "actor_f32_min" = actors per call from which every setting takes it with TWO actors per workgroup (the 256-channel layers' weight stream is
  // then shared by two actors: 7.1 vs 8.1 ms for the 13.8 k actors of a cfg4 round); "actor_f32_pair_min" = the same threshold inside the
  // exact-fp32 setting.  Both default to never: a threshold on the batch size would give the blocks of a sharded round another kernel -- other
  // last bits -- than the whole round (a workload that wants it sets 0, as with "dec_mfma_min")
  bool actor_f32 = true;
  int actor_f32_min = 1 << 30, actor_f32_pair_min = 1 << 30;
  // layer-wise batched ActorNet (actor_lw_kernels.hip): actors per call from which it replaces k_actor_mfma<NP> ("actor_lw_min" /
  // MIND_ACTOR_LW_MIN; default never; bit-identical, so ranks and rounds may differ in which one they take), actors per chunk
  // ("actor_lw_chunk", 0 = LW_CHUNK; tests and A/B runs)
  int actor_lw_min = 1 << 30, actor_lw_chunk = 0;
  // token kernel on the fp32 MFMA (k_token_mfma; MIND_TOK_MFMA=1 / mind_set_tuning("tok_mfma")).  Opt-in: measured on the MI355X it is
  // SLOWER than the VALU kernel -- 41 vs 30 us per launch at demo size (6 workgroups), 315 vs 282 us average on the full cfg4 tree
  // (profiles/r03o_*, r03p_*): 640 fp32 MFMAs of 32 cycles per wave and launch are 8.5 us by themselves and the weight stream (64 KB per
  // projection and workgroup) is the same; a bf16-split variant would cut the MFMA time, not the rest
  bool tok_mfma = false;
  // scenes of at least this many tokens run k_token_mfma<1> (bf16 hi + lo split operands) under the bf16 arithmetics ("tok_bf_min_n";
  // 0 = never, the default).  Measured on the cfg4 full tree (N = 321, launches of up to 69 k tokens): 221 us per launch on average and
  // 0.80 ms for the largest, the same as the VALU kernel (which is LDS-bound there) -- with 97 KB of LDS the MFMA kernel keeps one
  // four-wave workgroup per CU and waits on its partial-sum and fragment loads instead (profiles/r03bb); opt-in until it is faster
  int tok_bf_min_n = 0;
  // layer-wise token stage (token_lw_kernels.hip; the bits of k_token_mfma<0>).  "tok_lw_min_n" / MIND_TOK_LW_MIN_N: a SCENE of at least this
  // many tokens takes the fp32-MFMA token class (by the scene's own N: its result does not depend on its batch, round or rank); "tok_lw_min" /
  // MIND_TOK_LW_MIN: a run of consecutive scenes of that class with at least this many tokens runs layer-wise, a shorter one k_token_mfma<0>
  // (the same bits, so this rule may look at the batch).  Both default to never.  "tok_lw_chunk": tokens per chunk (0 = TL_CHUNK)
  int tok_lw_min_n = 1 << 30, tok_lw_min = 1 << 30, tok_lw_chunk = 0;
  bool tok_merge = true;        // small token launches merge their independent projections (k_token_m; MIND_TOK_MERGE=0 / "tok_merge": the plain kernel)
  int tok_small_max = 2048;     // batches of at most this many tokens run k_token with 4 tokens per workgroup ("tok_small_max")
  int dec_mfma_min = 1 << 30;   // agents per call from which the decoder's actor part runs on the MFMA kernel (MIND_DEC_MFMA_MIN; default: never)
  bool dec_overlap = true;      // actor_proj of the decoder on the side stream beside k_dec_scene (mind_set_tuning("dec_overlap"))
  // agents per workgroup of the split decoder's head, k_dec_actor<2, .> ("dec_head_ra"): 0 (default) = by the call's agents -- 1 while they fit
  // one workgroup per CU, else 2, else RA = 4; 1, 2 or 4 = that form whatever the call (4: the head as it was).  The forms give the same bits,
  // so the rule may look at the batch
  int dec_head_ra = 0;
  // k_dec_scene_mw: eight workgroups per scene on the decoder's five big stages (bit-identical to the one-workgroup kernel), possible whenever
  // every workgroup of the launch is resident, i.e. for calls of at most n_cu / 8 scenes.  Opt-in ("dec_mw" / MIND_DEC_MW=1): measured 88.6
  // against 94.9 us per demo-size launch (profiles/r06aa_*) -- only ctx_proj's second layer is really bound by one CU's L2 port (30 k -> 20 k
  // cycles); the feed-forward layers are bound by their 24 accumulators per thread and win 2-4 k cycles each, less the 36 KB exchange --
  // 12 us per plan, not worth eight spinning workgroups per scene when several scenes share the device.
  // With this knob and "dec_cls_side" off, calls of at most n_cu / 8 scenes take the launch chain k_dec_chain1..4 by rule instead (dec_chain.h,
  // PredChoice::dec_chain_g: the same stages dealt over 32 / 16 / 8 workgroups per scene and over rows, a kernel boundary where this form
  // spins -- the same bits); either knob keeps the one-launch kernels, which are then the reference forms the chain is tested against
  bool dec_mw = false;
  // the decoder's cls head as its own launch on the side stream beside the actor part's head ("dec_cls_side" / MIND_DEC_CLS_SIDE=1).  Opt-in:
  // bit-identical, but the second launch and its two event waits cost more than the ~10 us of overlap (1 609-1 630 against 1 632-1 652
  // sim steps/s, profiles/r06am_*)
  bool dec_cls_side = false;
  bool tgt_side = true;         // the target polyline's encoder + embedding stay on the side stream through the fusion layers ("tgt_side")
};

struct IlqrTuning {
  // nodes per forward step of a narrow tree's line search ("ilqr_chunk"; 0: whole segments, the default).  Measured on the recorded
  // demo_1 loop: chunks of 6 / 8 / 12 nodes cost 2.10 / 2.05 / 2.04 ms per launch against 1.99 for whole segments (round 3: the cost
  // waves shared the SIMDs' float64 pipe with five state-chain waves); with the chains of a level packed into ONE wave and the cost
  // chunks kept off its SIMD (round 4) still 2.12 / 2.00 / 2.02 against 1.89: every extra forward step pays a rollout prologue (parent
  // state, first operands: two dependent round trips) and a barrier, more than the shorter cost tail saves (profiles/r04x_*)
  int ilqr_chunk = 0;
  // wide cost trees: workgroups per tree (halved until every workgroup of the launch is resident; cfg4 full tree, six trees per launch:
  // 8.33 / 7.40 / 7.37 / 7.63 ms per plan with 8 / 16 / 24 / 32, profiles/r03an), node count from which they are used (mind_set_tuning)
  int ilqr_wgs = 16, ilqr_multi_min = 192, ilqr_wgs_big = 32, ilqr_big_min = 12288;
  // narrow cost trees (below ilqr_multi_min nodes): workgroups per tree that take the fit's Levenberg-Marquardt slots (k_ilqr<GEN, 2>: a master +
  // ilqr_slots - 1 followers, one slot each; 1 = everything in one workgroup).  "ilqr_slots" / MIND_ILQR_SLOTS
  int ilqr_slots = 10;
  // ... and one more workgroup per tree that differentiates a pass's first candidate while the master prices the candidates (il_speculate; the
  // master swaps derivative sets instead of running its derivative pass when that candidate is the accepted one).  "ilqr_spec_deriv" / MIND_ILQR_SPEC_DERIV
  bool ilqr_spec_deriv = true;
  // tree-iLQR launches of at most this many nodes in all write their results (xs, us, statistics) to the host staging themselves at the kernel's
  // end instead of two copies behind it (0 = always copies).  "ilqr_host_out_max" / MIND_ILQR_HOST_OUT_MAX
  long ilqr_host_out_max = 4096;
  // candidates per workgroup of a scoring launch (k_ilqr_score; a power of two 1 .. 64, 0 = il_score_block decides).  Same bits for every
  // value.  "ilqr_score_block"
  int ilqr_score_block = 0;
  // tests: launch a wide tree without its last workgroups / let the followers of a narrow tree leave at once
  bool ilqr_test_starve = false;
};

// the knobs of the context itself: the planning cycle's transport and bookkeeping choices, none of which changes a result
struct CtxTuning {
  // mind_aime_plan: a round whose edge tensor would exceed this many MB goes through the predictor in chunks of scenes ("plan_chunk_mb";
  // 96 GB by default: a third of the MI355X's HBM; the scenes of a round are independent, so chunking changes nothing but the launch sizes)
  int plan_chunk_mb = 96 * 1024;
  // "pl_tab_side" / MIND_PL_TAB_SIDE=1: the round tables travel on their own stream while the round's predictor runs instead of behind it
  // on the context stream.  Measured on the recorded demo_1 loop: no difference (AIME 2.00 vs 2.01 ms per plan, profiles/r03ag) -- off.
  bool pl_tab_side = false;
  // the scene tables of a round of at most AIME_SMALL scenes per chunk travel in the glue kernels' arguments (no upload between the
  // predictor and k_aime_world).  "tab_small" / MIND_TAB_SMALL
  bool tab_small = true;
  // the plan's small index tables (the branch set of a round, the job tables of the two packing kernels) are read by the kernels from the
  // page-locked staging directly while they name at most this many workgroups (0 = always uploaded).  "tab_host_max" / MIND_TAB_HOST_MAX
  int tab_host_max = 4096;
  // mind_loop: price a candidate tree as soon as the pending tree-iLQR launch marks it complete, beside the trees still being solved.  "early_eval" / MIND_EARLY_EVAL
  bool early_eval = true;
  // mind_aime_plan, unsharded: the pruning decisions + branch-time bits of a round come from one launch (k_aime_select_branch) instead of two.  "glue_fused" / MIND_GLUE_FUSED
  bool glue_fused = true;
  // ... and k_aime_branch writes a round's decisions to the host staging itself (no copy behind it).  "dec_mirror" / MIND_DEC_MIRROR
  bool dec_mirror = true;
  // ... and that kernel marks the mirrored decisions complete (a generation word behind them, counted in by its blocks on pl_cnt): the host
  // polls the word instead of draining the stream and sizes the next round's buffers while it waits (unchunked rounds).  "dec_poll" / MIND_DEC_POLL
  bool dec_poll = true;
  // ... and what a round queues beside ActorNet -- the root's lane graph, world-frame histories and lane-distance field ("root_head" / MIND_ROOT_HEAD), a
  // later round's repeated lane features ("round_head" / MIND_ROUND_HEAD), the frames' read-back -- is handed to the round's first predictor call (mind_ctx::enc_pre)
  bool root_head = true, round_head = true;
  // uploads of at most this many bytes from the context's page-locked staging run as a kernel on the consumer's queue (pl_upload; 0 = always
  // hipMemcpyAsync).  "upload_kernel_max" / MIND_UPLOAD_KERNEL_MAX
  int upload_kernel_max = 1 << 20;
  // the launch clock (launch_clock.h, predict.hip): "prof_clock" / MIND_PROF_CLOCK 1 (default) = with profiling on, the kernels that take a slot
  // pointer (the pair kernels, k_actor_mfma) are timed by stamps of their own workgroups and no HIP event is recorded around them; 0 = HIP
  // events as before; 2 = both on the same launches (the cross-check: mind_debug_launch_times)
  int prof_clock = 1;
};

// whichever records a caller may set: a null pointer makes its rows unknown names (mind_debug_predict_choice passes its PredTuning alone)
struct TnRefs { PredTuning *pt = nullptr; IlqrTuning *it = nullptr; CtxTuning *ct = nullptr; };

// the rule that turns an int into the stored value (a flag stores 0 / 1)
static inline int tn_any(int v) { return v; }
static inline int tn_flag(int v) { return v != 0; }
static inline int tn_min0(int v) { return v < 0 ? 0 : v; }
static inline int tn_min1(int v) { return v < 1 ? 1 : v; }
static inline int tn_1_32(int v) { return v < 1 ? 1 : (v > 32 ? 32 : v); }
static inline int tn_slots(int v) { return v < 1 ? 1 : (v > TN_IL_SLOTS ? TN_IL_SLOTS : v); }
static inline int tn_0_2(int v) { return v < 0 ? 0 : (v > 2 ? 2 : v); }
static inline int tn_split(int v) { return v == 3 ? 3 : 6; }
static inline int tn_head_ra(int v) { return (v == 1 || v == 2 || v == TN_RA) ? v : 0; }
static inline int tn_pow2_64(int v) { int s = 0; for (int b = 1; b <= 64 && v > 0; b <<= 1) if (b <= v) s = b; return s; }      // the largest power of two <= min(v, 64)
// the rule that turns the variable's text into that int; false: the text leaves the knob alone.  The two flag readings differ on "", "00", "x",
// "-0", ...: each knob keeps the one it was introduced with
static inline bool tn_atoi(const char *s, int *v) { *v = atoi(s); return true; }
static inline bool tn_flag_char(const char *s, int *v) { *v = !(s[0] == '0'); return true; }
static inline bool tn_flag_atoi(const char *s, int *v) { *v = atoi(s) != 0; return true; }
static inline bool tn_positive(const char *s, int *v) { *v = atoi(s); return *v > 0; }

// One row per knob.  env, text: null for a knob without a variable.  io: the row's field in its record -- stores *v when `set`, then reads it
// back into *v; false when `r` lacks the record
struct TnRow {
  const char *name, *env;
  int (*rule)(int);
  bool (*text)(const char *, int *);
  bool (*io)(const TnRefs &r, bool set, int *v);
};
template <class T> static inline bool tn_io(T *f, bool set, int *v) { if (f && set) *f = (T)*v; if (f) *v = (int)*f; return f != nullptr; }
#define TN(rec, name, env, field, rule, text) {name, env, rule, text, [](const TnRefs &r, bool set, int *v) { return tn_io(r.rec ? &r.rec->field : nullptr, set, v); }}

static const TnRow TN_TABLE[] = {
    TN(pt, "dec_mfma_min", "MIND_DEC_MFMA_MIN", dec_mfma_min, tn_any, tn_atoi),
    TN(pt, "enc_mfma", "MIND_ENC_MFMA", enc_mfma, tn_flag, tn_flag_char),
    TN(pt, "actor_f32", "MIND_ACTOR_F32", actor_f32, tn_flag, tn_flag_char),
    TN(pt, "actor_f32_min", "MIND_ACTOR_F32_MIN", actor_f32_min, tn_any, tn_atoi),
    TN(pt, "actor_f32_pair_min", nullptr, actor_f32_pair_min, tn_any, nullptr),
    TN(pt, "actor_lw_min", "MIND_ACTOR_LW_MIN", actor_lw_min, tn_any, tn_atoi),
    TN(pt, "actor_lw_chunk", nullptr, actor_lw_chunk, tn_min0, nullptr),
    TN(pt, "actor_split", "MIND_ACTOR_SPLIT", actor_np, tn_split, tn_atoi),
    TN(pt, "xcd_order", "MIND_XCD_ORDER", xcd_order, tn_flag, tn_flag_char),
    TN(pt, "pair_tile", "MIND_PAIR_TILE", pair_tile, tn_flag, tn_flag_char),
    TN(pt, "dec_overlap", "MIND_DEC_OVERLAP", dec_overlap, tn_flag, tn_flag_char),
    TN(pt, "dec_head_ra", "MIND_DEC_HEAD_RA", dec_head_ra, tn_head_ra, tn_atoi),
    TN(pt, "tok_mfma", "MIND_TOK_MFMA", tok_mfma, tn_flag, tn_flag_char),
    TN(pt, "tok_small_max", "MIND_TOK_SMALL_MAX", tok_small_max, tn_any, tn_atoi),
    TN(pt, "tok_merge", "MIND_TOK_MERGE", tok_merge, tn_flag, tn_flag_char),
    TN(pt, "dec_mw", "MIND_DEC_MW", dec_mw, tn_flag, tn_flag_char),
    TN(pt, "dec_cls_side", "MIND_DEC_CLS_SIDE", dec_cls_side, tn_flag, tn_flag_char),
    TN(pt, "tok_bf_min_n", "MIND_TOK_BF_MIN_N", tok_bf_min_n, tn_any, tn_atoi),
    TN(pt, "tok_lw_min_n", "MIND_TOK_LW_MIN_N", tok_lw_min_n, tn_any, tn_atoi),
    TN(pt, "tok_lw_min", "MIND_TOK_LW_MIN", tok_lw_min, tn_any, tn_atoi),
    TN(pt, "tok_lw_chunk", nullptr, tok_lw_chunk, tn_min0, nullptr),
    TN(pt, "tgt_side", "MIND_TGT_SIDE", tgt_side, tn_flag, tn_flag_char),
    TN(it, "ilqr_chunk", "MIND_ILQR_CHUNK", ilqr_chunk, tn_min0, tn_atoi),
    TN(it, "ilqr_wgs", "MIND_ILQR_WGS", ilqr_wgs, tn_1_32, tn_atoi),
    TN(it, "ilqr_multi_min", nullptr, ilqr_multi_min, tn_any, nullptr),
    TN(it, "ilqr_wgs_big", nullptr, ilqr_wgs_big, tn_1_32, nullptr),
    TN(it, "ilqr_big_min", nullptr, ilqr_big_min, tn_any, nullptr),
    TN(it, "ilqr_slots", "MIND_ILQR_SLOTS", ilqr_slots, tn_slots, tn_atoi),
    TN(it, "ilqr_spec_deriv", "MIND_ILQR_SPEC_DERIV", ilqr_spec_deriv, tn_flag, tn_flag_atoi),
    TN(it, "ilqr_host_out_max", "MIND_ILQR_HOST_OUT_MAX", ilqr_host_out_max, tn_min0, tn_atoi),
    TN(it, "ilqr_score_block", nullptr, ilqr_score_block, tn_pow2_64, nullptr),
    TN(it, "ilqr_test_starve", nullptr, ilqr_test_starve, tn_flag, nullptr),
    TN(ct, "plan_chunk_mb", "MIND_PLAN_CHUNK_MB", plan_chunk_mb, tn_min1, tn_positive),
    TN(ct, "pl_tab_side", "MIND_PL_TAB_SIDE", pl_tab_side, tn_flag, tn_flag_char),
    TN(ct, "tab_small", "MIND_TAB_SMALL", tab_small, tn_flag, tn_flag_atoi),
    TN(ct, "tab_host_max", "MIND_TAB_HOST_MAX", tab_host_max, tn_min0, tn_atoi),
    TN(ct, "early_eval", "MIND_EARLY_EVAL", early_eval, tn_flag, tn_flag_atoi),
    TN(ct, "glue_fused", "MIND_GLUE_FUSED", glue_fused, tn_flag, tn_flag_atoi),
    TN(ct, "dec_mirror", "MIND_DEC_MIRROR", dec_mirror, tn_flag, tn_flag_atoi),
    TN(ct, "dec_poll", "MIND_DEC_POLL", dec_poll, tn_flag, tn_flag_atoi),
    TN(ct, "root_head", "MIND_ROOT_HEAD", root_head, tn_flag, tn_flag_atoi),
    TN(ct, "round_head", "MIND_ROUND_HEAD", round_head, tn_flag, tn_flag_atoi),
    TN(ct, "upload_kernel_max", "MIND_UPLOAD_KERNEL_MAX", upload_kernel_max, tn_min0, tn_atoi),
    TN(ct, "prof_clock", "MIND_PROF_CLOCK", prof_clock, tn_0_2, tn_atoi),
};
#undef TN
constexpr int TN_ROWS = (int)(sizeof(TN_TABLE) / sizeof(TN_TABLE[0]));

static inline const TnRow *tn_find(const char *name) {
  for (const TnRow &row : TN_TABLE)
    if (strcmp(row.name, name) == 0) return &row;
  return nullptr;
}
// false: no such knob among the records r holds
static inline bool tn_set(const TnRefs &r, const char *name, int value) {
  const TnRow *row = tn_find(name);
  if (row) value = row->rule(value);
  return row && row->io(r, true, &value);
}
static inline bool tn_get(const TnRefs &r, const char *name, int *value) {
  const TnRow *row = tn_find(name);
  return row && row->io(r, false, value);
}

// every variable `lookup` knows (getenv's shape: the text, or null) into its knob
template <class Lookup> static inline void tn_apply_env(const TnRefs &r, Lookup lookup) {
  for (const TnRow &row : TN_TABLE) {
    const char *s = row.env ? lookup(row.env) : nullptr;
    int v;
    if (s && row.text(s, &v)) { v = row.rule(v); (void)row.io(r, true, &v); }
  }
}
