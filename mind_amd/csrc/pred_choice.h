// Which kernels a mind_predict_batch call runs: the predictor's knobs (PredTuning, tuning.h), and the one pure function that turns them, the precision
// setting and the call's scene sizes into a record of decisions (PredChoice).  No HIP call, no context: predict.hip's stages switch on the
// record and read no knob themselves; tests read it through mind_debug_predict_choice.  A new kernel form is a knob here (if it has one), a
// case in pred_choose and a case in the stage that launches its family.
// Included by mind_hip.hip behind the kernel files (LW_CHUNK, TL_CHUNK, DEC_MW_G, RA, P6_QK_STRIDE, LW_NSTAGE) and pair_jobs.h.
#pragma once
#include <vector>

#include "tuning.h"
#include "dec_chain.h"

// partial products per term of the MFMA contractions outside the pair kernel (ActorNet, layer-wise ActorNet, MFMA decoder) under a bf16
// arithmetic: bf16x6 -> 6, bf16x3 -> actor_np (6 or 3), bf16 -> 1
static inline int pred_mfma_parts(const PredTuning &t, int pair_prec) {
  return (pair_prec == 3 || (pair_prec == 1 && t.actor_np == 6)) ? 6 : (pair_prec == 1 ? 3 : 1);
}

// k_pair_t / k_pair_t6: the edge tensor in its tile-native layout
static inline bool pred_edge_tiled(const PredTuning &t, int pair_prec) { return pair_prec == 3 || (pair_prec != 0 && t.pair_tile); }

// bytes of edge tensor per token pair: 128 fp32 features, or bf16 under k_pair_t<*, 1>
static inline int pred_edge_pair_bytes(const PredTuning &t, int pair_prec) { return pred_edge_tiled(t, pair_prec) && pair_prec == 2 ? 256 : 512; }

enum PredActorForm { PRED_ACTOR_VALU = 0, PRED_ACTOR_F32 = 1, PRED_ACTOR_MFMA = 2, PRED_ACTOR_LW = 3 };      // k_actor_net, k_actor_f32<np>, k_actor_mfma<np>, lw_run<np>
enum PredPairFamily { PRED_PAIR_F32 = 0, PRED_PAIR_BF = 1, PRED_PAIR_T = 2, PRED_PAIR_T6 = 3 };              // k_pair, k_pair_bf<., np>, k_pair_t<., np>, k_pair_t6
enum PredDecActor { PRED_DEC_ONE = 0, PRED_DEC_SPLIT = 1, PRED_DEC_MFMA = 2 };                               // k_dec_actor<0>, <1> + <2>, k_dec_actor_mfma<np>

// consecutive scenes of one token class share a launch.  kind 0: VALU, 1: fp32 MFMA (opt-in), 2: bf16 split MFMA
struct PredTokRun {
  int t0, n, kind;
  bool layerwise;       // kind 1 only: the layer-wise kernels (token_lw_kernels.hip) instead of k_token_mfma<0>
  bool small, merged;   // kind 0 only: four tokens per workgroup instead of eight; k_token_m instead of k_token<TOK_TPW_SMALL>
  int form;             // small && merged only (else 0): PRED_TOK_M k_token_m, PRED_TOK_S4 / PRED_TOK_S2 k_token_s with four / two tokens per workgroup
};

// the kernel of a small, merged run (mind_debug_token_form's numbers; 0 there: by rule)
enum PredTokForm { PRED_TOK_RULE = 0, PRED_TOK_M = 1, PRED_TOK_S4 = 2, PRED_TOK_S2 = 3 };

// by rule the small-launch form (k_token_s: k_token_m's bits with its dependent memory round trips cut), on two tokens per workgroup while
// every workgroup still gets a CU of its own, else on four; `forced` (a debug setting, no knob) names a form instead
static inline int pred_tok_form(int forced, int n_tok, int n_cu) {
  if (forced == PRED_TOK_M || forced == PRED_TOK_S4 || forced == PRED_TOK_S2) return forced;
  return (n_tok + 1) / 2 <= n_cu ? PRED_TOK_S2 : PRED_TOK_S4;
}

struct PredChoice {
  int np = 1;                   // pred_mfma_parts
  // ActorNet: form, template argument (actors per workgroup of k_actor_f32, parts of the MFMA forms, 0 for k_actor_net), workgroups of the
  // per-actor forms' one launch, and for the layer-wise form actors per chunk, chunks and launches (lw_build_plan: per chunk the input
  // split, then conv + GroupNorm of every stage)
  int actor_form = PRED_ACTOR_VALU, actor_arg = 0, actor_grid = 0, actor_chunk = 0, actor_chunks = 1, actor_launches = 1;
  // the bf16 pair kernels read the folded query as hi / lo (bf16x6: hi / mid / lo) fragments: mode bits of the token kernel, dwords per token
  int qsplit = 0, qk_stride = 1024;
  bool tiled = false, edge_bf16 = false;
  std::vector<PredTokRun> tok_runs;
  int tok_chunk = 0;            // tokens per chunk of the layer-wise runs
  bool tok_lw = false;          // some run is layer-wise
  int last_tok_chunks = 0;      // ... chunks of all of them (mind_last_token_stats)
  // pair kernel: family, parts of the k_pair_bf / k_pair_t forms, whether layer 5 walks the list of consumed columns, and the XCD grouping
  // factor a fresh deal of the full list / of jobs5 takes (pair_xcd_lanes)
  int pair_family = PRED_PAIR_F32, pair_np = 0;
  bool l5_jobs5 = false;
  int xcd_lanes = 1, xcd_lanes5 = 1;
  // decoder: actor part, the wish for k_dec_scene_mw and its workgroups, the cls head on the side stream when the scene part is not mw
  int dec_actor = PRED_DEC_ONE;
  int dec_head_ra = RA;         // agents per workgroup of the split form's head
  bool fp32_dec = true, split_dec = false, want_mw = false, cls_side = false;
  int mw_blocks = 0;
  int dec_chain_g = 0;          // workgroups per scene of the scene part's launch chain (k_dec_chain1..4); 0: one of the one-launch forms above
  bool tgt_wait_first = false;  // the context stream waits for the target embedding before the fusion layers
};

static PredChoice pred_choose(const PredTuning &t, int pair_prec, int n_cu, bool have_side, int n_scenes, const int *scene_actors, const int *scene_lanes,
                              int tok_form = PRED_TOK_RULE) {
  PredChoice ch;
  int A = 0;
  for (int b = 0; b < n_scenes; ++b) A += scene_actors[b];
  ch.np = pred_mfma_parts(t, pair_prec);

  // ActorNet: fp32 VALU kernel under MIND_PAIR_F32, the bf16-split / bf16 MFMA kernel otherwise (the precision setting covers every MFMA
  // contraction of the predictor) ... and the fp32-MFMA kernel (plain fp32 operands on the matrix core: the reference's arithmetic class):
  // the ActorNet of the exact-fp32 setting, and -- two actors per workgroup -- of every setting on full-tree rounds (thousands of actors per
  // call) ... and for rounds of thousands of actors the MFMA kernel's arithmetic layer by layer over chunks of actors (bit-identical to it)
  ch.actor_grid = A;
  if (t.actor_f32 && A >= (pair_prec == 0 ? t.actor_f32_pair_min : t.actor_f32_min)) {
    ch.actor_form = PRED_ACTOR_F32; ch.actor_arg = 2; ch.actor_grid = (A + 1) / 2;
  } else if (pair_prec == 0 && t.actor_f32 && t.enc_mfma) {
    ch.actor_form = PRED_ACTOR_F32; ch.actor_arg = 1;
  } else if (pair_prec == 0 || !t.enc_mfma) {
    ch.actor_form = PRED_ACTOR_VALU;
  } else if (A >= t.actor_lw_min) {
    ch.actor_form = PRED_ACTOR_LW; ch.actor_arg = ch.np;
    ch.actor_chunk = t.actor_lw_chunk > 0 ? t.actor_lw_chunk : LW_CHUNK;
    ch.actor_chunks = (A + ch.actor_chunk - 1) / ch.actor_chunk;
    ch.actor_grid = ch.actor_chunks;
    ch.actor_launches = ch.actor_chunks * (1 + 2 * LW_NSTAGE);
  } else {
    ch.actor_form = PRED_ACTOR_MFMA; ch.actor_arg = ch.np;
  }

  ch.qsplit = pair_prec == 3 ? 48 : pair_prec != 0 ? 16 : 0;
  ch.qk_stride = pair_prec == 3 ? P6_QK_STRIDE : 1024;      // (three parts under bf16x6)
  ch.tiled = pred_edge_tiled(t, pair_prec);
  ch.edge_bf16 = pred_edge_pair_bytes(t, pair_prec) == 256;

  // The token kernel by SCENE (a scene's result must not depend on what else is in its batch): scenes of at least tok_bf_min_n tokens
  // under the bf16 pair-kernel arithmetics run k_token_mfma<1> (bf16 hi + lo split operands on the MFMA, 16 tokens per workgroup: the
  // VALU kernel is LDS-bound at those sizes), every other scene the VALU kernel -- consecutive scenes of one class share a launch, small
  // launches take four tokens per workgroup (more workgroups, half the LDS operand traffic each; bit-identical to eight)
  // ... and scenes of at least tok_lw_min_n tokens the fp32-MFMA class (kind 1; tok_bf_min_n keeps its precedence under bf16x3 / bf16): a run
  // of them with at least tok_lw_min tokens runs layer-wise (token_lw_kernels.hip), a shorter run k_token_mfma<0> -- the same bits
  ch.tok_chunk = t.tok_lw_chunk > 0 ? t.tok_lw_chunk : TL_CHUNK;
  long long njobs = 0, njobs5 = 0;
  int t0 = 0;
  for (int b = 0; b < n_scenes; ++b) {
    const int N = scene_actors[b] + scene_lanes[b] + 1;
    // (the two-way-split token kernel is not an fp32-class arithmetic: never under bf16x6)
    const int kind = t.tok_mfma ? 1 : (pair_prec != 0 && pair_prec != 3 && t.tok_bf_min_n > 0 && N >= t.tok_bf_min_n) ? 2 : N >= t.tok_lw_min_n ? 1 : 0;
    if (!ch.tok_runs.empty() && ch.tok_runs.back().kind == kind) ch.tok_runs.back().n += N;
    else ch.tok_runs.push_back({t0, N, kind, false, false, false, 0});
    t0 += N;
    njobs += (long long)N * pair_column_splits(N);
    njobs5 += (long long)(scene_actors[b] + 1) * pair_column_splits(N);
  }
  for (PredTokRun &r : ch.tok_runs) {
    r.layerwise = r.kind == 1 && r.n >= t.tok_lw_min;
    // (small launches: independent projections merged -- bit-identical; "tok_merge" 0 keeps the plain form, the reference, for A/B)
    r.small = r.kind == 0 && r.n <= t.tok_small_max;
    r.merged = r.small && t.tok_merge;
    r.form = r.merged ? pred_tok_form(tok_form, r.n, n_cu) : 0;
    if (r.layerwise) {
      ch.tok_lw = true;
      ch.last_tok_chunks += (r.n + ch.tok_chunk - 1) / ch.tok_chunk;
    }
  }

  // The last fusion layer runs the consumed columns only (actors + cls): the tile-native kernels walk a list of their own instead of
  // skipping the other jobs after a dependent load each
  ch.pair_family = pair_prec == 0 ? PRED_PAIR_F32 : pair_prec == 3 ? PRED_PAIR_T6 : ch.tiled ? PRED_PAIR_T : PRED_PAIR_BF;
  ch.pair_np = (ch.pair_family == PRED_PAIR_T || ch.pair_family == PRED_PAIR_BF) ? (pair_prec == 1 ? 3 : 1) : 0;
  ch.l5_jobs5 = ch.tiled;
  ch.xcd_lanes = pair_xcd_lanes(t.xcd_order, n_scenes, pair_grid(njobs, n_cu));
  ch.xcd_lanes5 = pair_xcd_lanes(t.xcd_order, n_scenes, pair_grid(njobs5, n_cu));

  // decoder.  The actor part's first half (actor_proj: 85 % of its weights) needs only the fused actor tokens: it runs on the side stream
  // beside k_dec_scene, the head follows both on the context stream (bit-identical to the one-kernel form); or -- opt-in, "dec_mfma_min" --
  // the MFMA kernel (16 agents per workgroup: 104 against 62 us at 40 agents, 209 vs 277 us at 13.8 k).  Off by default: a plan's result must
  // not depend on what else is in the batch.
  // The scene part: eight workgroups per scene while the whole launch is resident (one workgroup per CU: 158 KB of LDS), else one per scene --
  // the two kernels give the same bits, so a scene's result does not depend on the size of its batch
  ch.fp32_dec = pair_prec == 0 || !t.enc_mfma || A < t.dec_mfma_min;
  ch.split_dec = ch.fp32_dec && have_side && t.dec_overlap;
  ch.dec_actor = ch.split_dec ? PRED_DEC_SPLIT : ch.fp32_dec ? PRED_DEC_ONE : PRED_DEC_MFMA;
  // the split form's head on as many workgroups as the agents give while each has a CU to itself (same bits in every form)
  if (ch.split_dec) ch.dec_head_ra = t.dec_head_ra ? t.dec_head_ra : A <= n_cu ? 1 : (A + 1) / 2 <= n_cu ? 2 : RA;
  ch.mw_blocks = ((n_scenes + 7) / 8) * 8 * DEC_MW_G;
  ch.want_mw = t.dec_mw && ch.mw_blocks <= n_cu;
  ch.cls_side = ch.split_dec && t.dec_cls_side;
  // ... and by rule, with neither knob set, the launch chain: G workgroups per scene on the three big stages, no barrier (dec_chain.h), for calls
  // of at most n_cu / 8 scenes -- the same bits again.  The two knobs keep the one-launch kernels: they are the in-tree reference forms.
  ch.dec_chain_g = (t.dec_mw || t.dec_cls_side) ? 0 : dc_choose_g(n_scenes, n_cu);
  ch.tgt_wait_first = have_side && !t.tgt_side;
  return ch;
}
