/*
 * libmind_hip.so -- C-ABI of the MI355X-native MIND hot path.
 *
 * The reference (HKUST-Aerial-Robotics/MIND) is pure Python and has no FFI of its own; every entry
 * point below cites the reference Python interface it replaces.  All functions return 0 on success
 * or a negative MIND_E* code; no exception crosses the boundary.  The caller owns every buffer it
 * passes in (host or device as stated); the library never frees caller memory.  One context per
 * (process, GPU); calls on one context are serialised on its HIP stream.
 */
#ifndef MIND_HIP_H
#define MIND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIND_OK 0
#define MIND_EINVAL (-1)   /* bad argument / shape */
#define MIND_ENOMEM (-2)   /* device allocation failed */
#define MIND_EHIP (-3)     /* HIP runtime error, see mind_last_error_string */
#define MIND_ESTATE (-4)   /* weights not loaded, context destroyed ... */
#define MIND_ENOTFOUND (-5)/* tensor name missing from the state_dict table */

typedef struct mind_ctx mind_ctx;

/* replaces MINDPlanner.init_device (planners/mind/planner.py:35-39).  `stream` is a hipStream_t
 * on which all work of this context is queued (NULL = the device's default stream).  */
int mind_ctx_create(int device, void *stream, mind_ctx **out);
int mind_ctx_destroy(mind_ctx *ctx);
const char *mind_last_error_string(mind_ctx *ctx);
/* blocks until all work queued on the context's stream is done */
int mind_ctx_synchronize(mind_ctx *ctx);

/* One tensor of ckpt["state_dict"] (planners/mind/planner.py:46-47): fp32, C-contiguous, host. */
typedef struct {
  const char *name;     /* reference state_dict key, e.g. "fusion_net.proj_actor.0.weight" */
  const float *data;    /* host pointer */
  int64_t numel;
} mind_tensor_desc;

/* replaces network.load_state_dict(ckpt["state_dict"]) + .to(device) (planner.py:47-48).  The
 * library re-lays the 328 tensors out into its packed device blob (MFMA fragment order). */
int mind_weights_load(mind_ctx *ctx, const mind_tensor_desc *tensors, int n_tensors);

/* Inputs of ScenePredNet.pre_process / forward (planners/mind/networks/network.py:582-606) for a
 * batch of B scenes (= AIME scenario-tree nodes).  Scene b has a_b = actor_off[b+1]-actor_off[b]
 * agents (ego first) and l_b lane polylines; its token order is [agents, lanes, cls].
 * Device pointers unless stated. */
typedef struct {
  int n_scenes;
  const int32_t *actor_off;   /* HOST [B+1] prefix sums (ACTOR_IDCS are contiguous ranges)        */
  const int32_t *lane_off;    /* HOST [B+1]                                                       */
  const float *actors;        /* [A,14,48]  ACTORS  (mind/utils.py:114-139)                       */
  const float *lanes;         /* [L,10,16]  LANES   (mind/utils.py:103-110); may be NULL if lane_feat */
  const float *lane_feat;     /* [L,128] optional LaneNet output computed earlier (reuse across tree
                                 nodes of one plan: lane node features do not change), or NULL    */
  const float *actor_ctrs;    /* [A,2] TRAJS_CTRS, [A,2] TRAJS_VECS                               */
  const float *actor_vecs;
  const float *lane_ctrs;     /* [L,2] lane_ctrs, lane_vecs of each scene's LANE_GRAPH            */
  const float *lane_vecs;
  const float *const *rpe;    /* HOST array of B device pointers to RPE['scene'] [5,n,n], or NULL
                                 to have it computed in-kernel from ctrs/vecs (utils.py:193-212)  */
  const float *tgt_nodes;     /* [B,10,16] TGT_NODES                                               */
  const float *tgt_rpe;       /* [B,20]    TGT_RPE                                                 */
} mind_scene_batch;

/* Outputs of ScenePredNet.forward (network.py:545-556): res_cls, res_reg, res_aux[0] (res_aux[1], [2]: mind_pred_aux below). */
typedef struct {
  float *cls;        /* [B,6]          softmax mode probabilities                                  */
  float *reg;        /* [A,6,60,5]     (x, y, exp sx, exp sy, exp rho)  agent-local frame          */
  float *vel;        /* [A,6,60,2]                                                                 */
  float *lane_feat;  /* optional [L,128]: LaneNet output written back for reuse (may be NULL)      */
  float *actor_emb;  /* optional debug taps [A,128] fused actor tokens, may be NULL                */
  float *cls_emb;    /* optional [B,128] fused cls token, may be NULL                              */
} mind_pred_out;

/* replaces ScenePredNet.forward over the whole AIME batch (scenario_tree.py:69-71). */
int mind_predict_batch(mind_ctx *ctx, const mind_scene_batch *in, mind_pred_out *out);

/* The rest of res_aux[b] = (vel, cov_vel, param) (network.py:554).  mind_pred_out keeps its layout (callers bind it by layout); these
 * travel beside it.  Device pointers, each may be NULL. */
typedef struct {
  float *cov_vel;   /* optional [A,6,60,3]  d/dt of (log sx, log sy, log rho): Tp diff(param[..., 2:]) / 6 in BOTH bases -- the
                       reference applies diff under the monomial Tp as well (network.py:523 / :534)                                 */
  float *param;     /* optional [A,6,8,5]   control points (x, y, sx, sy, rho), agent-major like reg (the reference's param is
                       [6,a,8,5] per scene: network.py:515 / :526)                                                                  */
} mind_pred_aux;
/* mind_predict_batch with the aux outputs: the decoder's head kernels write them themselves (no further launch).  aux == NULL is
 * mind_predict_batch: the same launches, the same bits of cls / reg / vel -- as is any aux. */
int mind_predict_batch_aux(mind_ctx *ctx, const mind_scene_batch *in, mind_pred_out *out, const mind_pred_aux *aux);

/* The curve basis of the eight control points: SceneDecoder's param_out (network.py:408-435, :449-481).
 *   MIND_BASIS_BEZIER   (default)  T = C(7,i) (1-t)^(7-i) t^i, Tp = 7 C(6,i) (1-t)^(6-i) t^i, vel = Tp diff(P) / 6     (:514-523)
 *   MIND_BASIS_MONOMIAL            T = t^i,                    Tp = (i+1) t^i,                 vel = Tp P[1:] / 6      (:525-534)
 * A checkpoint of either basis has the same tensor shapes: the caller says which one it was trained with.  The setting rewrites the
 * two tables of the loaded weights in place (it drains the context's stream first), holds across later mind_weights_load calls, and
 * covers everything that runs the predictor on the context (mind_predict_batch, mind_aime_plan, the native loop and planner).
 * mind_set_decoder_basis: MIND_EINVAL for an unknown basis; MIND_ESTATE while a plan begun with mind_aime_plan_begin runs or a
 * tree-iLQR call begun with mind_ilqr_contingency_begin(_plan) is pending on the context.  mind_get_decoder_basis returns the basis. */
#define MIND_BASIS_BEZIER 0
#define MIND_BASIS_MONOMIAL 1
int mind_set_decoder_basis(mind_ctx *ctx, int basis);
int mind_get_decoder_basis(mind_ctx *ctx);

/* The decoder's curves at arbitrary times (k_dec_curve): the control points are the continuous-time form of a forecast, the 60
 * samples of reg / vel only its 10 Hz grid.
 * param: DEVICE [n_rows,8,5] (mind_pred_aux.param: n_rows = 6 A); tau: HOST [n_tau], each in [0,1] (fraction of the 6 s horizon);
 * basis: MIND_BASIS_* or -1 = the context's.  reg [n_rows,n_tau,5] = (x, y, exp sx, exp sy, exp rho), vel [n_rows,n_tau,2],
 * cov_vel [n_rows,n_tau,3]: DEVICE, each may be NULL.  The host evaluates the basis rows in double as the weight packer does and
 * rounds them to fp32; the kernel runs the head kernels' contraction, so that at tau = linspace(0, 1, 60) the results are
 * bit-identical to the decoder's own reg / vel / cov_vel for the same param.  Queued on the context's stream.
 * MIND_EINVAL: a non-finite tau or one outside [0,1], n_tau < 1, n_rows < 0, an unknown basis, all three outputs NULL, or
 * n_rows * n_tau > MIND_CURVE_MAX_POINTS.  n_rows == 0 is a successful no-op. */
#define MIND_CURVE_MAX_POINTS (1LL << 26)   /* 40 bytes of output per point: 2.7 GB */
int mind_curve_eval(mind_ctx *ctx, int basis, const float *param, long long n_rows, const double *tau, int n_tau,
                    float *reg, float *vel, float *cov_vel);
/* The basis rows mind_curve_eval uploads (host only, no context): T [n_tau,8], Tp [n_tau,7].  MIND_EINVAL as above. */
int mind_debug_curve_basis(int basis, const double *tau, int n_tau, float *T, float *Tp);

/* Per-kernel timing of the last mind_predict_batch (profiling on: the launch clock, or HIP events on the context stream under "prof_clock" 0):
 * returns the number of fusion pair-kernel launches and their summed milliseconds. */
int mind_last_fusion_stats(mind_ctx *ctx, int *n_launches, float *total_ms, double *pairs_processed);
/* The ActorNet of the last mind_predict_batch: layerwise = 1 when the layer-wise batched kernels ran (mind_set_tuning "actor_lw_min"), 0 for
 * a per-actor kernel; its number of launches and of actor chunks (1 / 1 for a per-actor kernel); total_ms = the time from its first
 * launch to its last on the context stream (HIP events; 0 unless profiling is on, and 0 for the predictor calls inside mind_aime_plan,
 * which do not drain the stream per call).  Any output may be NULL. */
int mind_last_actor_stats(mind_ctx *ctx, int *layerwise, int *n_launches, int *n_chunks, float *total_ms);
/* The token stage (init + the epilogue / prologue behind each fusion layer) of the last mind_predict_batch: layerwise = 1 when a run of
 * scenes took the layer-wise kernels (mind_set_tuning "tok_lw_min_n" / "tok_lw_min"), the launches of all its token steps, the token chunks
 * the layer-wise runs were cut into (0 when none ran), total_ms = the summed time of those launches (HIP events around every one; 0 unless
 * profiling is on, and 0 for the predictor calls inside mind_aime_plan).  Any output may be NULL. */
int mind_last_token_stats(mind_ctx *ctx, int *layerwise, int *n_launches, int *n_chunks, float *total_ms);
/* ... and that time by kernel: out_ms[0..6] = the layer-wise stages (init, merge + V, out-projection + LN2, FFN 1, FFN 2 + LN3, S / T / q,
 * folded K query), out_ms[7] = the one-kernel forms (k_token, k_token_m, k_token_s, k_token_mfma).  Writes min(cap, 8) floats, returns 8. */
int mind_last_token_stage_ms(mind_ctx *ctx, float *out_ms, int cap);
/* Duration of the tree-iLQR kernel of the last mind_ilqr_* call on this context (HIP events on the context stream; 0 unless
 * profiling is on), its number of cost trees and the workgroups per tree it ran with. */
int mind_last_ilqr_stats(mind_ctx *ctx, float *kernel_ms, int *n_trees, int *workgroups_per_tree);
/* Shader-clock cycles of the last tree-iLQR launch's critical cost tree (the one that bounds the launch), summed over its fits:
 * out9 = { nodes M, serial depth (levels), passes of the iteration loop, cycles of the derivative pass, the backward (Riccati) sweep,
 * the line search's state chain, its cost pass, the selection, cost trees in the launch }. */
int mind_last_ilqr_profile(mind_ctx *ctx, double *out9);
/* Per-iteration trace of one fit of the last mind_ilqr_* call on this context (iLQR.fit's loop, planners/ilqr/solver.py:133-158): row k
 * = reference iteration k = { mu the backward pass ran with, J of the nominal trajectory (the reference's J_opt when the line search
 * starts), index of the accepted step size among the ten candidates (-1: every candidate rejected, mu raised; -2: Q_uu singular, the
 * iteration is retried), J of the accepted candidate (J of the nominal trajectory otherwise) }.  tree: index in the call's tree array;
 * phase: 0, or 1 for the full fit of mind_ilqr_contingency.  Writes min(rows, cap_rows) rows of 4 doubles to out and the number of
 * iterations to *n_rows.  MIND_ESTATE when the last call holds no such fit.  Parity diagnostics: the tests compare this trace with the
 * reference's own, iteration by iteration. */
int mind_last_ilqr_trace(mind_ctx *ctx, int tree, int phase, double *out, int cap_rows, int *n_rows);
/* enable/disable kernel timing (off by default).  With mind_set_tuning("prof_clock", 1) (the default; MIND_PROF_CLOCK) the pair kernels and the
 * one-launch ActorNet forms are timed by the launch clock (mind_amd/csrc/launch_clock.h): their workgroups stamp the device's constant-rate
 * wall clock at entry and behind their last store, and a launch counts from its first workgroup in to its last workgroup out -- no HIP event is
 * recorded around them, so the timed path keeps the launch chain of the untimed one.  "prof_clock" 0: HIP events on the context stream around
 * every timed launch, as before (a marker packet on either side of a kernel: DESIGN.md 6).  "prof_clock" 2: both on the same launches
 * (mind_debug_launch_times).  The figures go out under the same names either way (mind_last_fusion_stats, mind_last_actor_stats,
 * mind_aime_plan_out.pair_ms, mind_loop_totals.pair_ms).  The tree-iLQR launch, the token launches and the layer-wise ActorNet keep their events. */
int mind_set_profiling(mind_ctx *ctx, int enable);
/* The timed launches of the last read of kind (0 pair kernels, 1 ActorNet) -- the last mind_predict_batch with profiling on, or the last
 * mind_aime_plan's predictor calls -- one duration in ms per launch in launch order: by the launch clock ("prof_clock" 1, 2) and by HIP events
 * ("prof_clock" 0, 2).  Up to cap values each; *n_clock / *n_event = how many there are.  Any output may be NULL. */
int mind_debug_launch_times(mind_ctx *ctx, int kind, float *clock_ms, float *event_ms, int cap, int *n_clock, int *n_event);
/* host-only helper (tests): the launch clock's ring bookkeeping and reduction (mind_amd/csrc/launch_clock.h) on a ring of n_blocks blocks of
 * block_slots slots, driven by n_ops operations of four long long {op, a, b, 0}:
 *   0 take(grid a, kind b) -> block or -1     1 runs of the pending records a .. a + b - 1 -> count, first0, count0, first1, count1
 *   2 drain the oldest a records               3 fits(records a, grid b) -> 0 / 1          4 grow for (records a, grid b): the ring is reset to the
 *   geometry returned -> blocks, slots         5 reduce block a over a grid of b workgroups of `stamps` (n_slots pairs {t0, t1}: the host
 *   mirror of the ring) -> ticks, ms at rate_khz   6 mark the copy of records a .. a + b - 1 queued   7 the oldest a records have one -> 0 / 1
 * out receives eight doubles per operation: the results above in [0..4], then pending records, head block, launches dropped so far.  Returns
 * the doubles written or MIND_EINVAL (unknown op, a reduce outside `stamps`, cap too small).  Needs no GPU and no context. */
int mind_debug_launch_clock(int n_blocks, int block_slots, int rate_khz, const long long *ops, int n_ops, const unsigned long long *stamps,
                            long long n_slots, double *out, int cap);

/* Arithmetic of the RelaFusionLayer pair contractions (planners/mind/networks/network.py:165-232; the reference runs them
 * in torch fp32) -- and of every other MFMA contraction of the predictor (ActorNet, the MFMA decoder / token kernels where enabled):
 *   MIND_PAIR_BF16X6 (default) = both operands split EXACTLY into three bf16 parts (hi + mid + lo = the 24 significand bits of the fp32
 *     value), the six partial products of weight >= 2^-24 on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: the reference's fp32
 *     arithmetic class at 2.7 x the fp32-MFMA rate (k_pair_t6; ActorNet: k_actor_mfma<6>); error against the fp32 oracle = the fp32 MFMA's;
 *   MIND_PAIR_F32 = plain fp32 operands on the fp32 MFMA (v_mfma_f32_16x16x4_f32; k_pair, k_actor_f32);
 *   MIND_PAIR_BF16X3 = operands split into bf16 hi + lo (16 significand bits), hi.hi + hi.lo + lo.hi: narrower than the reference's fp32 (1e-5 m
 *     from the oracle where the fp32 classes show 3e-6; meets the 2e-4 m parity bar), 1.5-1.8 x faster than bf16x6 on large scenes; opt-in;
 *   MIND_PAIR_BF16 = plain bf16 operands (BASELINE config 5's "bf16 MFMA attention": misses the 1e-3 m parity bar; opt-in).
 * Also settable at context creation through the environment, MIND_PAIR_PREC=f32|bf16x3|bf16|bf16x6. */
#define MIND_PAIR_F32 0
#define MIND_PAIR_BF16X3 1
#define MIND_PAIR_BF16 2
#define MIND_PAIR_BF16X6 3
int mind_set_pair_precision(mind_ctx *ctx, int mode);

/* Tuning knobs (A/B measurements and tests; the defaults are the measured winners, the results are the same within the arithmetic's
 * accuracy).  Every knob is one row of the table in mind_amd/csrc/tuning.h; this list is in the table's order.  Per knob: its name for
 * mind_set_tuning / mind_get_tuning, the environment variable read once at mind_ctx_create (- = none), its default, the values it stores (a
 * value outside them is clamped as shown, never refused), what it does.  A flag stores value != 0; its variable is read either by its first
 * character ("char": on unless the text begins with '0') or as a number ("atoi": on when atoi(text) != 0), as the knob was introduced.
 *   the predictor (mind_predict_batch)
 *   "dec_mfma_min"       MIND_DEC_MFMA_MIN      1 << 30  any int   agents per call from which the decoder's actor part uses the MFMA kernel; default: never
 *   "enc_mfma"           MIND_ENC_MFMA          1        flag char 0: the fp32 VALU ActorNet / decoder kernels under every precision
 *   "actor_f32"          MIND_ACTOR_F32         1        flag char 0: the fp32 VALU ActorNet instead of the fp32-MFMA one under the exact-fp32 setting
 *   "actor_f32_min"      MIND_ACTOR_F32_MIN     1 << 30  any int   actors per call from which the fp32-MFMA ActorNet runs with two actors per workgroup under every setting; default never
 *   "actor_f32_pair_min" -                      1 << 30  any int   the same threshold under exact fp32
 *   "actor_lw_min"       MIND_ACTOR_LW_MIN      1 << 30  any int   actors per call from which the layer-wise batched ActorNet -- actor_lw_kernels.hip: one conv-as-GEMM
 *       launch and one GroupNorm launch per layer over chunks of actors, the layer's weight fragments stationary in LDS -- replaces k_actor_mfma<NP> under
 *       the bf16x6 / bf16x3 / bf16 settings; default never; bit-identical to k_actor_mfma<NP>, so calls, rounds and ranks may differ in which of the two
 *       they take; MIND_PAIR_F32, "enc_mfma" 0 and "actor_f32_min" keep their precedence
 *   "actor_lw_chunk"     -                      0        >= 0      its actors per chunk, 0 = the default of 1024; the scratch arena is one chunk, 137 472 bytes per actor; for
 *       tests and A/B runs only: same bits for every value
 *   "actor_split"        MIND_ACTOR_SPLIT       6        3, else 6 6: three-way operand split, fp32-class; 3: two-way
 *   "xcd_order"          MIND_XCD_ORDER         1        flag char XCD-aware job order of the pair kernel
 *   "pair_tile"          MIND_PAIR_TILE         1        flag char 0: the row-major k_pair_bf instead of the tile-native k_pair_t under bf16x3 / bf16 (same-box A/B measurements)
 *   "dec_overlap"        MIND_DEC_OVERLAP       1        flag char 0: the decoder's actor part as one kernel behind k_dec_scene instead of its actor_proj half beside it on
 *       the side stream; bit-identical
 *   "dec_head_ra"        MIND_DEC_HEAD_RA       0        1, 2, 4, else 0   agents per workgroup of that form's head: 0 = 1 while the call's agents fit one workgroup per CU,
 *       else 2, else 4; 1, 2 or 4 = that form whatever the call, 4 being the head as it was; bit-identical
 *   "tok_mfma"           MIND_TOK_MFMA          0        flag char 1: the per-token epilogue / prologue of the fusion layers on the fp32 MFMA kernel k_token_mfma instead of
 *       the fp32 VALU one; off by default: measured slower
 *   "tok_small_max"      MIND_TOK_SMALL_MAX     2048     any int   batches of at most this many tokens run k_token with four tokens per workgroup instead of eight; same bits
 *   "tok_merge"          MIND_TOK_MERGE         1        flag char small token launches merge their independent projections (k_token_s, the small-launch form of k_token_m); 0: the plain kernel
 *   "dec_mw"             MIND_DEC_MW            0        flag char 1: k_dec_scene_mw, eight workgroups per scene on the decoder's five big stages while every workgroup of the
 *       launch is resident (calls of at most n_cu / 8 scenes); bit-identical to the one-workgroup kernel
 *   "dec_cls_side"       MIND_DEC_CLS_SIDE      0        flag char 1: the decoder's cls head as its own launch on the side stream beside the actor part's head; bit-identical
 *   "tok_bf_min_n"       MIND_TOK_BF_MIN_N      0        any int   scenes of at least this many tokens run k_token_mfma<1> (bf16 hi + lo split operands) under bf16x3 / bf16; 0 = never
 *   "tok_lw_min_n"       MIND_TOK_LW_MIN_N      1 << 30  any int   a SCENE of at least this many tokens takes the fp32-MFMA token class -- the bits of k_token_mfma<0> --
 *       whatever its batch, round or rank; "tok_mfma" 1 still puts every scene there and "tok_bf_min_n" keeps its precedence under bf16x3 / bf16; default never
 *   "tok_lw_min"         MIND_TOK_LW_MIN        1 << 30  any int   a run of consecutive scenes of that class with at least this many tokens runs the layer-wise token kernels
 *       -- token_lw_kernels.hip: one launch per stage over chunks of tokens, the stage's weight fragments stationary in registers -- instead of
 *       k_token_mfma<0>; bit-identical to it, so calls, rounds and ranks may differ; default never
 *   "tok_lw_chunk"       -                      0        >= 0      its tokens per chunk, 0 = the default of 32 768; the scratch arena is one chunk, 2 560 bytes per token; same bits
 *       for every value
 *   "tgt_side"           MIND_TGT_SIDE          1        flag char 0: the context stream waits for the target embedding before the fusion layers
 *   the tree-iLQR solver
 *   "ilqr_chunk"         MIND_ILQR_CHUNK        0        >= 0      nodes per forward step of a narrow tree's line search; 0: whole segments
 *   "ilqr_wgs"           MIND_ILQR_WGS          16       1 .. 32   workgroups per wide cost tree, halved until the launch is resident; 1 = the one-workgroup kernel
 *   "ilqr_multi_min"     -                      192      any int   node count from which a tree is "wide"; a wide-tree launch that is not fully resident -- another context
 *       holds CUs -- aborts at its first barrier and the call is solved again by the one-workgroup kernel: mind_last_ilqr_stats then reports 1
 *       workgroup per tree
 *   "ilqr_wgs_big"       -                      32       1 .. 32   workgroups per tree of at least "ilqr_big_min" nodes
 *   "ilqr_big_min"       -                      12288    any int   ... and that node count
 *   "ilqr_slots"         MIND_ILQR_SLOTS        10       1 .. 12   narrow cost trees: workgroups per tree that take the fit's Levenberg-Marquardt slots -- the master evaluates
 *       slot 0 of every pass, a follower the value the schedule reaches after its number of rejections; 1 = everything in one workgroup; followers
 *       that are not resident are simply not used; same bits for every value
 *   "ilqr_spec_deriv"    MIND_ILQR_SPEC_DERIV   1        flag atoi with slots on follower workgroups one more workgroup per tree runs the derivative pass of a pass's first
 *       candidate beside the master's pricing of the candidates, and the master swaps derivative sets instead of differentiating when that
 *       candidate is the accepted one; same bits; mind_last_ilqr_stats counts it among the workgroups per tree
 *   "ilqr_host_out_max"  MIND_ILQR_HOST_OUT_MAX 4096     >= 0      tree-iLQR launches of at most this many nodes write xs / us / statistics to the host staging themselves; 0 =
 *       always copies
 *   "ilqr_score_block"   -                      0        0, 1, 2, 4 .. 64   mind_ilqr_score_trees: candidates per workgroup, rounded down to a power of two 1 .. 64; 0: 64 while
 *       that keeps two workgroups per CU, halved otherwise down to 4; same bits for every value
 *   "ilqr_test_starve"   -                      0        flag      tests: launch a wide tree without its last workgroups / let the followers of a narrow tree leave at once
 *   the context: copies and launches off the planning cycle's critical path (all of them leave every result bit for bit)
 *   "plan_chunk_mb"      MIND_PLAN_CHUNK_MB     98304    >= 1      mind_aime_plan: a round whose edge tensor would exceed this many MB goes through the predictor in chunks of
 *       scenes.  The variable is ignored unless it is > 0
 *   "pl_tab_side"        MIND_PL_TAB_SIDE       0        flag char 1: the round tables travel on their own stream while the round's predictor runs; measured: no difference
 *   "tab_small"          MIND_TAB_SMALL         1        flag atoi mind_aime_plan's scene tables of a small round travel in the kernel arguments
 *   "tab_host_max"       MIND_TAB_HOST_MAX      4096     >= 0      its small index tables are read from the host staging while they name at most this many workgroups; 0 = always uploaded
 *   "early_eval"         MIND_EARLY_EVAL        1        flag atoi mind_loop prices a candidate tree as soon as the pending launch marks it complete
 *   "glue_fused"         MIND_GLUE_FUSED        1        flag atoi mind_aime_plan's pruning decisions and branch-time bits from one launch, k_aime_select_branch
 *   "dec_mirror"         MIND_DEC_MIRROR        1        flag atoi mind_aime_plan, unsharded: the round's last glue kernel writes the decisions where the host reads them
 *   "dec_poll"           MIND_DEC_POLL          1        flag atoi with "dec_mirror", rounds of one launch: that kernel marks the mirrored decisions complete with a generation
 *       word and the host polls the word, bounded, instead of draining the stream, sizing the next round's buffers while it waits
 *   "root_head"          MIND_ROOT_HEAD         1        flag atoi the root's lane graph, world-frame histories and lane-distance field are queued beside the first round's ActorNet
 *   "round_head"         MIND_ROUND_HEAD        1        flag atoi ... and a later round's repeated lane features beside that round's
 *   "upload_kernel_max"  MIND_UPLOAD_KERNEL_MAX 1 << 20  >= 0      uploads of at most this many bytes from the context's page-locked staging -- the root scene, the solver's
 *       tables -- run as a kernel on the consumer's queue that reads the host buffer, instead of a copy the SDMA engine hands over; 0 = always copies
 *   "prof_clock"         MIND_PROF_CLOCK        1        0 .. 2    which clock times the pair kernels and the one-launch ActorNet forms with profiling on (mind_set_profiling)
 * mind_set_tuning and mind_get_tuning return MIND_EINVAL for an unknown name ("unknown knob '<name>'" in mind_last_error_string).
 * mind_get_tuning writes the stored value: a flag as 0 or 1, "actor_split" as 3 or 6. */
int mind_set_tuning(mind_ctx *ctx, const char *name, int value);
int mind_get_tuning(mind_ctx *ctx, const char *name, int *value);
/* host-only helper (tests): the knob table without a context.  name == NULL: row `index` of the table -- *out_name, *out_env (NULL: the knob
 * has no variable) and *out_value = its default; returns the number of rows, MIND_EINVAL for an index outside them.  name != NULL: what a fresh
 * record stores for that knob after mind_set_tuning(name, value) (text == NULL) or after its variable was read with the text `text` (MIND_EINVAL
 * for a knob without a variable) -> *out_value; returns MIND_OK, MIND_EINVAL for an unknown name.  out_name / out_env may be NULL. */
int mind_debug_tuning(int index, const char *name, const char *text, int value, const char **out_name, const char **out_env, int *out_value);
/* handles the library's contexts hold in this process -- device and page-locked allocations, events, streams: acquisitions less releases.
 * Back at its earlier value once a context is destroyed.  Needs no GPU. */
int mind_debug_live_handles(void);
int mind_get_pair_precision(mind_ctx *ctx);   /* -> mode, or MIND_EINVAL */
/* host-only helper (tests): the bf16 hi / lo MFMA fragment packing of one [128][row_stride] weight matrix,
 * out[16384] dwords = [part 2][out block 8][k group 4][lane 64][4] (see pair_bf16_kernels.hip).  Needs no GPU. */
int mind_debug_pack_bfrag(const float *w, int row_stride, uint32_t *out);

/* host-only helper (tests): the pair kernels' job schedule (mind_amd/csrc/pair_jobs.h) for a batch of n_scenes scenes of scene_tokens[b]
 * tokens on a device of n_cu compute units -- mind_predict_batch's own builder, with "xcd_order" on.  last_layer != 0: the list of the last fusion layer
 * (actor + cls columns only; scene_actors[b] actors per scene).  out_jobs receives up to cap records of six ints
 * {scene, column, first tile, one past the last tile, partial slot, wave slot = wave * grid + workgroup} in list order without the empty
 * padding jobs; out_info[4] = {jobs per column of scene 0, grid, list length with padding, number of jobs}.  Returns the number of jobs or a
 * negative error.  Needs no GPU. */
int mind_debug_pair_schedule(const int *scene_tokens, const int *scene_actors, int n_scenes, int n_cu, int last_layer, int *out_jobs, int cap,
                             int *out_info);

/* host-only helper (tests): which kernels a mind_predict_batch call runs -- the record of pred_choose (mind_amd/csrc/pred_choice.h), the
 * function the call itself decides with -- for a fresh context's knobs with the n_knobs (name, value) pairs of mind_set_tuning applied, the
 * arithmetic pair_prec (0..3), a device of n_cu compute units, with or without the internal side stream, and n_scenes scenes of
 * scene_actors[b] actors and scene_lanes[b] lanes.  out receives up to cap long long of the record: a header
 *   [0] header length (32)  [1] token runs  [2] parts np of the MFMA contractions outside the pair kernel (6, 3, 1)
 *   [3] ActorNet form (0 k_actor_net, 1 k_actor_f32, 2 k_actor_mfma, 3 layer-wise)  [4] its template argument (actors per workgroup of
 *   k_actor_f32, np of the MFMA forms, 0)  [5] workgroups of a per-actor form's launch  [6] actors per chunk, [7] chunks, [8] launches (1 / 1
 *   for a per-actor form: mind_last_actor_stats)
 *   [9] QK format bits of the token kernels' mode (0, 16, 48)  [10] dwords of folded query per token  [11] edge tensor tile-native
 *   [12] ... and bf16  [13] its bytes per token pair  [14] tokens per chunk of a layer-wise token run  [15] some run is layer-wise
 *   [16] chunks of all layer-wise runs (mind_last_token_stats)
 *   [17] pair-kernel family (0 k_pair, 1 k_pair_bf, 2 k_pair_t, 3 k_pair_t6)  [18] parts of k_pair_bf / k_pair_t (3, 1; else 0)
 *   [19] the last fusion layer walks its own list of consumed columns  [20] XCD grouping factor of the full job list, [21] of that list
 *   [22] decoder actor part (0 k_dec_actor<0>, 1 k_dec_actor<1> + <2> over two streams, 2 k_dec_actor_mfma)  [23] np of the MFMA form, else 0
 *   [24] fp32 decoder  [25] split over two streams  [26] k_dec_scene_mw wanted  [27] its workgroups  [28] k_dec_scene_c + k_dec_cls
 *   [29] the context stream waits for the target embedding before the fusion layers  [30] agents per workgroup of the split form's head
 *   (k_dec_actor<2, .>: 1, 2 or 4; 0 outside that form)  [31] workgroups per scene of the scene part's launch chain k_dec_chain1..4 (32, 16 or
 *   8: the largest with scenes x workgroups <= n_cu; 0: one of the one-launch forms [26] / [28] / k_dec_scene -- "dec_mw" or "dec_cls_side" set,
 *   or more than n_cu / 8 scenes)
 * and one row {first token, tokens, kind (0 VALU, 1 fp32 MFMA, 2 bf16 split MFMA), layer-wise, small (four tokens per workgroup), merged
 * (k_token_s, or k_token_m under mind_debug_token_form)} per token run.  Returns the length of the full record, or MIND_EINVAL for an unknown knob, pair_prec outside 0..3, a scene
 * with no actor or a negative lane count, or a null pointer.  Needs no GPU and no context. */
int mind_debug_predict_choice(const char *const *knob_names, const int *knob_values, int n_knobs, int pair_prec, int n_cu, int have_side,
                              const int *scene_actors, const int *scene_lanes, int n_scenes, long long *out, int cap);

/* host-only helper (tests): how a tree-iLQR call launches and what index tables it uploads -- the records of il_choose and il_tree_tables
 * (mind_amd/csrc/ilqr_choice.h), the two functions the solver itself decides with -- for a fresh context's knobs with the n_knobs (name,
 * value) pairs of mind_set_tuning applied ("ilqr_*" only), a device of n_cu compute units, the call's mode (bit 0: generic mode of
 * mind_ilqr_solve_fields, bit 1: mind_cost_eval, bit 2: two fits in one launch -- no decision depends on it today) and n_trees cost trees of
 * n_nodes[t] nodes whose parent arrays lie one behind the other in `parents`.  out receives up to cap long long of the record: a header
 *   [0] header length (16)  [1] trees  [2] kernel form (0 one workgroup per tree, 1 wide trees: G workgroups share a tree, 2 narrow trees: a
 *   master + followers take a tree's Levenberg-Marquardt slots)  [3] G (1 outside form 1)  [4] GS (workgroups per tree that take slots)
 *   [5] derivative speculators per tree (0, 1)  [6] sets of per-slot arrays in the arena  [7] workgroups of the launch
 *   [8] workgroups_per_tree as mind_last_ilqr_stats reports it  [9] the kernel writes its results to the host staging itself
 *   [10] ... and marks each tree when it is complete  [11] "ilqr_test_starve" lets the followers of form 2 leave at once  [12]..[15] 0
 * and per tree {nodes, levels nl, segments nseg, segment levels nsl, widest segment level maxls, forward steps nfs}, the lengths of its
 * fourteen tables and then the tables themselves: level starts, level nodes, child starts, child list, segment starts, segment nodes,
 * segment-level starts, segment-level segments, segment records (16 ints each: s0, s1, last node, first node, node before the last, the last
 * node's child count, its child-list start, 0, its first six children, 0, 0), step starts, step items (8 ints each: q0, q1, first node, second
 * node, the first node's parent, 0, 0, 0), the items' q1, step node starts, step nodes.  Returns the length of the full record, or
 * MIND_EINVAL for an unknown knob, a tree without nodes, a null pointer, or a node whose parent is not below it (node 0: not -1); bad (two
 * ints, may be null) then names that tree and node, and is {-1, -1} otherwise.  Needs no GPU and no context. */
int mind_debug_ilqr_plan(const char *const *knob_names, const int *knob_values, int n_knobs, int n_cu, int mode, int n_trees, const int *n_nodes,
                         const int32_t *parents, long long *out, int cap, int *bad);

/* host-only helper (tests): the bookkeeping of mind_aime_plan -- AimeBook, pl_route and pl_chunk (mind_amd/csrc/aime_book.h), the functions the
 * plan itself calls -- replayed over the decision words of n_rounds rounds, on rank `rank` of `world` (force: a one-rank group exchanges too,
 * as with mind_set_exchange).  dec holds the rounds one behind the other, dec_len[r] floats each: per rank of the group (one rank when no
 * exchange runs) sel [Bmax,6] (kept mode or -1, visiting order) | sel_prob [Bmax,6] | hit [Bmax,6,2] (branch-time bits, two 32-bit words),
 * Bmax = the largest block of the round's scenes; a length that does not fit the round is MIND_EINVAL.  The plan stops at the first empty
 * branch set; this replay goes on while rounds are given.  n_tokens > 0: the chunk size of every round for that many tokens per scene,
 * bytes_per_pair and plan_chunk_mb; per_scene: floats per scene in the all-to-all's byte table.  The record `out` (as much of it as `cap`
 * holds) is a header of 16,
 *   [0] header length  [1] which "unsupported" exit was taken (0 none; msg then holds the plan's error string), [2], [3] the numbers it names
 *   [4] rounds consumed  [5] nodes  [6] cost trees  [7] their trajectory nodes  [8] floats of rows  [9] root flags  [10] exchanges run  [11] world
 * per consumed round {scenes B, this rank's block lo, hi, Bmax, chunk size, branch set S, this rank's children s0, Sm, scenes the all-to-all
 * moves on any rank} and todo [S], cnt_r [world], s0_r [world + 1], k_aime_windows' ints [3 Sm], the byte table [2][world], the scene ranges
 * sent to / received from every rank [world][2] each; and without an exit: per node {round, scene, mode, parent, prob (float32 bits), cur_t,
 * end_t, flags, dur, row_off, owner rank, scene in the owner's block}; the gather and then the flat job table, each {jobs, workgroups, bytes of
 * the device image} + per job {row0, n, dst, a, round of its world buffer} + job of workgroup + agent of workgroup; tree_top, tree_off
 * [trees + 1], flat_parent, flat_prob (float32 bits).  Returns the length of the full record or MIND_EINVAL.  Needs no GPU and no context. */
int mind_debug_aime_book(int pred_len, int max_depth, int max_rounds, int n_agents, int world, int rank, int force, int n_rounds, const int *dec_len,
                         const float *dec, int n_tokens, int bytes_per_pair, int plan_chunk_mb, int per_scene, long long *out, int cap, char *msg,
                         int msg_cap);

/* host-only helper (tests): the bounded wait of mind_aime_plan's polled decisions (pl_wait_word, mind_amd/csrc/aime_book.h) over the caller's
 * word and clock: acquire loads of *word until it holds `want`; clock(user) (seconds, any origin; null: the steady clock) is read every
 * spins_per_look misses and the wait gives up once more than timeout_s have passed.  Returns 1 when the word arrived, 0 after the time-out,
 * MIND_EINVAL for a null word, a negative time-out or spins_per_look <= 0.  Needs no GPU and no context. */
int mind_debug_wait_word(const unsigned *word, unsigned want, double timeout_s, double (*clock)(void *user), void *user, int spins_per_look);

/* host-only helper (tests): the launch list of the layer-wise batched ActorNet for a call of n_actors actors in the arithmetic np (6, 3, 1 =
 * bf16x6, bf16x3, bf16; anything else: MIND_EINVAL) with `chunk` actors per chunk (0 = the default) -- exactly what mind_predict_batch issues.
 * out_launches receives up to cap records of 16 long long in issue order: {stage 0..25 (-1: the input split), kind (0 input split, 1 conv,
 * 2 GroupNorm epilogue), grid x, grid y, threads per workgroup, LDS bytes, first actor of the chunk, actors in the chunk, Cin, Cout, kernel
 * size, stride, Tin, Tout, fragment bytes a conv workgroup keeps stationary, 1 for the stage that writes actor_feat}.  out_info[3] = {chunk
 * size, arena bytes, number of launches}.  Returns the number of launches or a negative error.  Needs no GPU. */
int mind_debug_actor_lw_plan(int n_actors, int np, int chunk, long long *out_launches, int cap, long long *out_info);

/* host-only helper (tests): the launch list of the layer-wise token stage for one token step of `mode` (1|4 init, 2|4 behind fusion layers
 * 0-4, 2|8 behind the last; | 16 or | 16|32 for the bf16 / bf16x6 QK formats; anything else: MIND_EINVAL) over a run of n_tokens tokens with
 * `chunk` tokens per chunk (0 = the default), grids sized for 256 compute units.  out_launches receives up to cap records of 8 long long in
 * issue order: {stage (0 init, 1 merge + V, 2 out-projection + LN2, 3 FFN 1, 4 FFN 2 + LN3, 5 S / T / q, 6 folded K query), grid x, grid y,
 * threads per workgroup, LDS bytes, first token of the chunk, tokens in the chunk, 16-token tiles in the chunk}.  out_info[4] = {chunk size,
 * arena bytes, number of launches, number of chunks}.  Returns the number of launches or a negative error.  Needs no GPU. */
int mind_debug_token_lw_plan(int n_tokens, int mode, int chunk, long long *out_launches, int cap, long long *out_info);

/* host-only helper (tests): the bf16 hi / mid / lo MFMA A-operand packing of one Conv1d weight [co][ci][ksz] (torch layout) for the
 * ActorNet GEMMs of actor_mfma_kernels.hip: [co/16][k-step][part 3 = hi, mid, lo][lane 64][4] dwords, GEMM index k = tap * ci_pad + ci
 * (ci_pad = ci rounded up to a power of two >= 16).  Returns the number of dwords written (<= cap) or a negative error. */
int mind_debug_pack_conv_frag(const float *w, int co, int ci, int ksz, uint32_t *out, size_t cap);

/* host-only helpers (tests) over mind_amd/csrc/weight_pack.h, the packer and the binder mind_weights_load itself runs.  None needs a GPU or a
 * context.
 *
 * mind_debug_pack: one packer by name -- "afrag" (a = row stride), "wk_frag", "tok_bfrag" (a = row stride), "bfrag_lo3" (a = row stride),
 * "conv_f32" (a, b, c = co, ci, ksz of a torch-layout Conv1d weight), "center_outputs" (W [a][b] followed by the bias [a], in and out).  The
 * fragment packers read a [128][128] block of w with the given row stride.  Returns the number of floats (or dwords as float bit patterns)
 * written (<= cap) or MIND_EINVAL.
 *
 * mind_debug_weight_image: the packed blob of a state_dict.  out_info[3] = {entries, floats of the blob, bytes of the name list with its
 * terminator}; blob, names (the entry keys in blob order, each followed by '\n') and entries ({offset, length} in floats per entry) are each
 * filled when non-null and large enough (blob_cap in floats, names_cap in bytes, entries_cap in entries).  MIND_ENOTFOUND with the
 * tensor's name in msg when a tensor is missing or has the wrong size.
 *
 * mind_debug_weight_bind: packs the state_dict, forgets the blob entry `drop` (may be null; MIND_EINVAL when there is no such entry) and binds
 * the pointer tables against the host image.  MIND_OK, or MIND_ENOTFOUND with msg = the missing tensor (packing) or blob key (binding). */
int mind_debug_pack(const char *what, const float *w, int a, int b, int c, float *out, size_t cap);
int mind_debug_weight_image(const mind_tensor_desc *tensors, int n_tensors, float *blob, size_t blob_cap, char *names, size_t names_cap,
                            long long *entries, int entries_cap, long long *out_info, char *msg, int msg_cap);
int mind_debug_weight_bind(const mind_tensor_desc *tensors, int n_tensors, const char *drop, char *msg, int msg_cap);

/* Debug tap (tests): the tree-iLQR kernel's sin / cos / tan (mind_amd/csrc/mind_trig.h, the routine oracle/ilqr_ref.c shares) of n host
 * doubles, evaluated on the device one wave of 64 arguments at a time -- out[4 n] = sin, cos, tan, the cosine that comes with the
 * tangent.  The oracle's oracle_sincos / oracle_tan_cos must give the same bits (tests/test_gpu_ilqr.py). */
int mind_debug_trig(mind_ctx *ctx, const double *x, int n, double *out);

/* Debug tap (tests, tools/dec_chain_forms.py): the decoder's scene part alone, with the context's weights, on n_scenes caller-given cls token
 * rows (host, [n_scenes][128]) in a given form -- 0: the one-workgroup kernel k_dec_scene; 8, 16 or 32: the launch chain k_dec_chain1..4 with
 * that many workgroups per scene (mind_amd/csrc/dec_chain.h), whatever mind_predict_batch's rule would take for the call.  Every form gives
 * the same bits.  Cout (host, [n_scenes][6][128]) receives the mode tokens, cls (host, [n_scenes][6]) the mode probabilities.  The form is
 * queued reps (1..1024) times; ms (reps floats, may be null) receives the time of each repetition between two events on the context's
 * stream.  MIND_EINVAL for a null pointer, another form, n_scenes outside 1..4096 or reps outside 1..1024; MIND_ESTATE without weights. */
int mind_debug_dec_scene(mind_ctx *ctx, const float *rows, int n_scenes, int form, float *Cout, float *cls, int reps, float *ms);

/* Debug taps used by the parity tests only: run just the first n (0..6) fusion layers on the next
 * mind_predict_batch calls, and read internal device buffers ("x", "ST", "QK", "edge", "part",
 * "actor_feat", "tokpos"; "pl_root": the root scene of the last mind_aime_plan as it lies on the device, laid out as RootLayout,
 * mind_amd/csrc/aime_book.h, up to the buffer's capacity) back to the host.  mind_debug_read returns the number of floats copied (or
 * the buffer's size when host == NULL) or a negative error. */
int mind_debug_set_layers(mind_ctx *ctx, int n);
int64_t mind_debug_read(mind_ctx *ctx, const char *name, float *host, int64_t max_floats);

/* A/B of the small, merged token launches (runs whose row of mind_debug_predict_choice ends 1, 1; no knob, bit-identical forms): form 0 by
 * rule -- k_token_s, on two tokens per workgroup while (n_tok + 1) / 2 <= n_cu, else on four --, 1 k_token_m, 2 / 3 k_token_s on four / two
 * tokens per workgroup.  A non-null ctx keeps `form` for its later calls; ctx may be NULL (no GPU).  Returns the form (1..3) that a lone
 * scene of n_tok tokens takes on n_cu CUs under `form` and the default knobs, 0 if its run is not small and merged; with n_tok 0 `form` itself;
 * MIND_EINVAL for a form outside 0..3, a negative n_tok or n_cu <= 0 with n_tok > 0. */
int mind_debug_token_form(mind_ctx *ctx, int form, int n_tok, int n_cu);

/* ------------------------------------------------------------------------------------------------
 * Tree-iLQR contingency solves: replaces TrajectoryTreeOptimizer.init_warm_start_cost_tree /
 * warm_start_solve / init_cost_tree / solve (planners/mind/trajectory_tree.py:19-147) together with
 * iLQR.fit (planners/ilqr/solver.py:80-167), TreeCost (ilqr/cost.py:326-446) and the potentials
 * (ilqr/potential.py).  One cost tree per scenario tree; all trees of a plan are solved in one call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int n_nodes;              /* M trajectory nodes, keys 0..M-1 in creation order (LIFO DFS, Q13)  */
  const int32_t *parent;    /* HOST [M] parent key, -1 for node 0 (child of the x0 root)          */
  const float *prob;        /* HOST [M] scenario-node probability (fp32 as in the reference)      */
  int n_agents;             /* a (agent 0 = ego)                                                  */
  const float *agent_mean;  /* HOST [M, a, 2] predicted mean of every agent at the node's step    */
  const float *agent_cov;   /* HOST [M, a]    max-sigma                                           */
  /* generic mode only (mind_ilqr_solve_fields / mind_cost_eval with a grid), NULL otherwise:        */
  const double *field;      /* HOST [M, H, W] cost_field of each node's PotentialField             */
  const double *node_w;     /* HOST [M, 32]  per node: diag w_des[6], diag w_con[6], lower[6],     */
                            /*   upper[6], diag w_ctrl[2], des_state[6] (StatePotential,           */
                            /*   StateConstraint, ControlPotential of ilqr/potential.py:4-59)      */
} mind_cost_tree;

typedef struct {
  double dt, wheelbase;                 /* 0.2, 2.5 (trajectory_tree.py:15)                        */
  double w_des_state[6];                /* diag of w_des_state                                     */
  double w_state_con[6];                /* diag of w_state_con                                     */
  double state_lower[6], state_upper[6];
  double w_ctrl[2];                     /* diag of w_ctrl                                          */
  double w_tgt, w_ego, w_ego_cov_offset, w_exo, w_exo_cov_offset, w_exo_cost_offset;
  double grid_res; int grid_w, grid_h;  /* 0.4, 256, 256                                           */
  int max_iter;                         /* 100                                                     */
} mind_ilqr_cfg;

typedef struct { int iterations; int converged; double J; double mu; } mind_ilqr_stats;

/* x0[6] = (x,y,v,yaw,a,delta); target_lane HOST [P,2] float64 (gt_tgt_lane as float64);
 * us_init HOST [sum M, 2] (NULL = zeros); use_exo = 0 builds the warm-start tree (lane term only).
 * Outputs HOST xs [sum M, 6], us [sum M, 2], stats [n_trees]. */
int mind_ilqr_solve_trees(mind_ctx *ctx, const mind_ilqr_cfg *cfg, const mind_cost_tree *trees,
                          int n_trees, const double *x0, const double *target_lane, int n_lane_pts,
                          double target_vel, int use_exo, const double *us_init, double *xs,
                          double *us, mind_ilqr_stats *stats);

/* MINDPlanner.get_traj_tree (planner.py:174-178) for every scenario tree of a plan in ONE launch: the warm-start
 * fit (init_warm_start_cost_tree + warm_start_solve: lane term only, cfg_warm = w_opt_cfg, zero initial controls)
 * followed, from its controls, by the full fit (init_cost_tree + solve, cfg_full = opt_cfg).  xs / us are the
 * full fit's; both configurations must share dt, wheelbase and the grid. */
int mind_ilqr_contingency(mind_ctx *ctx, const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full,
                          const mind_cost_tree *trees, int n_trees, const double *x0,
                          const double *target_lane, int n_lane_pts, double target_vel, double *xs,
                          double *us, mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full);
/* The same call in two halves, for a caller that has host work of its own while the kernel runs (the planner builds the scenario
 * trees' Python objects meanwhile): _begin uploads, launches and queues the read-backs on the context stream and returns without
 * waiting (trees / x0 / target_lane are consumed before it returns); mind_ilqr_finish waits and writes xs / us / stats_* -- those
 * arrays must stay valid until then.  One call can be pending per context; another mind_ilqr_* call in between returns MIND_ESTATE,
 * as does mind_ilqr_finish with nothing pending. */
int mind_ilqr_contingency_begin(mind_ctx *ctx, const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full,
                                const mind_cost_tree *trees, int n_trees, const double *x0,
                                const double *target_lane, int n_lane_pts, double target_vel, double *xs,
                                double *us, mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full);
/* ... on the cost trees the last mind_aime_plan of this context flattened (mind_aime_plan_out.flat_*: n_trees trees of tree_off[t+1] -
 * tree_off[t] nodes): the tree arrays stay inside the library.  xs / us: [tree_off[n_trees], 6 / 2], stats_*: [n_trees]. */
int mind_ilqr_contingency_begin_plan(mind_ctx *ctx, const mind_ilqr_cfg *cfg_warm, const mind_ilqr_cfg *cfg_full, const double *x0,
                                     const double *target_lane, int n_lane_pts, double target_vel, double *xs, double *us,
                                     mind_ilqr_stats *stats_warm, mind_ilqr_stats *stats_full);
int mind_ilqr_finish(mind_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * AIME glue (k7): the arithmetic of ScenarioTreeGenerator.prune_merge (planners/mind/scenario_tree.py:
 * 281-412) that touches every (agent, mode, step) -- world-frame positions / velocities / headings,
 * max-sigma covariances and the topology signatures -- for all scenes of one AIME round, reading the
 * predictor outputs where they already are (device), and optionally the pruning decisions themselves.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int n_scenes;
  const int32_t *actor_off;   /* HOST [n+1]                                                        */
  const float *reg, *vel;     /* DEVICE [A,6,60,5], [A,6,60,2]: mind_pred_out.reg / .vel            */
  const float *actor_ctrs, *actor_vecs; /* DEVICE [A,2] agent frames (as in mind_scene_batch)      */
  const float *rot, *orig;    /* HOST [n,2,2], [n,2]: scene frames ROT / ORIG                       */
  const float *cov_last;      /* HOST [A] last history covariance TRAJS_COV_HIST[:, -1, 0]          */
  const int32_t *last;        /* HOST [n] index of the last predicted step kept by seq_len (or < 0) */
  const float *target_lane;   /* HOST [n_lane_pts,2] target lane polyline (float32), or NULL            */
  int n_lane_pts;
  /* optional: the pruning decisions on the device too (needs mind_world_out.sel / sel_prob) */
  const float *cls;           /* DEVICE [n,6] mode probabilities (mind_pred_out.cls), or NULL                */
  const float *scen_prob;     /* HOST [n] SCEN_PROB of every scene                                          */
  int lane_check;             /* 1: drop modes whose ego end point is farther than dist_thres (+ sigma) from the target
                                 lane (needs target_lane and last >= 0 for every scene)                     */
  float dist_thres;           /* tar_dist_thres                                                             */
} mind_world_in;

typedef struct {
  float *world;               /* DEVICE [A,6,60,6]: x, y, vx, vy, heading, max-sigma (world frame)  */
  float *topo;                /* DEVICE [A,6] winding of (agent - ego of its scene); ego rows = 0   */
  float *ego_end;             /* DEVICE [n,6,4]: ego x, y, max-sigma at step `last` and the distance */
                              /*   of that point to the target lane (if last >= 0; inf without lane) */
  float *sel, *sel_prob;      /* DEVICE [n,6] or NULL: kept modes of every scene in visiting order (mode index as a    */
                              /*   float, -1 = none) and their path probabilities: probability floor, target-lane      */
                              /*   pruning and the greedy topology merge of prune_merge (:293-327, 361-395)            */
} mind_world_out;

/* asynchronous on the context stream (read the outputs after mind_ctx_synchronize or a stream-ordered copy) */
int mind_aime_world(mind_ctx *ctx, const mind_world_in *in, const mind_world_out *out);

/* tests: the decision kernels of an AIME round on GIVEN inputs, with the launch shapes of the plan's round -- fused = 0: k_aime_select then
 * k_aime_branch, fused = 1: k_aime_select_branch; by_value = 0: scene tables in device memory, 1: by value in the kernel arguments (at most 8
 * scenes, all with the same agent count: MIND_EINVAL otherwise).  actor_off [n+1], cmp [n] (predicted step the branch-time test divides by,
 * 0..59), scen_prob [n]: HOST.  cls [n,6], topo [A,6], ego_end [n,6,4], world [A,6,60,6] (only record 5, max-sigma, is read): DEVICE.
 * prob_floor <= 0: 0.001.  Outputs (DEVICE): sel, sel_prob [n,6] as mind_world_out, hit [n,6,2]: bit t of the two 32-bit words of kept slot j is
 * set when some agent's max-sigma at step t exceeds 9 x its max-sigma at step cmp (get_branch_time, scenario_tree.py:592-611).  Synchronous. */
int mind_debug_aime_decide(mind_ctx *ctx, int n_scenes, const int32_t *actor_off, const int32_t *cmp, const float *cls, const float *scen_prob,
                           const float *topo, const float *ego_end, const float *world, int lane_check, float dist_thres, float prob_floor,
                           int fused, int by_value, float *sel, float *sel_prob, uint32_t *hit);

/* Re-basing of the observation at a branch point for all branching nodes of a round: update_obser
 * (scenario_tree.py:467-567) = get_origin_rotation / normalisation into the AV and agent frames
 * (utils.py:180-190, scenario_tree.py:128-158), actor features (utils.py:113-134), get_new_lane_graph
 * (utils.py:171-177), get_high_level_command (scenario_tree.py:613-652) and the target RPE (utils.py:193-242).
 * The outputs are the next round's mind_scene_batch tensors, written on the device. */
typedef struct {
  int n_scenes, n_agents, n_lanes;  /* S child scenes sharing one agent set (a) and one lane graph (l)   */
  const float *pos, *ang, *vel;     /* HOST [S,a,50,2], [S,a,50], [S,a,50,2]: last 50 world-frame steps    */
  const float *types;               /* HOST [a,50,7] TRAJS_TYPE                                            */
  const float *pad;                 /* HOST [S,a,50] PAD_OBS or NULL (= ones, as update_obser sets it)     */
  const float *lane_ctrs, *lane_vecs; /* HOST [l,2] lane_graph["lane_ctrs"/"lane_vecs"]                    */
  const float *target_lane;         /* HOST [P,2]                                                          */
  const float *target_lane_info;    /* HOST [P,12]                                                         */
  int n_lane_pts;                   /* P >= 12                                                             */
  float time_ahead, min_vel;        /* tar_time_ahead (5.0), 0.5                                           */
  /* Optional: the windows assembled ON THE DEVICE instead of uploaded (pos / ang / vel may then be NULL).  A child's window is
   * the last 50 steps of [its parent's window | its own first `dur` predicted steps] (scenario_tree.py:396-412, 470-473): the
   * parent's window is taken from the arena of the PREVIOUS mind_aime_rebase call on this context (its generation must be
   * prev_gen), the child's steps from `rows` (the [R,60,6] world-frame rows mind_aime_world's caller gathered for the kept modes:
   * x, y, vx, vy, heading, max-sigma). */
  const float *rows_dev;            /* DEVICE [R,60,6] or NULL (= host windows above)                      */
  const int32_t *parent_slot;       /* HOST [S] scene index of the parent in the previous call             */
  const int32_t *row0;              /* HOST [S] first row (agent 0) of the child in rows_dev                */
  const int32_t *dur;               /* HOST [S] number of predicted steps kept (END_T - CUR_T), 0..60       */
  int prev_gen;                     /* generation of the call that re-based the parents                     */
} mind_rebase_in;

typedef struct {
  float *actors;                    /* DEVICE [S*a,14,48]                                                  */
  float *actor_ctrs, *actor_vecs;   /* DEVICE [S*a,2]                                                      */
  float *lane_ctrs, *lane_vecs;     /* DEVICE [S*l,2]                                                      */
  float *tgt_nodes, *tgt_rpe;       /* DEVICE [S,10,16], [S,20]                                            */
  float *frames;                    /* DEVICE [S,28]: ROT (4, row-major), ORIG (2), TGT_PTS (11 x 2)       */
  int32_t *gen;                     /* HOST, optional: receives this call's generation (for the children's prev_gen) */
} mind_rebase_out;

int mind_aime_rebase(mind_ctx *ctx, const mind_rebase_in *in, const mind_rebase_out *out);

/* ------------------------------------------------------------------------------------------------
 * ScenarioTreeGenerator.branch_aime (planners/mind/scenario_tree.py:38-58) in ONE call: every AIME round -- the batched scene
 * prediction (:69-71), prune_merge (:281-412), create_nodes (:73-80), decide_branch / get_branch_time (:82-100, 592-611) and
 * update_obser (:467-567) of the branching nodes -- runs on the device with the per-round bookkeeping in native code; the host
 * sees one small read-back per round (kept modes + branch-time bits).  The caller supplies what process_data (:122-206) and
 * prepare_root_data (:414-465) produce for the root and receives the internal tree's nodes plus, for the nodes of finished
 * branches, the rows get_scenario_tree (:208-272) attaches.  All pointers HOST, float32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int n_agents, n_lanes, n_lane_pts;
  const float *actors;                       /* [a,14,48]  ACTORS of the root scene                                       */
  const float *actor_ctrs, *actor_vecs;      /* [a,2]      TRAJS_CTRS / TRAJS_VECS                                        */
  const float *lanes;                        /* [l,10,16]  LANES (instance-frame lane features)                           */
  const float *lane_ctrs, *lane_vecs;        /* [l,2]      lane_graph anchors (AV frame; update_obser re-expresses them)  */
  const float *tgt_nodes, *tgt_rpe;          /* [10,16], [20]                                                             */
  const float *rot, *orig, *tgt_pts;         /* [2,2], [2], [11,2]: ROT, ORIG, TGT_PTS of the root                        */
  const float *hist;                         /* [a,50,6]   root world-frame history: x, y, vx, vy, heading, max-sigma     */
  const float *types;                        /* [a,50,7]   TRAJS_TYPE                                                     */
  const float *target_lane;                  /* [P,2]                                                                     */
  const float *target_lane_info;             /* [P,12]                                                                    */
  float time_ahead, min_vel, dist_thres;     /* tar_time_ahead, 0.5, tar_dist_thres                                       */
  int max_depth;                             /* ScenTreeCfg.max_depth                                                     */
  int max_rounds;                            /* safety bound on the number of rounds (>= max_depth + 1)                   */
  int pred_len;                              /* planning horizon in predicted steps (the generator's pred_len, 50: END_T of  */
                                             /*   a fresh observation; seq_len = 50 + pred_len), <= 60                     */
  /* Root scene built ON THE DEVICE (process_data + prepare_root_data as kernels): when raw_pos != NULL the fields actors ... hist
   * above are ignored (may be NULL) and the library computes them from what get_agent_trajectories (utils.py:245-342) returns and
   * the map's resampled lane polylines: normalisation into the AV / agent frames and actor features (k_aime_rebase on the raw
   * windows), lane graph + LANES features (k_aime_root_lanes, float64 as update_lane_graph_from_argo), high-level command, the
   * root's world-frame histories as prepare_root_data reconstructs them (k_aime_root_hist). */
  const float *raw_pos, *raw_ang, *raw_vel;  /* [a,50,2], [a,50], [a,50,2] world-frame padded histories, AV first            */
  const float *raw_pad;                      /* [a,50] observed flags (PAD_OBS)                                               */
  const double *lane_pts;                    /* [l,11,2] world-frame points of every 15 m lane piece (10 sub-segments)        */
  const int32_t *lane_flags;                 /* [l,6]: lane type (0 vehicle, 1 bike, 2 bus), intersection, left / right mark   */
                                             /*   class (0 crossable, 1 not, 2 other), has left / right neighbour              */
  float travel0;                             /* max(ego speed, min_vel) * time_ahead (float32), scenario_tree.py:131,620-624   */
  /* Test / benchmark hook (mind_amd/synth.py ScriptedBranching, ScriptedFullTree: the reference ships no trained checkpoint and the
   * formula weights collapse every plan to a node or two, so the full-tree workloads of BASELINE configs 4 / 5 script the modes): when
   * script_cls != NULL the predictor still runs on every scene of every round, and these DEVICE arrays then take the place of its
   * outputs for every scene: cls [6], reg [a,6,60,5], vel [a,6,60,2]. */
  const float *script_cls, *script_reg, *script_vel;
  /* path-probability floor of prune_merge (scenario_tree.py:368-370).  0 = the reference's 0.001; the scripted stress workload lifts it
   * (a small positive value) so that a full 6-ary depth-5 tree can grow: 6^-4 is already below 0.001. */
  float prob_floor;
  /* Optional: begin the contingency solves of the plan (planner.py:174-178: warm-start fit + full fit of every scenario tree) straight
   * behind it, before the call returns -- everything they need besides the plan's own cost trees is known when the plan starts (ego
   * state x0 [6], target lane [solve_n_lane_pts, 2] float64, target velocity, the two configurations).  solve_cfg_full != NULL asks
   * for it; out->solves_begun tells whether it happened (not on a sharded context, not without a finished branch), and
   * mind_ilqr_finish_plan collects.  Saves the host round trip between the plan's last kernel and k_ilqr. */
  const mind_ilqr_cfg *solve_cfg_warm, *solve_cfg_full;
  const double *solve_x0, *solve_lane;
  int solve_n_lane_pts;
  double solve_target_vel;
} mind_aime_plan_in;

#define MIND_AIME_BRANCH 1
#define MIND_AIME_END 2
#define MIND_AIME_TERMINATE 4
typedef struct {
  int round, scene, mode;      /* SCEN_ID = "{round}_{scene}_{mode}" (scenario_tree.py:321)                               */
  int parent;                  /* index of the parent node in this table, -1 = child of the root                          */
  float prob;                  /* SCEN_PROB (path probability, float32)                                                   */
  int cur_t, end_t;            /* CUR_T, END_T after the branching decisions                                              */
  int flags;                   /* MIND_AIME_BRANCH | _END | _TERMINATE of the internal tree node                          */
  int dur;                     /* steps of `rows` (END_T - CUR_T), 0 when the node is not on a finished branch            */
  int64_t row_off;             /* offset in floats of its rows [a, dur, 3] = (x, y, max-sigma) in out->rows, or -1        */
  float tgt_pts[22];           /* TGT_PTS [11,2] of the scene the node was predicted from                                 */
} mind_aime_node;

typedef struct {
  const mind_aime_node *nodes; /* library-owned host table [n_nodes] in creation order (= the internal tree's insertion order     */
  int n_nodes;                 /*   without its root), valid until the next mind_aime_plan call on this context                 */
  const float *rows;           /* library-owned host buffer [n_row_floats], same lifetime                                        */
  int64_t n_row_floats;
  int n_expanded, n_rounds;    /* scenes pushed through the predictor, rounds                                             */
  int root_flags;              /* flags of the internal root node                                                         */
  int round_scenes[32];        /* scenes of every round (for the caller's throughput accounting)                          */
  float pair_ms;               /* summed duration of the pair-kernel launches (HIP events; 0 unless profiling is on)      */
  int pair_launches;
  /* The cost trees TrajectoryTreeOptimizer builds from the returned scenario trees (trajectory_tree.py:19-124: LIFO depth-first
   * order, every even step of a node's window = one trajectory node), ready for mind_ilqr_contingency: one per root child on a
   * finished branch, in the order get_scenario_tree returns them.  Library-owned, same lifetime as `nodes`. */
  int n_trees;                 /* scenario trees                                                                          */
  const int32_t *tree_top;     /* [n_trees] index in `nodes` of every tree's top node                                     */
  const int32_t *tree_off;     /* [n_trees+1] trajectory-node offsets of the trees in the arrays below                    */
  const int32_t *flat_parent;  /* [M_total] parent key inside its tree, -1 for a tree's node 0                            */
  const float *flat_prob;      /* [M_total] sibling-normalised scenario probability (float32 arithmetic)                   */
  const float *flat_mean;      /* [M_total, a, 2]                                                                         */
  const float *flat_cov;       /* [M_total, a]                                                                            */
  int solves_begun;            /* the contingency solves were begun behind the plan (in->solve_cfg_full): mind_ilqr_finish_plan   */
} mind_aime_plan_out;

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU: one process (one mind_ctx) per GPU plans the SAME scene; the scenes of every AIME round of mind_aime_plan are
 * block-distributed over the ranks.  (The reference has no distributed code; the independence this rests on: the predictor loops
 * per scene, planners/mind/networks/network.py:318,497, and prune_merge works scene by scene, scenario_tree.py:281-412.)
 * Per round: every rank runs predictor + pruning + branch-time test on its block -> ONE all-gather of the decisions (96 B per
 * scene) -> every rank replays create_nodes / decide_branch on the same table (the tree is replicated, 0.2 ms at 1 555 nodes) ->
 * the rank that holds a branching node's parent scene re-bases it (update_obser, on the device) -> ONE small all-gather of the
 * children's frames (28 floats per scene: the replicated tree's node records; + LaneNet's output after the root round) and ONE
 * all-to-all that moves a re-based scene (predictor inputs + history windows, ~240 KB at 64 agents) from the rank that re-based it to
 * the rank whose block of the next round holds it -- on a full tree the two are the same rank except at the block boundaries, so only
 * the boundary scenes travel (skipped by every rank when nothing does).  At the end every rank packs the rows / cost tree entries of
 * the nodes whose predicted rows it holds and ONE all-reduce (sum over zero-filled buffers) completes them everywhere.  With
 * world == 1 the same code runs without exchanges.
 *
 * The transport is the caller's: a function that performs a collective on DEVICE buffers of this context's device,
 *   MIND_XCHG_ALLGATHER:  recv [world][bytes] <- every rank's send [bytes], in rank order;
 *   MIND_XCHG_ALLREDUCE:  recv [bytes / 4 words] <- sum over the ranks of send (send may equal recv).  Every word is non-zero on at most
 *                         one rank (its owner), so the transport should sum 32-bit INTEGERS: the owner's bits then arrive unchanged
 *                         (a float sum would turn an owner's -0.0 into +0.0).
 *   MIND_XCHG_ALLTOALLV:  the last argument is the ADDRESS of a host table int64 [2][world]: bytes this rank sends to / receives from every
 *                         rank; send / recv hold the per-rank segments packed in rank order (torch.distributed.all_to_all_single with split
 *                         sizes).
 * It is called with everything the library queued on the context's stream complete, and must return with the result complete
 * (mind_amd/parallel.py: torch.distributed -- RCCL over xGMI on a node, gloo in the tests).  world <= 1 or fn == NULL switches
 * the sharding off; force != 0 runs the exchanges of a one-rank group too (tests: RCCL on a one-GPU box). */
#define MIND_XCHG_ALLGATHER 0
#define MIND_XCHG_ALLREDUCE 1
#define MIND_XCHG_ALLTOALLV 2
typedef int (*mind_exchange_fn)(void *user, int op, void *send, void *recv, int64_t bytes);
int mind_set_exchange(mind_ctx *ctx, int rank, int world, mind_exchange_fn fn, void *user, int force);
/* collectives run and bytes received by this context's sharded plans so far */
int mind_last_exchange_stats(mind_ctx *ctx, long long *collectives, long long *bytes);

/* Returns MIND_ESTATE ("unsupported: ...") for the situations only the round-by-round host path handles -- a node re-expanded in a
 * later round than the one that created it, no finished branch (the host path raises the reference's assertion), more than
 * max_rounds rounds -- in which case the caller runs that path instead. */
int mind_aime_plan(mind_ctx *ctx, const mind_aime_plan_in *in, mind_aime_plan_out *out);
/* mind_aime_plan in two halves, for a host thread that plans several scenes (one context each): _begin copies *in (the arrays it
 * points to must stay valid until _finish) and runs the plan on a thread of the library; _poll returns 1 while it runs, 0 once
 * _finish will not block; _finish returns what mind_aime_plan would have.  No other call on the context between _begin and _finish
 * (a second _begin while the plan runs returns MIND_ESTATE; a finished plan that was never collected is dropped by the next _begin).
 * mind_ctx_busy: 1 while work queued on the context's stream has not completed (e.g. the contingency solves begun with
 * mind_ilqr_contingency_begin), 0 once collecting it will not block. */
/* collects the contingency solves a plan began itself (out->solves_begun): waits for them and copies the results of all its
 * scenario trees, concatenated in tree order: xs [n_nodes, 6], us [n_nodes, 2], the warm-start and full fits' statistics [n_trees].
 * n_nodes / n_trees = out->tree_off[out->n_trees] / out->n_trees of the plan the caller collects for: MIND_EINVAL (nothing copied) when
 * the pending solves belong to a plan of another shape, MIND_ESTATE when none is pending.  Solves that are never collected are
 * drained and dropped by the context's next mind_aime_plan. */
int mind_ilqr_finish_plan(mind_ctx *ctx, int n_nodes, int n_trees, double *xs, double *us, mind_ilqr_stats *stats_warm,
                          mind_ilqr_stats *stats_full);
int mind_aime_plan_begin(mind_ctx *ctx, const mind_aime_plan_in *in);
int mind_aime_plan_poll(mind_ctx *ctx);
int mind_aime_plan_finish(mind_ctx *ctx, mind_aime_plan_out *out);
int mind_ctx_busy(mind_ctx *ctx);

/* The array part of get_agent_trajectories (planners/mind/utils.py:245-342): raw [a,T,6] float64 rows (observed flag, x, y, heading, vx,
 * vy; T = 50) of the kept tracks, slot [a] = the type one-hot position of every track -> pos [a,T,2], ang [a,T], vel [a,T,2] float32 with the
 * positions / headings of unobserved steps taken from the nearest earlier observed step (the first observed one before it), velocities zero
 * there, typ [a,T,7] int16 one-hot on observed steps, have [a,T] int16.  Host arithmetic (copies and casts), no context needed. */
int mind_fill_tracks(const double *raw, int a, int T, const int32_t *slot, float *pos, float *ang, float *vel, int16_t *typ, int16_t *have);

/* MINDPlanner.evaluate_traj_tree (planners/mind/planner.py:180-198) for every candidate trajectory tree of a plan (host arithmetic,
 * float64, numpy's operation and summation order): states [sum counts, 6], ctrls [sum counts, 2] = the trees' nodes in key order, root
 * (x0, zero control) first; lane [P,2] float32 (lane_is_f32 != 0) or float64; out[n_trees] = mean node cost.  Needs no context. */
int mind_eval_traj_trees(const double *states, const double *ctrls, const int32_t *counts, int n_trees, const void *lane,
                         int lane_is_f32, int n_lane_pts, double target_vel, double *out);

/* ------------------------------------------------------------------------------------------------
 * The closed loop of one scene behind ONE call per simulator step (or per planning cycle): Simulator.run_sim (simulator.py:51-107),
 * CustomizedAgent.check_enable / check_trigger / step (agent.py:255-299), MINDAgent.observe / plan (agent.py:317-331), MINDPlanner.
 * update_observation / plan (planner.py:50-145), kine_propagate (common/kinematics.py:22-36).  A step = take-over check -> planner
 * trigger (every plan_step seconds) -> observation fan-out into the 50-frame windows of every track seen so far (unobserved tracks
 * repeat their last state with observed = false) -> when the agent is enabled: get_agent_trajectories (kept tracks, AV first) ->
 * mind_aime_plan with the device-built root and the plan-begun contingency solves -> mind_ilqr_finish_plan -> evaluate_traj_tree of
 * every candidate -> the reference's strict `<` scan -> first control -> ego plant.  Everything the interpreter did between the two
 * device waits of a cycle happens here; mind_amd/closed_loop.py ClosedLoopSim.step calls it once and reads the plan's objects only
 * when somebody asks for them (mind_loop_last_plan).  Exo agents are replayed from tables the caller tabulated once (one row per
 * simulator step, built with the driver's own observation code, so the windows hold the same float64 values).
 * Host arithmetic is float64 in the reference's operation order; sin / cos / tan are the C library's (the Python driver uses
 * math.sin / math.cos / math.tan for the same expressions).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mind_loop mind_loop;
typedef struct {
  /* replayed scene, one row per simulator step n (sim_time = n additions of sim_step): tables are copied */
  int n_tracks;                 /* tracks of the world, track 0 = the closed-loop agent ("AV")                                  */
  int n_steps;                  /* rows of the tables below                                                                     */
  int clamp_last;               /* != 0: steps >= n_steps read row n_steps - 1 (a recording that holds its last frame)          */
  const double *ego_state;      /* [n_steps][4] world.agent_state(0, t_n) = (x, y, v, yaw): observation before the take-over and    */
                                /*   the state taken over at enable_time                                                        */
  int ego_state_is_f32;         /* world.agent_state returns float32 arrays (the reference's loader keeps tracks in float32,       */
                                /*   loader.py:166-168): numpy then evaluates the FIRST plant step after the take-over in float32   */
                                /*   (Python floats are weak operands, the state array is float64 from the second step on)          */
  const double *ego_obs;        /* [n_steps][5] ObjectState of the RECORDED ego at step n (x, y, heading, vx, vy), as the driver's     */
                                /*   to_object_state builds it: the ego's window entry before the take-over and at the take-over step  */
  const float *ego_trig32;      /* [n_steps][2] numpy's float32 cos / sin of the recorded yaw (the first plant step after a take-over  */
                                /*   from a float32 recording uses them); may be NULL when ego_state_is_f32 == 0                      */
  /* numpy's elementary functions where they are not the C library's: on AVX-512 hosts np.tan (float64) is a SIMD routine that differs
   * from libm's by an ulp in 0.5 % of the arguments, and the reference's plant (kinematics.py:22-36) calls np.tan.  NULL = the C library's
   * tan / sin / cos.  tan_fn is called once per control (the steer angle is constant between two plans), sincos_fn once per step. */
  double (*tan_fn)(double);
  void (*sincos_fn)(double, double *sin_cos);
  const double *exo_obs;        /* [n_steps][n_tracks][5] ObjectState of track i at step n: x, y, heading, vx, vy (row 0 unused)    */
  const uint8_t *exo_valid;     /* [n_steps][n_tracks] the track is reported at step n (simulator.py:60-63)                       */
  const int32_t *timestep;      /* [n_steps] ObjectState.timestep = int(round(t_n / 0.1))                                        */
  const int32_t *type_slot;     /* [n_tracks] one-hot slot of the track's object type (utils.py:245-342)                          */
  /* simulator + ego plant (simulator.py:51-107, agent.py:255-299, kinematics.py:22-36) */
  double sim_step, plan_step, enable_time;
  double wheelbase, max_speed, max_steer, max_acc, max_dec;
  /* planner constants of the scene (planner.py:147-171, scenario_tree.py:106-126): as mind_aime_plan_in with the device-built root */
  int n_lanes; const double *lane_pts; const int32_t *lane_flags;      /* [l,11,2], [l,6]                                       */
  int n_lane_pts; const float *target_lane, *target_lane_info;         /* resampled target lane [P,2], info [P,12]               */
  double time_ahead; float min_vel, dist_thres; int max_depth, max_rounds, pred_len; float prob_floor;
  /* contingency solves (planner.py:174-178) and candidate evaluation (planner.py:180-198) */
  const mind_ilqr_cfg *cfg_warm, *cfg_full;
  int solve_n_lane_pts; const double *solve_lane;                      /* gt_tgt_lane [P',2] float64                              */
  double target_vel;
  int eval_n_lane_pts, eval_lane_is_f32; const void *eval_lane;        /* lcl_smp.target_lane [P'',2] in its own dtype            */
  /* != 0: the speculative warm start of this repo's TrajectoryTreeOptimizer (trajectory_tree.py speculate_warm): the warm-start fits of
   * the previous plan's tree shapes run on a second context of the loop beside the AIME rounds; a tree whose shape recurs runs the full fit
   * only.  Same kernels on the same inputs: the results are the same bits either way; it pays when several loops share the device. */
  int speculative;
} mind_loop_desc;

/* running totals over every plan of the loop since it was created (a caller's accounting takes differences) */
typedef struct {
  long long plans, expansions, scen_trees, rounds;
  double aime_s, ilqr_s, total_s;   /* host wall time: the AIME call | collecting the solves | the whole planning cycle                */
  long long iterations, node_iterations, node_iterations_exo;      /* warm + full fits (TrajectoryTreeOptimizer.counters)              */
  long long warm_speculated, warm_hits;                             /* speculated warm-start fits begun / used                           */
  /* with profiling on (mind_set_profiling): kernel durations from HIP events on the context stream, as mind_aime_plan_out.pair_ms /
   * mind_last_ilqr_stats / mind_last_ilqr_profile report them per call */
  double pair_ms; long long pair_launches;
  double scene_n2, scene_n_a1;      /* sums over the expanded scenes of N^2 and N (a + 1), N = a + l + 1 tokens (algorithmic FLOPs / bytes) */
  double ilqr_ms; long long ilqr_launches, ilqr_trees; int ilqr_workgroups_per_tree;
  double ilqr_prof[9], ilqr_node_steps;
} mind_loop_totals;

typedef struct {
  int planned;                  /* the call computed at least one plan                                                          */
  int enabled;
  long long n_steps, n_plans;   /* since the loop was created (resets do not clear them)                                        */
  long long episode_steps;      /* simulator steps of the current episode (= table row of the next step)                          */
  double sim_time, last_trigger;    /* last_trigger < 0: none yet                                                               */
  double state[4], ctrl[2];     /* ego plant state (x, y, v, yaw) and the control in force                                      */
  /* the last plan */
  int n_agents, n_trees, best, n_expanded, n_rounds, n_traj_nodes;
  const double *costs;          /* [n_trees] library-owned, valid until the loop's next plan                                    */
  double aime_s, ilqr_s, total_s;
  mind_loop_totals tot;
} mind_loop_out;

/* the loop runs on `ctx` (weights loaded; not sharded); one loop per context at a time plans */
int mind_loop_create(mind_ctx *ctx, const mind_loop_desc *desc, mind_loop **out);
int mind_loop_destroy(mind_loop *loop);
/* ClosedLoopSim._start_episode: scene back to t = 0, windows cleared, agent disabled (n_steps / n_plans keep counting) */
int mind_loop_reset(mind_loop *loop);
/* Steps until `until_plans` more plans were computed (> 0), or sim_time >= until_time - 1e-9 (until_time >= 0: ClosedLoopSim.run_until),
 * or `max_steps` steps were taken -- whichever comes first; until_plans = 0, until_time < 0, max_steps = 1 is ClosedLoopSim.step.
 * MIND_ESTATE "unsupported: ..." = a plan only the round-by-round host path handles (see mind_aime_plan): the step's observation update has
 * happened, the plan and the rest of the step have not; the caller takes the loop over (mind_loop_export) and finishes the step on the host. */
int mind_loop_advance(mind_loop *loop, int until_plans, double until_time, long long max_steps, mind_loop_out *out);
/* the state of the loop without stepping */
int mind_loop_state(mind_loop *loop, mind_loop_out *out);
/* The last plan's tables for a caller that builds the reference's objects from them (scenario trees, trajectory trees): *plan as
 * mind_aime_plan returned it, the solves' results concatenated in tree order (xs [n_traj_nodes,6], us [n_traj_nodes,2], statistics
 * [n_trees]), the tracks of the plan's agents (index into the world's tracks, AV first) and their TRAJS_TYPE [a,50,7] float32.
 * Library-owned, valid until the next plan on the loop's context; MIND_ESTATE when another plan ran on the context since (a context may be
 * shared by several planners). */
int mind_loop_last_plan(mind_loop *loop, mind_aime_plan_out *plan, const double **xs, const double **us, const mind_ilqr_stats **stats_warm,
                        const mind_ilqr_stats **stats_full, const int32_t **agent_tracks, const float **types, double *x0);
/* Hands the loop over to a host driver (ClosedLoopSim falls back to its Python steps: a planner attribute changed under it, a plan the
 * library reports unsupported): the tracks seen so far in first-appearance order (track 0 first), their window lengths and rows
 * [n][50][7] = (observed, x, y, heading, vx, vy, timestep), oldest first, the first `count` rows of every window used.  cap = tracks the
 * arrays hold; the number of tracks comes back in *n (MIND_EINVAL with *n set when cap is too small). */
int mind_loop_export(mind_loop *loop, int cap, int *n, int32_t *track, int32_t *count, double *rows);

/* ------------------------------------------------------------------------------------------------
 * MINDPlanner.plan() behind ONE call, for a caller that keeps the simulator: the reference's simulator.py / agent.py (agent.py:317-331
 * update_observation -> update_state_ctrl -> plan), a world whose observations are noisy or react to the ego, a co-simulation that
 * delivers one frame at a time -- nothing that could be tabulated ahead of time as mind_loop_desc wants it.  The caller pushes one
 * observation frame per planner trigger (mind_planner_observe = MINDPlanner.update_observation, planner.py:50-64) and asks for a plan
 * with the current ego state (mind_planner_plan = MINDPlanner.plan, planner.py:66-145): get_agent_trajectories (utils.py:245-342; AV
 * first, tracks whose last state is unobserved dropped, windows left-padded) -> mind_fill_tracks -> mind_aime_plan with the device-built
 * root and the plan-begun contingency solves -> collect -> evaluate_traj_tree of every candidate (planner.py:180-198; priced while the
 * solves still run) -> the reference's strict `<` scan (planner.py:131-136) -> first control (planner.py:138-141).  It is the cycle of
 * mind_loop, the same code on the same kernels: a mind_loop step and a mind_planner_plan on the same windows give the same bits.
 * The plant, the clock and who is visible stay with the caller.
 * mind_planner_observe / _reset / _export touch no device and work on a planner created with ctx = NULL; every other call on such a
 * planner returns MIND_ESTATE.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mind_planner mind_planner;
#define MIND_PLANNER_EGO_KEY (-0x7fffffffffffffffLL - 1)   /* the key under which the ego's own track ("AV") is reported; not a caller's key */
typedef struct {
  /* what does not change with the frame; the fields mind_loop_desc has under the same names, with the same meaning */
  double time_ahead; float min_vel, dist_thres; int max_depth, max_rounds, pred_len; float prob_floor;
  const mind_ilqr_cfg *cfg_warm, *cfg_full;      /* copied */
  int speculative;
  int ego_type_slot;            /* one-hot slot of the ego's object type (utils.py:245-342)                                     */
} mind_planner_desc;

typedef struct {
  long long n_plans;            /* plans computed since the planner was created (resets do not clear it)                         */
  /* the last plan (zero while the planner holds none: before the first plan, after a reset, after a plan that failed) */
  int n_agents, n_trees, best, n_expanded, n_rounds, n_traj_nodes;
  const double *costs;          /* [n_trees] library-owned, valid until the planner's next plan                                 */
  double ctrl[2];               /* the chosen control (a, delta)                                                                 */
  double aime_s, ilqr_s, total_s;
  mind_loop_totals tot;         /* running totals over every plan of the planner                                                 */
} mind_planner_out;

/* ctx: a context with weights loaded (not sharded), or NULL for a planner that only keeps windows */
int mind_planner_create(mind_ctx *ctx, const mind_planner_desc *desc, mind_planner **out);
int mind_planner_destroy(mind_planner *planner);
/* ClosedLoopSim._start_episode: the windows are cleared and the last plan is forgotten (mind_planner_last_plan reports MIND_ESTATE until
 * the next plan); the scene tables and the running totals stay */
int mind_planner_reset(mind_planner *planner);
/* MINDPlanner.update_observation (planner.py:50-64) for one frame: ego[5] and rows[n][5] = (x, y, heading, vx, vy) as the caller's
 * to_object_state built them (float32 recordings and numpy's elementary functions are the caller's business, as with
 * mind_loop_desc.ego_obs), `timestep` the frame's ObjectState.timestep.  Tracks are keyed by caller-chosen integers: a key seen for the
 * first time joins behind the tracks known so far (type_slot is read then), a known track missing from the frame repeats its last state
 * with observed = false, windows hold 50 frames.  MIND_EINVAL (nothing changed): a NULL pointer, n < 0, a key twice in one frame,
 * MIND_PLANNER_EGO_KEY among the keys, a type slot outside 0..6. */
int mind_planner_observe(mind_planner *planner, int timestep, const double *ego, int n, const long long *track_key, const int32_t *type_slot,
                         const double *rows);
/* The scene tables mind_loop_desc takes once, settable at any time between two plans (a target lane that changes during the run):
 * lane_pts [n_lanes,11,2] float64 + lane_flags [n_lanes,6]; the resampled target lane [n,2] + info [n,12] float32 (n >= 12);
 * gt_tgt_lane [n,2] float64 + target velocity of the contingency solves; lcl_smp.target_lane [n,2] in its own dtype for the candidate
 * evaluation (which reads the same target velocity).  Tables are copied; a call with a table equal to the planner's copy changes nothing.
 * The next plan carries the tables to the device in its own staging upload, as every mind_aime_plan does. */
int mind_planner_set_lanes(mind_planner *planner, int n_lanes, const double *lane_pts, const int32_t *lane_flags);
int mind_planner_set_target_lane(mind_planner *planner, int n, const float *lane, const float *info);
int mind_planner_set_solve_lane(mind_planner *planner, int n, const double *lane, double target_vel);
int mind_planner_set_eval_lane(mind_planner *planner, int n, const void *lane, int is_f32);
/* The cycle (MINDPlanner.update_state_ctrl + plan): state = the ego's (x, y, v, yaw), ctrl = the control in force (a, delta).
 * MIND_ESTATE: no observation yet, a table not set, a sharded context; MIND_ESTATE "unsupported: ..." has the meaning it has in
 * mind_loop_advance: the plan is left to the round-by-round host path.  Whatever the code, the windows are intact: the caller may set
 * what was missing and plan again, or take the windows over (mind_planner_export).  *out is filled in every case. */
int mind_planner_plan(mind_planner *planner, const double *state, const double *ctrl, mind_planner_out *out);
/* as mind_loop_last_plan; agent_keys [n_agents] = the keys of the plan's agents, MIND_PLANNER_EGO_KEY first */
int mind_planner_last_plan(mind_planner *planner, mind_aime_plan_out *plan, const double **xs, const double **us, const mind_ilqr_stats **stats_warm,
                           const mind_ilqr_stats **stats_full, const long long **agent_keys, const float **types, double *x0);
/* as mind_loop_export: the tracks in first-appearance order (the ego first, under MIND_PLANNER_EGO_KEY, once it has a frame) */
int mind_planner_export(mind_planner *planner, int cap, int *n, long long *key, int32_t *count, double *rows);

/* ------------------------------------------------------------------------------------------------
 * planners/ilqr call surface (iLQR.fit over a TreeCost of arbitrary PotentialField / StatePotential /
 * StateConstraint / ControlPotential objects; solver.py:80-167, cost.py:326-446, potential.py:62-264).
 * The grid is what PotentialField.__init__ receives: field_offset, resolution, xx[0,:], yy[:,0].
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int W, H;                 /* cost_field.shape = (H, W)                                          */
  double res;               /* resolution                                                         */
  double off_x, off_y;      /* field_offset                                                       */
  const double *gx, *gy;    /* HOST [W] = xx[0,:], [H] = yy[:,0]                                  */
} mind_field_grid;

/* gen_dist_field (ilqr/utils.py:5-22): grid of W x H centroids centred on ego_xy, distance of each to
 * the polyline `lane` [n_pts,2].  Outputs HOST offset[2] (field_offset), gx[W] (= xx[0,:]), gy[H]
 * (= yy[:,0]), dist[H,W]. */
int mind_lane_dist_field(mind_ctx *ctx, const double *ego_xy, const double *lane, int n_pts, int W, int H,
                         double res, double *offset, double *gx, double *gy, double *dist);

/* iLQR.fit on trees whose nodes carry materialised cost fields and their own quadratic potentials
 * (tree[i].field / .node_w set; .prob / agents ignored).  cfg supplies dt, wheelbase, max_iter only. */
int mind_ilqr_solve_fields(mind_ctx *ctx, const mind_ilqr_cfg *cfg, const mind_field_grid *grid,
                           const mind_cost_tree *trees, int n_trees, const double *x0,
                           const double *us_init, double *xs, double *us, mind_ilqr_stats *stats);

/* TreeCost.l / l_x / l_u / l_xx / l_uu (cost.py:341-446) of ONE tree at arbitrary points:
 * out HOST [n_query, 47] = { l, l_x[6], l_u[2], l_xx[36] row-major, diag l_uu[2] } for node[q] at
 * (x[q], u[q]).  grid == NULL: planner mode (fields from prob / agents / target lane as in
 * mind_ilqr_solve_trees); grid != NULL: generic mode (tree->field / node_w; lane arguments ignored). */
int mind_cost_eval(mind_ctx *ctx, const mind_ilqr_cfg *cfg, const mind_field_grid *grid,
                   const mind_cost_tree *tree, const double *x0, const double *target_lane,
                   int n_lane_pts, double target_vel, int use_exo, int n_query,
                   const int32_t *node, const double *x, const double *u, double *out);

/* Rollout + TreeCost of n_cand candidate control trees per cost tree, no optimisation (solver.py:255-330
 * without the derivatives).  grid == NULL: planner mode, arguments as mind_ilqr_solve_trees; grid != NULL:
 * generic mode as mind_ilqr_solve_fields (lane arguments ignored).  us_cand HOST [n_cand, sum M, 2];
 * outputs HOST xs [n_cand, sum M, 6] (NULL = not wanted), L [n_cand, sum M] (NULL = not wanted),
 * J [n_cand, n_trees] = numpy-order sum of the tree's L. */
int mind_ilqr_score_trees(mind_ctx *ctx, const mind_ilqr_cfg *cfg, const mind_field_grid *grid,
                          const mind_cost_tree *trees, int n_trees, const double *x0,
                          const double *target_lane, int n_lane_pts, double target_vel, int use_exo,
                          int n_cand, const double *us_cand, double *xs, double *L, double *J);

/* The gains of ONE backward pass (solver.py:332-373; the rule they feed: solver.py:202-253) about the controls
 * us HOST [sum M, 2], with the regularisation mu HOST [n_trees] (>= 0), on every cost tree; no optimisation.
 * grid selects the planner or the generic mode as in mind_ilqr_score_trees.  Outputs HOST, rows in key order, tree
 * after tree: k [sum M, 2], K [sum M, 2, 6], dV [sum M], V_x [sum M, 6], V_xx [sum M, 6, 6] (the values after the
 * node's own update), the nominal xs [sum M, 6] = rollout of us, L [sum M], J [n_trees] = numpy-order sum of L,
 * bad_node [n_trees].  k, K and bad_node are required, the others may be NULL.  The reference's root key -1
 * aliases numpy row -1, so ITS V_x / V_xx row M-1 also holds node 0's value; here row M-1 is that node's own.
 * A singular Q_uu is no error: bad_node[t] = the lowest key among the nodes whose own Q_uu was singular while all
 * their descendants were fine (-1: none); that tree's k, K, dV, V_x, V_xx are zeros, its xs / L / J are valid.
 * One workgroup per tree: meant for planner-size trees (a 12 288-node tree is served, but slowly). */
typedef struct {
  double *k, *K, *dV, *V_x, *V_xx, *xs, *L, *J;
  int32_t *bad_node;
} mind_ilqr_gains_out;
int mind_ilqr_gains(mind_ctx *ctx, const mind_ilqr_cfg *cfg, const mind_field_grid *grid,
                    const mind_cost_tree *trees, int n_trees, const double *x0, const double *target_lane,
                    int n_lane_pts, double target_vel, int use_exo, const double *us, const double *mu,
                    const mind_ilqr_gains_out *out);

/* Closed-loop rollouts under given gains (the line search's rule, solver.py:202-253, with the gains of
 * solver.py:332-373): candidate c, with the step size alpha[c] and the start offset dx0[c] (HOST [n_cand, 6];
 * NULL = zeros), applies at node i with parent p
 *   u_new[i] = us[i] + alpha[c] k[i] + K[i] (x_new[p] - xs[p]),   x_new[i] = f(x_new[p], u_new[i]),
 * xs = the nominal states, recomputed from us by the call; for node 0 the pair is (x0 + dx0[c], x0) -- the one
 * extension over the reference, whose node 0 has no feedback term.  us HOST [sum M, 2], k [sum M, 2], K [sum M, 2, 6],
 * alpha [n_cand].  Outputs HOST xs [n_cand, sum M, 6], us_out [n_cand, sum M, 2], L [n_cand, sum M] (each may be
 * NULL), J [n_cand, n_trees] = the LINE SEARCH's sum of the tree's L: sequential from 0.0 in key order (python's
 * sum()), not the numpy-order sum mind_ilqr_score_trees reports.  Modes, limits and MIND_ESTATE as
 * mind_ilqr_score_trees. */
int mind_ilqr_policy_rollouts(mind_ctx *ctx, const mind_ilqr_cfg *cfg, const mind_field_grid *grid,
                              const mind_cost_tree *trees, int n_trees, const double *x0, const double *target_lane,
                              int n_lane_pts, double target_vel, int use_exo, const double *us, const double *k,
                              const double *K, int n_cand, const double *alpha, const double *dx0, double *xs,
                              double *us_out, double *L, double *J);

/* ------------------------------------------------------------------------------------------------
 * Clearance audit of plans and closed-loop episodes (mind_amd/csrc/box_geom.h, audit_kernels.hip).  The reference gives
 * every agent a BBox by object type (agent.py:92-105, common/bbox.py), draws it centred on state[:2]
 * (visualization.py:69-72) and never tests it against anything; evaluate_traj_tree (planner.py:180-198) ignores every exo
 * agent.  These calls say what a plan or an episode did to the other road users.  They sit outside every planning cycle:
 * synchronous on the context's stream, with scratch of their own.  Hit convention: clearance < 0 (touching, 0.0, is no hit).
 * A box is {length, width, center_offset}: its centre is (x, y) + center_offset (cos yaw, sin yaw); 0 is the reference's
 * footprint convention.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { double length, width, center_offset; } mind_audit_box;

/* n_cand candidate state sets xs HOST [n_cand, sum M, 6] (rows in key order, tree after tree, as mind_ilqr_score_trees
 * returns them) on the cost trees of a plan; only n_nodes, prob, n_agents, agent_mean and agent_cov of the trees are read.
 * For trajectory node i of tree t, paired with agent_mean[i] as the solver pairs them (trajectory_tree.py:78-118),
 *   node_clear[i] = min over exo agents j = 1..a_t-1 of
 *                   dist(mean[i,j] -> ego box at xs[i], yaw xs[i][3]) - ((double)cov[i,j] + exo_margin),
 * the signed distance of the disc the exo term prices (trajectory_tree.py:95-102) to the ego box; node_agent[i] = that j,
 * the lowest winning ties; a_t == 1: +inf / -1.  Per (candidate, tree): tree_min with tree_node and tree_agent (the lowest
 * key wins ties), tree_hits = nodes with clearance < 0, tree_first = the lowest such key (-1: none), tree_mass = the
 * sequential key-order sum from 0.0 of (double)prob[i] over the hit nodes.  A node whose state is not finite reports
 * NaN / -1, and its tree min = NaN, node = that key, agent = -1, hits = -1, first = -1, mass = NaN.
 * Outputs HOST, each may be NULL (not all): node_* [n_cand, sum M], tree_* [n_cand, n_trees].
 * MIND_EINVAL: a NULL required pointer, a negative count, a non-finite or negative box dimension, margin or cov, a
 * non-finite mean, all outputs NULL, n_cand x sum M > 2^20.  n_cand == 0 is a successful no-op.  MIND_ESTATE while a plan
 * begun with mind_aime_plan_begin runs or a tree-iLQR call begun on the context is pending. */
typedef struct {
  double *node_clear; int32_t *node_agent;
  double *tree_min; int32_t *tree_node, *tree_agent, *tree_hits, *tree_first; double *tree_mass;
} mind_audit_plan_out;
int mind_audit_plan(mind_ctx *ctx, const mind_audit_box *ego, double exo_margin, const mind_cost_tree *trees,
                    int n_trees, int n_cand, const double *xs, const mind_audit_plan_out *out);

/* n_ego ego traces ego_states HOST [n_ego, n_steps, 4] = (x, y, v, yaw) against one replayed scene: exo HOST
 * [n_steps, n_tracks, 5] = (x, y, heading, vx, vy) and valid HOST [n_steps, n_tracks] uint8, the layouts of
 * mind_loop_desc.exo_obs / exo_valid (row 0 is the ego's and is not read); boxes HOST [n_tracks, 2] = (length, width)
 * centred on the track's (x, y).  Per (ego, step): step_clear = the minimum signed rectangle-rectangle clearance over
 * the valid tracks 1..n_tracks-1 and step_track = that track, the lowest winning ties; no valid track: +inf / -1.  Per ego:
 * ego_min with ego_step and ego_track (the lowest step wins ties), ego_hits = steps with clearance < 0, ego_first = the
 * first of them (-1: none).  Outputs HOST, each may be NULL (not all): step_* [n_ego, n_steps], ego_* [n_ego].
 * MIND_EINVAL: a NULL required pointer, a negative count, n_tracks < 1, a non-finite or negative box dimension, a
 * non-finite ego state or valid track row, all outputs NULL, n_ego x n_steps > 2^22, n_steps x n_tracks > 2^24.
 * n_ego == 0 or n_steps == 0 is a successful no-op.  MIND_ESTATE as mind_audit_plan. */
typedef struct {
  double *step_clear; int32_t *step_track;
  double *ego_min; int32_t *ego_step, *ego_track, *ego_hits, *ego_first;
} mind_audit_episode_out;
int mind_audit_episode(mind_ctx *ctx, const mind_audit_box *ego, int n_ego, int n_steps, int n_tracks,
                       const double *ego_states, const double *exo, const uint8_t *valid, const double *boxes,
                       const mind_audit_episode_out *out);

/* box_geom.h on the CPU (host only, no context): n pairs, a HOST [n, 5] = (x, y, yaw, L, W), the offset taken as b - a.
 * kind 0: rectangle a against the disc b = (x, y, r, -, -): bg_point_rect - r.  kind 1: rectangle a against the rectangle
 * b [n, 5]: bg_rect_rect.  trig HOST [n, 4] = (cos a, sin a, cos b, sin b), or NULL = the kernels' own sin / cos
 * (mind_trig.h).  out HOST [n].  MIND_EINVAL for another kind, n < 0 or a NULL pointer. */
int mind_debug_box_clearance(int kind, int n, const double *a, const double *b, const double *trig, double *out);

/* ------------------------------------------------------------------------------------------------
 * Forecast scoring (mind_amd/csrc/forecast_score.h, forecast_kernels.hip): what the predictor said about the other road
 * users against what they went on to do.  The reference carries reg [a,6,60,5] = (x, y, sx, sy, exp rho) per agent in the
 * agent-local frame (network.py:545), prices every other agent as a disc of radius max(sx, sy) + w_exo_cov_offset around
 * the predicted mean (trajectory_tree.py:95-102, scenario_tree.py:325) and never compares either with a recorded future.
 * Like the audit this call sits outside every planning cycle: synchronous on the context's stream (a mind_predict_batch
 * queued before it is ordered in front), with scratch of its own.
 *
 * Inputs: reg DEVICE [A, K, T, 5] and cls DEVICE [B, K] exactly as mind_pred_out holds them (K = 6, T = 60 there); gt HOST
 * [A, T, 2] float64, the truth in the same agent-local frame; valid HOST [A, T] uint8; scored HOST [A] uint8 or NULL = all;
 * actor_off HOST [B + 1], actor_off[0] = 0.  cfg: K in 1..8, T in 1..256, n_h in 1..4 horizons, strictly ascending within
 * 1..T (horizon h covers the samples t < horizon[h]); miss_radius, disc_scale, disc_offset finite and >= 0.
 *
 * Per valid sample, after conversion to double: d = sqrt(dx dx + dy dy), inside when d <= disc_scale max(sx, sy) + disc_offset.
 * Per (agent, horizon, mode) over the valid samples below the horizon in ascending t: ade = (sequential sum of d) / n_valid,
 * fde = d at the last valid sample, cover = inside samples, first_out = the first sample not inside (-1: none); no valid
 * sample: NaN, NaN, 0, -1.  Per (agent, horizon): n_valid, last (-1: none), k_ade / k_fde = the arg-minima over the modes
 * (the lowest k wins ties, a NaN never wins, -1 when every mode is NaN or +inf), brier_fde = fde[k_fde] + (1 - cls[b, k_fde])^2
 * (NaN for -1).  Per (scene, horizon) over the agents with scored[a] and n_valid > 0, in index order: s_n_scored, s_ade[k] /
 * s_fde[k] = the means over those agents (sequential sums; NaN without one), s_k_ade, s_k_fde, s_brier_fde as above -- the
 * joint metrics: one mode index serves every agent of the scene --, s_miss_rate = the share of those agents with
 * fde[a, h, s_k_fde] > miss_radius, s_k_top = argmax cls[b] (the lowest k on ties), s_miss_top = the same share at s_k_top.
 * A non-finite forecast value has no special case: the arithmetic and comparisons decide (forecast_score.h).
 * Outputs HOST, each may be NULL (not all).
 * MIND_EINVAL: a NULL required pointer, K, T, n_h or a horizon out of range or not ascending, a negative or non-finite
 * radius, scale or offset, actor_off not starting at 0 or not monotone, a non-finite gt at a valid sample, all outputs NULL,
 * A > 2^20.  A == 0 or n_scenes == 0 is a successful no-op; an empty scene inside a batch is legal.  MIND_ESTATE as
 * mind_audit_plan. */
typedef struct { int K, T, n_h; const int32_t *horizon; double miss_radius, disc_scale, disc_offset; } mind_forecast_cfg;
typedef struct {
  double *ade, *fde; int32_t *cover, *first_out;                                           /* [A, n_h, K] */
  int32_t *n_valid, *last, *k_ade, *k_fde; double *brier_fde;                              /* [A, n_h] */
  int32_t *s_n_scored; double *s_ade, *s_fde;                                              /* [B, n_h], [B, n_h, K] x 2 */
  int32_t *s_k_ade, *s_k_fde, *s_k_top; double *s_brier_fde, *s_miss_rate, *s_miss_top;    /* [B, n_h] */
} mind_forecast_out;
int mind_forecast_score(mind_ctx *ctx, const mind_forecast_cfg *cfg, int n_scenes, const int32_t *actor_off,
                        const float *reg, const float *cls, const double *gt, const uint8_t *valid,
                        const uint8_t *scored, const mind_forecast_out *out);

/* forecast_score.h on the CPU (host only, no context): the same call with reg / cls HOST. */
int mind_debug_forecast_score(const mind_forecast_cfg *cfg, int n_scenes, const int32_t *actor_off, const float *reg,
                              const float *cls, const double *gt, const uint8_t *valid, const uint8_t *scored,
                              const mind_forecast_out *out);

/* ------------------------------------------------------------------------------------------------
 * Road audit of plans and closed-loop episodes (mind_amd/csrc/road_geom.h, road_kernels.hip): what the ego did to the ROAD.
 * Every AV2 map carries `drivable_areas` polygons beside `lane_segments`; the reference reads the file and never looks at
 * them, and no cost term of the tree-iLQR knows where the pavement ends.  Like the clearance audit these calls sit outside
 * every planning cycle: synchronous on the context's stream, with scratch of their own.
 *
 * A road is n_rings >= 1 rings: verts HOST [V, 2] float64 world coordinates and poly_off HOST [n_rings + 1], poly_off[0] = 0,
 * ring r = the vertices poly_off[r] .. poly_off[r + 1] - 1, implicitly closed (last -> first), at least three, no holes.
 * The ego box is a mind_audit_box at (x, y, yaw).  Per corner, in the order (+,+), (+,-), (-,-), (-,+) of (long, lat): in at
 * least one ring, its margin = the maximum over the containing rings of the distance to that ring's boundary; otherwise
 * -(the minimum over all rings of that distance).  Outside this is the exact distance to the road; inside it is a LOWER
 * BOUND of the distance to the boundary of the rings' union, exact wherever rings neither overlap nor abut near the point.
 * Per box: margin = the minimum over the corners (the first wins ties) with that corner, its ring and its edge (index within
 * the ring; edge e joins vertex e to vertex e + 1, the last to the first); corners only -- a verge passing under the middle
 * of a box whose corners are all inside is not seen.  Hit: margin < 0; touching (0.0) is no hit.  A state row holding a
 * non-finite value reports NaN / -1 / -1 / -1.  A duplicated vertex (a zero-length edge) is skipped.
 * ---------------------------------------------------------------------------------------------- */

/* n_cand candidate state sets xs HOST [n_cand, sum M, 6] (as mind_audit_plan takes them) on the cost trees of a plan; only
 * n_nodes and prob of the trees are read.  Per node: node_margin, node_corner, node_ring, node_edge.  Per (candidate, tree):
 * tree_min with tree_node and tree_corner (the lowest key wins ties), tree_hits = nodes with margin < 0, tree_first = the
 * lowest such key (-1: none), tree_mass = the sequential key-order sum from 0.0 of (double)prob[i] over the hit nodes; a tree
 * holding a NaN node: min = NaN, node = that key, corner = -1, hits = -1, first = -1, mass = NaN.
 * Outputs HOST, each may be NULL (not all): node_* [n_cand, sum M], tree_* [n_cand, n_trees].
 * MIND_EINVAL: a NULL required pointer, a negative count, n_rings < 1 or > 2^16, a ring of fewer than three vertices,
 * poly_off not starting at 0 or not ascending, more than 2^20 vertices, a non-finite vertex, a non-finite or negative box
 * dimension, all outputs NULL, n_cand x sum M > 2^20.  n_cand == 0 is a successful no-op.  MIND_ESTATE as mind_audit_plan. */
typedef struct {
  double *node_margin; int32_t *node_corner, *node_ring, *node_edge;
  double *tree_min; int32_t *tree_node, *tree_corner, *tree_hits, *tree_first; double *tree_mass;
} mind_audit_road_plan_out;
int mind_audit_road_plan(mind_ctx *ctx, const mind_audit_box *ego, const double *verts, const int32_t *poly_off, int n_rings,
                         const mind_cost_tree *trees, int n_trees, int n_cand, const double *xs,
                         const mind_audit_road_plan_out *out);

/* n_ego ego traces ego_states HOST [n_ego, n_steps, 4] = (x, y, v, yaw).  Per (ego, step): step_margin, step_corner,
 * step_ring, step_edge.  Per ego: ego_min with ego_step and ego_corner (the lowest step wins ties), ego_hits = steps with
 * margin < 0, ego_first = the first of them (-1: none); a trace holding a NaN step: min = NaN, step = the first such step,
 * corner = -1, hits = -1, first = -1.  Outputs HOST, each may be NULL (not all): step_* [n_ego, n_steps], ego_* [n_ego].
 * MIND_EINVAL as above, with n_ego x n_steps > 2^22 in place of the plan's cap.  n_ego == 0 or n_steps == 0 is a successful
 * no-op.  MIND_ESTATE as mind_audit_plan. */
typedef struct {
  double *step_margin; int32_t *step_corner, *step_ring, *step_edge;
  double *ego_min; int32_t *ego_step, *ego_corner, *ego_hits, *ego_first;
} mind_audit_road_episode_out;
int mind_audit_road_episode(mind_ctx *ctx, const mind_audit_box *ego, const double *verts, const int32_t *poly_off,
                            int n_rings, int n_ego, int n_steps, const double *ego_states,
                            const mind_audit_road_episode_out *out);

/* road_geom.h on the CPU (host only, no context): n boxes HOST [n, 3] = (x, y, yaw) of the box `ego` against the road.
 * trig HOST [n, 2] = (cos yaw, sin yaw), or NULL = the kernels' own sin / cos (mind_trig.h).  Outputs HOST [n], each may be
 * NULL (not all).  MIND_EINVAL for n < 0, a NULL required pointer, a bad box or a bad road (the rules above). */
int mind_debug_road_margin(int n, const double *boxes, const mind_audit_box *ego, const double *verts,
                           const int32_t *poly_off, int n_rings, const double *trig, double *margin, int32_t *corner,
                           int32_t *ring, int32_t *edge);

/* ------------------------------------------------------------------------------------------------
 * Time-to-collision audit of closed-loop episodes (mind_amd/csrc/ttc_geom.h, ttc_kernels.hip): how CLOSE to a collision the
 * ego drove.  The clearance audit says whether the ego box touched another; an episode that never did can still have spent
 * seconds one brake-tap from a rear-end collision.  The reference gives every agent a BBox by object type (agent.py:92-105),
 * draws it (visualization.py:69-72) and tests it against nothing, so the definition is this project's: both boxes are swept
 * at the constant velocity they have at the step -- the ego's v (cos yaw, sin yaw), a track's (vx, vy) --, rectangles that
 * translate keep their orientations, the four separating axes are constant in time and the first time of overlap is a closed
 * form (ttc_geom.h; no time sampling).  Conventions: boxes overlapping now: 0.0; boxes that only touch at an instant or
 * slide in contact are no hit (+inf), as are two point boxes; a time above `horizon` is reported as +inf.  Like the clearance
 * audit this call sits outside every planning cycle: synchronous on the context's stream, on the audits' scratch.
 *
 * Inputs exactly as mind_audit_episode takes them (ego rows (x, y, v, yaw); exo rows (x, y, heading, vx, vy), row 0 unused;
 * the same row caps); the ego's centre is (x, y) + center_offset (cos yaw, sin yaw).  Per (ego, step): step_ttc = the minimum
 * over the valid tracks 1..n_tracks-1 of the swept time, or +inf when that is above horizon (no valid track: +inf), and
 * step_track = the lowest track attaining it, -1 for +inf.  Per ego: ego_min with ego_step (the lowest step wins ties; 0 when
 * every step is +inf) and ego_track = that step's track, ego_hits = steps with ttc < bound (strict), ego_first = the first of
 * them (-1: none).  lanes picks the kernel's layout and changes no result: 0 = the library's rule (by n_ego x n_steps), 1 =
 * thread per ego, 2 = one wavefront per (step, ego), its lanes over the tracks.
 * Outputs HOST, each may be NULL (not all): step_* [n_ego, n_steps], ego_* [n_ego].
 * MIND_EINVAL as mind_audit_episode, and: horizon not finite or <= 0, bound not finite or < 0, lanes outside 0..2, a
 * non-finite v of an ego row or vx, vy of a valid track row.  n_ego == 0 or n_steps == 0 is a successful no-op.  MIND_ESTATE
 * as mind_audit_plan. */
typedef struct { double horizon, bound; int lanes; } mind_audit_ttc_cfg;
typedef struct {
  double *step_ttc; int32_t *step_track;
  double *ego_min; int32_t *ego_step, *ego_track, *ego_hits, *ego_first;
} mind_audit_ttc_out;
int mind_audit_ttc(mind_ctx *ctx, const mind_audit_box *ego, const mind_audit_ttc_cfg *cfg, int n_ego, int n_steps,
                   int n_tracks, const double *ego_states, const double *exo, const uint8_t *valid, const double *boxes,
                   const mind_audit_ttc_out *out);

/* ttc_geom.h on the CPU (host only, no context; no horizon): n pairs, a and b HOST [n, 7] = (x, y, yaw, L, W, vx, vy), offset
 * and relative velocity taken as b - a.  trig HOST [n, 4] = (cos a, sin a, cos b, sin b), or NULL = the kernels' own sin / cos
 * (mind_trig.h).  out HOST [n]: tg_rect_rect_ttc, +inf for never.  MIND_EINVAL for n < 0 or a NULL pointer. */
int mind_debug_box_ttc(int n, const double *a, const double *b, const double *trig, double *out);

/* ------------------------------------------------------------------------------------------------
 * Lane audit of plans and closed-loop episodes (mind_amd/csrc/lane_geom.h, lane_kernels.hip): whether the ego drove WHERE it
 * was told to drive -- how far from a lane centreline it got, whether it pointed along the traffic flow, how much arc length
 * it covered.  A planner that never leaves the drivable area and never hits anything can still crawl, cut across the oncoming
 * lane or park.  The reference projects one pose at a time on one polyline in Python (project_point_on_polyline,
 * get_closest_semantic_lane) and scores no trace with it, so the definitions are this project's.  Like the other audits these
 * calls sit outside every planning cycle: synchronous on the context's stream, on the audits' scratch.
 *
 * Lanes: verts HOST [V, 2] float64 world coordinates and lane_off HOST [n_lanes + 1], lane_off[0] = 0; lane l is the OPEN
 * polyline of the vertices lane_off[l] .. lane_off[l + 1] - 1, at least two, in the direction of travel.  Segment g (the
 * global index of its first vertex) joins vertex g to g + 1; a lane's last vertex and the next lane's first form none; a
 * duplicated vertex (a zero-length segment) is skipped.  The library forms the arc length at every vertex itself.
 * The reference point is the ego box's centre, (x, y) + center_offset (cos yaw, sin yaw).  Per box, twice -- index 0 over ALL
 * segments ("any"), index 1 over the segments whose direction e satisfies (cos yaw, sin yaw) . e >= cos_flow ("with the
 * flow") --: the nearest segment by squared clamped distance, the lowest g winning ties, and of it
 *   lat    = the distance, positive when the centre is left of the direction of travel, negative right of it;
 *   s      = the arc length of the projection from the lane's first vertex (0 before it, the lane's length beyond its end);
 *   along  = (cos yaw, sin yaw) . e, across = e x (cos yaw, sin yaw) (positive: the heading points left of the lane) -- the
 *            heading error is atan2(across, along), left to the caller;
 *   lane   = its lane, edge = its index within the lane.
 * No qualifying segment: lat = +inf, lane = edge = -1, s = along = across = NaN.  margin = bound - |lat with the flow|, the
 * audits' sign convention: a hit is margin < 0, exactly 0 is none, -inf when no segment goes the ego's way.  A state row holding
 * a non-finite value reports every double NaN, every index -1.
 * cfg: cos_flow in [-1, 1]; bound finite and > 0; form picks the kernel's shape and changes no result: 0 = the library's rule
 * (by rows), 1 = thread per box, 2 = one wavefront per box, its lanes over the segments.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { double cos_flow, bound; int form; } mind_audit_lane_cfg;

/* n_ego ego traces ego_states HOST [n_ego, n_steps, 4] = (x, y, v, yaw).  Per ego over step_margin, as mind_audit_road_episode
 * folds its margin: ego_min with ego_step and ego_lane = that step's with-flow lane (the lowest step wins ties), ego_hits =
 * steps with margin < 0, ego_first = the first of them (-1: none); a trace holding a NaN step: min = NaN, step = the first such
 * step, lane = -1, hits = -1, first = -1.  ego_progress / ego_back: sequentially from 0.0 over the steps k >= 1 whose "any"
 * lane equals step k - 1's and is >= 0, with d = s_any[k] - s_any[k - 1]: progress += d, and back += d when d < 0.
 * Outputs HOST, each may be NULL (not all).
 * MIND_EINVAL: a NULL required pointer, a negative count, n_lanes outside 1..2^16, lane_off not starting at 0 or not ascending
 * by at least 2, more than 2^20 vertices, a non-finite vertex, a non-finite or negative box dimension, cos_flow outside
 * [-1, 1], bound not finite or <= 0, form outside 0..2, all outputs NULL, n_ego x n_steps > 2^22.  n_ego == 0 or n_steps == 0
 * is a successful no-op.  MIND_ESTATE as mind_audit_plan. */
typedef struct {   /* per-step doubles / ints: [2, n_ego, n_steps], index 0 = any, 1 = with the flow */
  double *step_lat, *step_s, *step_along, *step_across; int32_t *step_lane, *step_edge;
  double *step_margin;                                                  /* [n_ego, n_steps] */
  double *ego_min; int32_t *ego_step, *ego_lane, *ego_hits, *ego_first; /* [n_ego], lowest step wins ties */
  double *ego_progress, *ego_back;                                      /* [n_ego] */
} mind_audit_lane_episode_out;
int mind_audit_lane_episode(mind_ctx *ctx, const mind_audit_box *ego, const mind_audit_lane_cfg *cfg, const double *verts,
                            const int32_t *lane_off, int n_lanes, int n_ego, int n_steps, const double *ego_states,
                            const mind_audit_lane_episode_out *out);

/* n_cand candidate state sets xs HOST [n_cand, sum M, 6] (as mind_audit_plan takes them) on the cost trees of a plan; n_nodes,
 * parent and prob of the trees are read.  Per (candidate, tree) over node_margin, as mind_audit_road_plan folds its margin:
 * tree_min, tree_node, tree_lane (that node's with-flow lane), tree_hits, tree_first, tree_mass.  tree_progress: sequentially
 * from 0.0 in key order over the nodes i with parent[i] >= 0 whose "any" lane equals the parent's and is >= 0,
 * progress += (double)prob[i] (s_any[i] - s_any[parent[i]]).
 * Outputs HOST, each may be NULL (not all).  MIND_EINVAL as above with n_cand x sum M > 2^20 in place of the episode's cap, and
 * a NULL parent or a parent index >= n_nodes.  n_cand == 0 is a successful no-op.  MIND_ESTATE as mind_audit_plan. */
typedef struct {   /* per-node doubles / ints: [2, n_cand, sum M], index 0 = any, 1 = with the flow */
  double *node_lat, *node_s, *node_along, *node_across; int32_t *node_lane, *node_edge;
  double *node_margin;                                                                          /* [n_cand, sum M] */
  double *tree_min; int32_t *tree_node, *tree_lane, *tree_hits, *tree_first; double *tree_mass; /* [n_cand, n_trees] */
  double *tree_progress;                                                                        /* [n_cand, n_trees] */
} mind_audit_lane_plan_out;
int mind_audit_lane_plan(mind_ctx *ctx, const mind_audit_box *ego, const mind_audit_lane_cfg *cfg, const double *verts,
                         const int32_t *lane_off, int n_lanes, const mind_cost_tree *trees, int n_trees, int n_cand,
                         const double *xs, const mind_audit_lane_plan_out *out);

/* lane_geom.h on the CPU (host only, no context): n boxes HOST [n, 3] = (x, y, yaw) of the box `ego` (only its center_offset
 * matters) against the lanes.  trig HOST [n, 2] = (cos yaw, sin yaw), or NULL = the kernels' own sin / cos (mind_trig.h).
 * Outputs HOST, each may be NULL (not all): lat, s, along, across, lane, edge [2, n] (0 = any, 1 = with the flow), margin [n].
 * MIND_EINVAL for n < 0, a NULL required pointer, a bad box, cfg or lanes (the rules above). */
int mind_debug_lane_project(int n, const double *boxes, const mind_audit_box *ego, const mind_audit_lane_cfg *cfg,
                            const double *verts, const int32_t *lane_off, int n_lanes, const double *trig, double *lat,
                            double *s, double *along, double *across, int32_t *lane, int32_t *edge, double *margin);

#ifdef __cplusplus
}
#endif
#endif /* MIND_HIP_H */
