// libmind_hip.so: C-ABI (include/mind_hip.h) over the hand-written gfx950 kernels.
// Host side: context, state_dict -> packed device blob, per-call job tables, kernel launches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <atomic>
#include <functional>
#include <vector>

#include "../../include/mind_hip.h"
#include "encdec_kernels.hip"
#include "fusion_kernels.hip"
#include "pair_bf16_kernels.hip"
#include "pair_tile_kernels.hip"
#include "pair_tile6_kernels.hip"
#include "token_mfma_kernels.hip"
#include "actor_mfma_kernels.hip"
#include "actor_lw_kernels.hip"
#include "token_lw_kernels.hip"
#include "actor_f32_kernels.hip"
#include "dec_mfma_kernels.hip"
#include "dec_curve_kernels.hip"
#include "ilqr_kernels.hip"
#include "ilqr_score_kernels.hip"
#include "ilqr_policy_kernels.hip"
#include "audit_kernels.hip"
#include "forecast_kernels.hip"
#include "road_kernels.hip"
#include "ttc_kernels.hip"
#include "lane_kernels.hip"
#include "pair_jobs.h"
#include "pred_choice.h"
#include "ilqr_choice.h"
#include "aime_book.h"
#include "audit_arena.h"
#include "weight_pack.h"
#include "aime_kernels.hip"

static_assert(TN_RA == RA && TN_IL_SLOTS == IL_SLOTS, "tuning.h restates the two kernel constants its clamps need");

// Owners of the context's HIP handles: each releases what it holds in its destructor and is move-only, so a context (or a vector of them)
// gives everything back when it goes, whichever path it goes by.  p is the raw handle (an owner also converts to it, where a HIP call or a
// kernel argument wants one), cap the bytes behind it for the two kinds that are memory.  live_handles counts acquisitions less releases
// over the process (mind_debug_live_handles): what a leak test can read on a shared device.
static std::atomic<long> live_handles{0};

template <class H, hipError_t (*Release)(H)> struct Owned {
  H p = nullptr;
  size_t cap = 0;
  Owned() = default;
  Owned(Owned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~Owned() { reset(); }
  operator H() const { return p; }
  template <class T> T *as() const { return (T *)p; }
  void reset() {
    if (p) { (void)Release(p); live_handles.fetch_sub(1, std::memory_order_relaxed); }
    p = nullptr; cap = 0;
  }
  hipError_t took(hipError_t e, size_t bytes = 0) {      // the result of the HIP call that just filled p (after a reset)
    if (e == hipSuccess) { live_handles.fetch_add(1, std::memory_order_relaxed); cap = bytes; } else p = nullptr;
    return e;
  }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> { hipError_t create(unsigned flags = hipEventDefault) { reset(); return took(hipEventCreateWithFlags(&p, flags)); } };
struct Stream : Owned<hipStream_t, hipStreamDestroy> { hipError_t create() { reset(); return took(hipStreamCreateWithFlags(&p, hipStreamNonBlocking)); } };
struct Pinned : Owned<void *, hipHostFree> {      // page-locked host memory
  hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) { reset(); return took(hipHostMalloc(&p, bytes, flags), bytes); }
};
struct DevBuf : Owned<void *, hipFree> {          // device memory (ensure / ensure_exact below keep their growth policy over alloc)
  hipError_t alloc(size_t bytes) { reset(); return took(hipMalloc(&p, bytes), bytes); }
};

// job / token tables of one batch shape (scene sizes), resident on the device
struct TableSet {
  std::vector<int> key;               // Bn, actor_off[0..Bn], lane_off[0..Bn]
  DevBuf meta, jobs, jobs5, rows;      // jobs5: the columns the last fusion layer runs (actors + cls), for k_pair_t
  std::vector<int> actor_row, cls_row, scene_n;
  long long edge_pairs = 0, edge_pairs_t = 0, stamp = 0;     // edge_pairs_t: with every column padded to whole 16-row tiles
  int ntok = 0, slot = 0, njobs = 0, njobs5 = 0;
  double pairs_full = 0, pairs_l5 = 0;
};
#define MIND_TABLE_SETS 8

struct mind_ctx {
  int device = 0;
  hipStream_t stream = nullptr;       // the caller's
  // internal side stream: the lane encoders run beside the actor encoder; always fenced against `stream` with
  // events on both sides, so callers only ever see work ordered on `stream`
  Stream side;
  Event ev_side, ev_main, ev_stage, ev_tgt, ev_cls;
  std::vector<char> aime_stage;   // host staging of mind_aime_world's small tables (guarded by ev_stage)
  bool aime_stage_busy = false;
  std::string err;
  // weights: the packed device blob and the kernels' pointer tables into it (weight_pack.h, weight_tables.h); valid while have_weights
  DevBuf wdev;
  bool have_weights = false;
  WeightTables W = {};
  // the knobs (tuning.h): the predictor's kernel selection, the tree-iLQR solver's launch, the context's own
  PredTuning pt; IlqrTuning it; CtxTuning ct;
  TnRefs knobs() { return {&pt, &it, &ct}; }
  // the decoder's curve basis (mind_set_decoder_basis): which tables the blob entries dec.T / dec.Tp hold and which vel formula the heads run;
  // survives mind_weights_load.  mind_curve_eval's basis rows on the device, and the (basis, tau) they were evaluated for
  int dec_basis = MIND_BASIS_BEZIER;
  DevBuf curve_tab;
  std::vector<double> curve_tau;
  int curve_tab_basis = -1;
  // layer-wise token stage (token_lw_kernels.hip): its scratch arena holds one chunk and is allocated at first use
  DevBuf tok_lw_arena;
  std::vector<TlLaunch> tok_lw_plan;
  // the token stage of the last mind_predict_batch (mind_last_token_stats): launches of all seven token steps, time per layer-wise stage
  // ([TL_NSTAGE]: the one-kernel forms) from HIP events around every launch with profiling on
  int last_tok_lw = 0, last_tok_launches = 0, last_tok_chunks = 0;
  float tok_ms = 0.f, tok_stage_ms[TL_NSTAGE + 1] = {};
  std::vector<Event> ev_tok;
  std::vector<int> ev_tok_tag;
  // job / token tables of recent mind_predict_batch calls (least-recently-used of MIND_TABLE_SETS): a call whose scene sizes
  // were seen before rebuilds, uploads and synchronises nothing -- the closed loop's rounds recur every cycle, a full tree's
  // rounds (1 / 6 / 36 / 216 scenes) every plan
  TableSet tabs[MIND_TABLE_SETS];
  long long tab_clock = 0;
  long long n_table_hits = 0;
  // mind_aime_plan's polled decisions ("dec_poll"): the generation the host waits for, the counter k_aime_select_branch's blocks count in on
  unsigned dec_gen = 0;
  DevBuf pl_cnt;
  // what a round hands to its first predictor call ("root_head" / "round_head"), which launches ActorNet first: enc_pre goes on the side stream
  // in front of the lane encoders, enc_post behind the target embedding (pred_encoders; both are the plan's, cleared when it returns)
  std::function<int(hipStream_t)> enc_pre, enc_post;
  // host side of a tree-iLQR call (ilqr_host.hip), kept between calls so that a planning cycle does not allocate a hundred small vectors: the
  // trees' index tables and the image of the arena's uploaded doubles / floats / ints
  std::vector<IlTables> il_tab;
  struct IlImage { std::vector<double> hD; std::vector<float> hF; std::vector<int> hI; } il_img;
  // the pending tree-iLQR launch writes its results to the host itself and marks every tree when it is complete (IlqrChoice::early): where, and
  // the word's value that means "complete" for THIS launch.  Valid between the launch and its mind_ilqr_finish.
  struct IlEarly { const double *xs = nullptr, *us = nullptr; volatile unsigned *done = nullptr; unsigned gen = 0; int n_trees = 0; long nodes = 0; } il_early;
  unsigned il_gen = 0;
  long long il_spec_req = 0, il_spec_hit = 0;       // last launch, all trees and fits: passes the speculator was asked in / results the master took
  // layer-wise batched ActorNet (actor_lw_kernels.hip): its scratch arena (one chunk, allocated at first use)
  DevBuf actor_lw_arena;
  std::vector<LwLaunch> actor_lw_plan;
  // the ActorNet of the last mind_predict_batch (mind_last_actor_stats)
  int last_actor_lw = 0, last_actor_launches = 0, last_actor_chunks = 0;
  float actor_ms = 0.f;
  Event ev_act0, ev_act1;
  int pair_prec = 3;            // arithmetic of the pair kernel: 0 = fp32 MFMA, 1 = bf16x3 (two-way split operands), 2 = bf16, 3 = bf16x6 (exact three-way split: fp32 class, default)
  std::vector<int> last_scene_n;   // tokens per scene of the last predictor call (mind_debug_read("edge") un-permutes with it)
  bool last_edge_tiled = false, last_edge_bf16 = false;
  // workspaces (grow only)
  DevBuf edge, x, ST, QK, part, tokpos, meta, jobs, actor_feat, lane_feat, tgt_feat, cmode, tgt_emb,
      rows, rpe_ptrs;
  // ilqr workspaces
  DevBuf ilqr_dev, aime_dev, rebase_dev2[2], dec_h2;
  // scratch of the two clearance audits, the two road audits, the two lane audits, mind_forecast_score and mind_audit_ttc (ar_begin, audit_host.hip).  One buffer serves all eight:
  // each is synchronous on the context's stream and refuses a busy context, so a call never sees another call's scratch in flight -- and
  // each uploads every input its kernels read, so none relies on what an earlier call left
  DevBuf audit_dev;
  // mind_aime_plan (aime_plan.hip): device arenas, page-locked staging (uploads / read-backs are true async copies: a pageable
  // source makes hipMemcpyAsync wait for the stream to drain first), host result tables
  DevBuf pl_root, pl_in[2], pl_lf, pl_lrep, pl_pred, pl_small, pl_tab[2], pl_win[2];
  std::vector<DevBuf> pl_world;
  Pinned pl_pin[8];     // [4], [5]: upload / read-back staging of the tree-iLQR calls; [6], [7]: sharded plan
  Event ev_pl, ev_tab, ev_root;
  // the lane-distance field of a plan's contingency solves (gen_dist_field: a function of the ego position, the grid and the target lane --
  // all known when the plan starts), computed on the side stream beside the plan's first round instead of between its last decisions and
  // k_ilqr (il_field_prepare; adopted by il_solve when grid and lane are the ones it was made for)
  DevBuf il_field;
  Pinned il_field_pin;
  Event ev_field;
  bool il_field_valid = false;
  double il_field_key[5] = {0, 0, 0, 0, 0};       // x0[0], x0[1], W, H, res
  std::vector<double> il_field_lane;
  // mind_set_exchange: the sharded mind_aime_plan (rank, world, the caller's transport, packing buffers, collectives of the last plan)
  int xr = 0, xw = 1;
  mind_exchange_fn xfn = nullptr;
  void *xuser = nullptr;
  bool xforce = false;
  DevBuf x_send, x_recv, x_seg;
  long long x_collectives = 0, x_bytes = 0;
  Stream pl_copy;       // the plan's own copy stream ("pl_tab_side": the round tables; the rows' read-back)
  std::vector<double> pl_sol_xs, pl_sol_us;          // results of the solves a plan began itself (mind_ilqr_finish_plan)
  std::vector<mind_ilqr_stats> pl_sol_stw, pl_sol_stf;
  // mind_aime_plan_begin / _finish: the plan on a thread of the library (state 0 idle, 1 running, 2 done)
  std::thread pa_thread;
  std::atomic<int> pa_state{0};
  mind_aime_plan_in pa_in;
  mind_aime_plan_out pa_out;
  int pa_rc = 0;
  // the context's last plan: its bookkeeping and host result tables (aime_book.h: node table, tree_top / tree_off / flat_parent / flat_prob) and
  // where its rows and flattened cost trees lie
  struct Plan {
    AimeBook book;
    int agents = 0;             // agents per scene of the plan those tables belong to
    long long gen = 0;          // plans begun on this context so far: whoever holds a plan's library-owned tables (mind_loop) checks they are still that plan's
    const float *rows_p = nullptr, *fmean_p = nullptr, *fcov_p = nullptr;      // into page-locked slot 2, valid until the next plan
    // the cost trees' agent means / sigmas where k_aime_flat wrote them (device): a tree-iLQR call on the plan's own trees
    // (mind_ilqr_contingency_begin_plan) reads them there instead of taking them through the host
    const float *dev_fmean = nullptr, *dev_fcov = nullptr;
  } plan;
  DevBuf pl_flat;
  DevBuf dec_xbuf, dec_bars;
  DevBuf dec_chain;      // what the kernels of the scene part's launch chain hand to each other (dec_chain.h: DC_SCENE_FLOATS per scene)
  Pinned dec_abort;      // host-visible abort word of its barriers (page-locked, mapped)
  int rb_cur = 0, rb_gen = 0;     // re-basing arenas: which one the last call filled, its generation and geometry
  size_t rb_S = 0, rb_a = 0;
  // profiling
  bool profiling = false;
  Event ev_il0, ev_il1;   // around the tree-iLQR launch of the last call (profiling on)
  float ilqr_ms = 0.f;
  int ilqr_multi = 0, ilqr_trees = 0;
  // per-iteration traces of the last tree-iLQR call (mind_last_ilqr_trace): device address per tree, rows per phase, iterations run
  std::function<int()> il_finish;     // the pending half of a call begun with mind_ilqr_contingency_begin
  bool il_finish_owned = false;       // ... whose outputs are library buffers (the solves a plan began itself): may be drained and dropped
  Event ev_rows;
  std::vector<const double *> il_trace_dev;
  std::vector<int> il_trace_its;      // [tree][phase 2]
  int il_trace_cap = 0, il_trace_phases = 0;
  double il_prof[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // critical tree of the last launch: M, depth, passes, cycles of the five phases, trees
  long long n_ilqr_fallbacks = 0;   // wide-tree launches that were not fully resident and were re-run on one workgroup per tree
  int n_pair_launch = 0;
  float pair_ms = 0.f;
  double pairs_done = 0.0;
  std::vector<Event> ev;
  // mind_aime_plan with profiling on: the pair-kernel events of its predictor calls are taken from this pool and read once, behind the
  // plan's last synchronisation (a stream drain per predictor call to read twelve events cost ~30 us per round of the timed plan)
  bool ev_defer = false;
  std::vector<Event> ev_pool;
  size_t ev_pool_used = 0;
  std::vector<size_t> ev_pending;      // first pool index of every predictor call not read yet
  // the launch clock ("prof_clock"; launch_clock.h, predict.hip): the ring on the device, its page-locked mirror, the wall clock's rate (0: no
  // such clock -- events), sums of records read early, the per-launch times of the last read
  int wall_khz = 0;
  LcRing lc;
  DevBuf lc_dev;
  Pinned lc_host;
  double lc_carry_ms[LC_KINDS] = {0, 0, 0};
  int lc_carry_n[LC_KINDS] = {0, 0, 0};
  std::vector<float> lc_last[LC_KINDS], ev_last[LC_KINDS];
  int n_cu = 256;
  int debug_layers = 6;
  int debug_tok_form = 0;          // mind_debug_token_form: 0 the rule, else the kernel of the small, merged token launches
  int last_ntok = 0;
  size_t il_dbg[6] = {0, 0, 0, 0, 0, 0};   // tree 0 of the last iLQR call: byte offsets of L, Lx, Lxx, Fx, xs in ilqr_dev; M
  long long last_edge_pairs = 0;
  int last_slots = 0, last_A = 0, last_B = 0;
};

static int fail(mind_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(c, call)                                                                        \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(c, MIND_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

static int ensure(mind_ctx *c, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return MIND_OK;
  b.reset();
  // growth: a buffer is re-allocated (hipFree + hipMalloc: a device synchronisation each) whenever a plan needs more than any before it --
  // small buffers (demo-size scenes: the scene and tree-node counts of the first dozens of plans of a process creep upwards) double and start
  // at 1 MB, so that a closed loop stops re-allocating after its first plans (a fresh process ran its first 20 timed cycles at 2.1-2.6 ms of
  // AIME wall instead of 1.8, profiles/r05w_*); big arenas (the deep stress trees: hundreds of GB) keep the 25 % margin
  const size_t want = bytes < ((size_t)64 << 20) ? std::max<size_t>(2 * bytes, (size_t)1 << 20) : bytes + bytes / 4 + 4096;
  if (b.alloc(want) != hipSuccess) {
    const hipError_t e = b.alloc(bytes);
    if (e != hipSuccess) return fail(c, MIND_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  return MIND_OK;
}

// a scratch arena of exactly `bytes` (no growth margin: tens of MB to GB, sized by a knob), re-allocated behind a drained stream
static int ensure_exact(mind_ctx *c, DevBuf &b, size_t bytes, const char *what) {
  if (bytes <= b.cap) return MIND_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (b.alloc(bytes) != hipSuccess) return fail(c, MIND_ENOMEM, "hipMalloc(%zu) for %s failed", bytes, what);
  return MIND_OK;
}

// Every kernel that takes more dynamic LDS than the default limit, and how much.  The attribute is per device: set for every created context.
struct KernelLds {
  const void *kernel; size_t bytes;
  template <class K> KernelLds(K *k, size_t b) : kernel((const void *)k), bytes(b) {}
};
static void set_kernel_attributes() {
  const size_t pair = mind_pair_lds_bytes(), pair_bf = mind_pair_bf_lds_bytes(), actor_m = mind_actor_mfma_lds_bytes(), dec_m = mind_dec_actor_mfma_lds_bytes(),
               il = il_lds_bytes(0), tok_m = mind_token_mfma_lds_bytes(), dec_s = mind_dec_scene_lds_bytes(), dec_a = mind_dec_actor_lds_bytes();
  const KernelLds lds[] = {
      {k_pair<0>, pair}, {k_pair<1>, pair}, {k_pair_bf<0, 3>, pair_bf}, {k_pair_bf<1, 3>, pair_bf}, {k_pair_bf<0, 1>, pair_bf}, {k_pair_bf<1, 1>, pair_bf},
      {k_pair_t<0, 3>, pair_bf}, {k_pair_t<1, 3>, pair_bf}, {k_pair_t<0, 1>, pair_bf}, {k_pair_t<1, 1>, pair_bf}, {k_pair_t6<0>, pair_bf}, {k_pair_t6<1>, pair_bf},
      {k_actor_net, mind_actor_lds_bytes()}, {k_actor_mfma<3>, actor_m}, {k_actor_mfma<6>, actor_m}, {k_actor_mfma<1>, actor_m},
      {k_dec_actor_mfma<1>, dec_m}, {k_dec_actor_mfma<3>, dec_m}, {k_dec_actor_mfma<6>, dec_m}, {k_actor_f32<1>, mind_actor_f32_lds_bytes(1)}, {k_actor_f32<2>, mind_actor_f32_lds_bytes(2)},
      {k_ilqr<true, 0>, il}, {k_ilqr<false, 1>, il}, {k_ilqr<false, 0>, il}, {k_ilqr<false, 2>, il}, {k_token_mfma<0>, tok_m}, {k_token_mfma<1>, tok_m},
      {k_dec_scene, dec_s}, {k_dec_scene_mw, dec_s}, {k_dec_scene_c, dec_s}, {k_dec_cls, dec_s}, {k_dec_tgt, dec_s},
      {k_dec_chain1<8>, dec_s}, {k_dec_chain2<8>, dec_s}, {k_dec_chain3<8>, dec_s}, {k_dec_chain1<16>, dec_s}, {k_dec_chain2<16>, dec_s}, {k_dec_chain3<16>, dec_s},
      {k_dec_chain1<32>, dec_s}, {k_dec_chain2<32>, dec_s}, {k_dec_chain3<32>, dec_s}, {k_dec_chain4, dec_s},
      {k_dec_actor<0>, dec_a}, {k_dec_actor<1>, dec_a}, {k_dec_actor<2>, dec_a}, {k_dec_actor<2, 1>, dec_a}, {k_dec_actor<2, 2>, dec_a},
  };
  for (const KernelLds &k : lds) (void)hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes);
  lw_set_attributes();
}

static const char *const PAIR_PREC_NAMES[4] = {"f32", "bf16x3", "bf16", "bf16x6"};      // MIND_PAIR_PREC: a name or its number

extern "C" int mind_ctx_create(int device, void *stream, mind_ctx **out) {
  if (!out) return MIND_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MIND_EHIP;
  if (device < 0 || device >= n) return MIND_EINVAL;
  std::unique_ptr<mind_ctx> c(new mind_ctx());      // (an early return gives back whatever the context holds by then)
  c->device = device;
  if (hipSetDevice(device) != hipSuccess) return MIND_EHIP;
  // NULL = the device's default (null) stream, which is what torch.cuda.current_stream() is unless the
  // caller switched streams; everything the caller can observe is ordered on this stream.
  c->stream = (hipStream_t)stream;
  // the side stream and the three events that fence it: all of them, or no side stream
  if (c->side.create() != hipSuccess || c->ev_side.create(hipEventDisableTiming) != hipSuccess || c->ev_main.create(hipEventDisableTiming) != hipSuccess ||
      c->ev_tgt.create(hipEventDisableTiming) != hipSuccess)
    c->side.reset();
  if (c->ev_stage.create(hipEventDisableTiming) != hipSuccess) return MIND_EHIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
  if (hipDeviceGetAttribute(&c->wall_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || c->wall_khz < 0) c->wall_khz = 0;
  set_kernel_attributes();
  tn_apply_env(c->knobs(), [](const char *name) -> const char * { return getenv(name); });
  if (const char *pe = getenv("MIND_PAIR_PREC"))      // (read by name, not as an int: no row of the table)
    for (int m = 0; m < 4; ++m)
      if (!strcmp(pe, PAIR_PREC_NAMES[m]) || (pe[0] == '0' + m && !pe[1])) (void)mind_set_pair_precision(c.get(), m);
  *out = c.release();
  return MIND_OK;
}

extern "C" int mind_ctx_destroy(mind_ctx *c) {
  if (!c) return MIND_EINVAL;
  if (c->pa_thread.joinable()) c->pa_thread.join();
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);      // nothing is freed before everything queued has run
  if (c->side) (void)hipStreamSynchronize(c->side);
  if (c->pl_copy) (void)hipStreamSynchronize(c->pl_copy);
  c->il_finish = nullptr;     // a begun and never collected tree-iLQR call: drained above, dropped here
  delete c;
  return MIND_OK;
}

extern "C" const char *mind_last_error_string(mind_ctx *c) { return c ? c->err.c_str() : "null context"; }

extern "C" int mind_ctx_synchronize(mind_ctx *c) {
  if (!c) return MIND_EINVAL;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MIND_OK;
}

extern "C" int mind_set_tuning(mind_ctx *c, const char *name, int value) {
  if (!c || !name) return MIND_EINVAL;
  if (!tn_set(c->knobs(), name, value)) return fail(c, MIND_EINVAL, "mind_set_tuning: unknown knob '%s'", name);
  return MIND_OK;
}

extern "C" int mind_get_tuning(mind_ctx *c, const char *name, int *value) {
  if (!c || !name || !value) return MIND_EINVAL;
  if (!tn_get(c->knobs(), name, value)) return fail(c, MIND_EINVAL, "mind_get_tuning: unknown knob '%s'", name);
  return MIND_OK;
}

// the knob table without a context (layout: include/mind_hip.h)
extern "C" int mind_debug_tuning(int index, const char *name, const char *text, int value, const char **out_name, const char **out_env, int *out_value) {
  PredTuning pt; IlqrTuning it; CtxTuning ct;
  const TnRefs fresh{&pt, &it, &ct};
  const TnRow *row = name ? tn_find(name) : (index >= 0 && index < TN_ROWS) ? &TN_TABLE[index] : nullptr;
  if (!row || !out_value || (name && text && !row->env)) return MIND_EINVAL;
  if (name && text) tn_apply_env(fresh, [&](const char *var) { return strcmp(var, row->env) ? nullptr : text; });
  else if (name) (void)tn_set(fresh, name, value);
  if (out_name) *out_name = row->name;
  if (out_env) *out_env = row->env;      // (null: no variable)
  (void)tn_get(fresh, row->name, out_value);
  return name ? MIND_OK : TN_ROWS;
}

extern "C" int mind_debug_live_handles(void) { return (int)live_handles.load(std::memory_order_relaxed); }

extern "C" int mind_set_exchange(mind_ctx *c, int rank, int world, mind_exchange_fn fn, void *user, int force) {
  if (!c) return MIND_EINVAL;
  if (fn && (world < 1 || rank < 0 || rank >= world)) return fail(c, MIND_EINVAL, "mind_set_exchange: rank %d of %d", rank, world);
  c->xfn = fn; c->xuser = user;
  c->xr = fn ? rank : 0; c->xw = fn ? world : 1; c->xforce = fn && force != 0;
  return MIND_OK;
}

extern "C" int mind_last_exchange_stats(mind_ctx *c, long long *collectives, long long *bytes) {
  if (!c) return MIND_EINVAL;
  if (collectives) *collectives = c->x_collectives;
  if (bytes) *bytes = c->x_bytes;
  return MIND_OK;
}

extern "C" int mind_set_pair_precision(mind_ctx *c, int mode) {
  if (!c || mode < 0 || mode > 3) return MIND_EINVAL;
  c->pair_prec = mode;
  return MIND_OK;
}

extern "C" int mind_get_pair_precision(mind_ctx *c) { return c ? c->pair_prec : MIND_EINVAL; }

extern "C" int mind_debug_pack_bfrag(const float *w, int row_stride, uint32_t *out) {
  if (!w || !out || row_stride < 128) return MIND_EINVAL;
  std::vector<float> v(w, w + (size_t)127 * row_stride + 128);
  v.resize((size_t)128 * row_stride, 0.f);
  const std::vector<float> t = pack_bfrag(v, row_stride);
  memcpy(out, t.data(), 16384 * sizeof(uint32_t));
  return MIND_OK;
}

static int lc_reserve(mind_ctx *c, int records, int grid);      // (predict.hip)
extern "C" int mind_set_profiling(mind_ctx *c, int enable) {
  if (!c) return MIND_EINVAL;
  c->profiling = enable != 0;
  // the launch clock's ring and its page-locked mirror are allocated here, outside anything timed: two predictor calls of pair launches on
  // every CU (a call with larger grids or more records grows it in front of its launches)
  if (c->profiling && c->ct.prof_clock != 0 && c->wall_khz > 0 && c->lc.n_blocks == 0) {
    HIPCHK(c, hipSetDevice(c->device));
    return lc_reserve(c, 12, c->n_cu);
  }
  return MIND_OK;
}

extern "C" int mind_last_ilqr_stats(mind_ctx *c, float *kernel_ms, int *n_trees, int *workgroups_per_tree) {
  if (!c) return MIND_EINVAL;
  if (kernel_ms) *kernel_ms = c->ilqr_ms;
  if (n_trees) *n_trees = c->ilqr_trees;
  if (workgroups_per_tree) *workgroups_per_tree = c->ilqr_multi;
  return MIND_OK;
}

extern "C" int mind_last_ilqr_trace(mind_ctx *c, int tree, int phase, double *out, int cap_rows, int *n_rows) {
  if (!c || !n_rows || (cap_rows > 0 && !out)) return MIND_EINVAL;
  if (tree < 0 || tree >= (int)c->il_trace_dev.size() || phase < 0 || phase >= c->il_trace_phases || !c->il_trace_dev[tree])
    return fail(c, MIND_ESTATE, "mind_last_ilqr_trace: no trace for tree %d phase %d (the last tree-iLQR call had %d trees, %d phases)", tree, phase,
                (int)c->il_trace_dev.size(), c->il_trace_phases);
  const int rows = std::min(c->il_trace_its[2 * tree + phase], c->il_trace_cap);
  *n_rows = rows;
  const int take = std::min(rows, cap_rows);
  if (take > 0) {
    HIPCHK(c, hipMemcpyAsync(out, c->il_trace_dev[tree] + (size_t)phase * c->il_trace_cap * IL_TRACE_W, (size_t)take * IL_TRACE_W * sizeof(double),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return MIND_OK;
}

extern "C" int mind_last_ilqr_profile(mind_ctx *c, double *out9) {
  if (!c || !out9) return MIND_EINVAL;
  memcpy(out9, c->il_prof, sizeof(c->il_prof));
  return MIND_OK;
}

// deferred pair-kernel events of a plan (ev_defer): summed once the stream has been drained
static int mind_pair_events_resolve(mind_ctx *c, float *total_ms) {
  float sum = 0.f;
  c->ev_last[LC_PAIR].clear(); c->lc_last[LC_PAIR].clear();
  for (size_t base : c->ev_pending)
    for (int L = 0; L < c->debug_layers; ++L) {
      float ms = 0.f;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[base + 2 * L], c->ev_pool[base + 2 * L + 1]));
      sum += ms;
      c->ev_last[LC_PAIR].push_back(ms);
    }
  c->ev_pending.clear();
  c->ev_pool_used = 0;
  *total_ms = sum;
  return MIND_OK;
}

extern "C" int mind_last_fusion_stats(mind_ctx *c, int *n_launches, float *total_ms, double *pairs) {
  if (!c) return MIND_EINVAL;
  if (n_launches) *n_launches = c->n_pair_launch;
  if (total_ms) *total_ms = c->pair_ms;
  if (pairs) *pairs = c->pairs_done;
  return MIND_OK;
}

extern "C" int mind_debug_launch_times(mind_ctx *c, int kind, float *clock_ms, float *event_ms, int cap, int *n_clock, int *n_event) {
  if (!c || kind < 0 || kind >= LC_KINDS || cap < 0) return MIND_EINVAL;
  const std::vector<float> &lc = c->lc_last[kind], &ev = c->ev_last[kind];
  for (int i = 0; clock_ms && i < cap && i < (int)lc.size(); ++i) clock_ms[i] = lc[i];
  for (int i = 0; event_ms && i < cap && i < (int)ev.size(); ++i) event_ms[i] = ev[i];
  if (n_clock) *n_clock = (int)lc.size();
  if (n_event) *n_event = (int)ev.size();
  return MIND_OK;
}

extern "C" int mind_debug_launch_clock(int n_blocks, int block_slots, int rate_khz, const long long *ops, int n_ops, const unsigned long long *stamps,
                                       long long n_slots, double *out, int cap) {
  if (n_blocks < 0 || block_slots < 0 || n_ops < 0 || (n_ops > 0 && (!ops || !out)) || cap < 8 * n_ops || n_slots < 0 || (n_slots > 0 && !stamps))
    return MIND_EINVAL;
  LcRing R;
  R.reset(n_blocks, block_slots);
  for (int k = 0; k < n_ops; ++k) {
    const long long op = ops[4 * k], a = ops[4 * k + 1], b = ops[4 * k + 2];
    double *o = out + 8 * k;
    for (int i = 0; i < 8; ++i) o[i] = 0.0;
    if (a < -(1LL << 30) || a > (1LL << 30) || b < -(1LL << 30) || b > (1LL << 30)) return MIND_EINVAL;
    switch (op) {
    case 0: o[0] = R.take((int)a, (int)b); break;
    case 1: {
      int first[2] = {0, 0}, count[2] = {0, 0};
      o[0] = R.pending_runs((int)a, (int)b, first, count);
      o[1] = first[0]; o[2] = count[0]; o[3] = first[1]; o[4] = count[1];
      break;
    }
    case 2: R.drained((int)a); break;
    case 3: o[0] = R.fits((int)a, (int)b) ? 1 : 0; break;
    case 4: {
      int blocks, slots;
      R.grown((int)a, (int)b, blocks, slots);
      R.reset(blocks, slots);
      o[0] = blocks; o[1] = slots;
      break;
    }
    case 5: {
      if (a < 0 || b < 0 || a >= R.n_blocks || (long long)R.slot_of((int)a) + b > n_slots) return MIND_EINVAL;
      const unsigned long long t = lc_reduce((const LcSlot *)stamps + R.slot_of((int)a), (int)b);
      o[0] = (double)t; o[1] = lc_ticks_ms(t, rate_khz);
      break;
    }
    case 6: R.mark_copied((int)a, (int)b); break;
    case 7: o[0] = R.copied((int)a) ? 1 : 0; break;
    default: return MIND_EINVAL;
    }
    o[5] = (double)R.pending.size(); o[6] = R.head; o[7] = (double)R.dropped;
  }
  return 8 * n_ops;
}

extern "C" int mind_last_actor_stats(mind_ctx *c, int *layerwise, int *n_launches, int *n_chunks, float *total_ms) {
  if (!c) return MIND_EINVAL;
  if (layerwise) *layerwise = c->last_actor_lw;
  if (n_launches) *n_launches = c->last_actor_launches;
  if (n_chunks) *n_chunks = c->last_actor_chunks;
  if (total_ms) *total_ms = c->actor_ms;
  return MIND_OK;
}

extern "C" int mind_last_token_stats(mind_ctx *c, int *layerwise, int *n_launches, int *n_chunks, float *total_ms) {
  if (!c) return MIND_EINVAL;
  if (layerwise) *layerwise = c->last_tok_lw;
  if (n_launches) *n_launches = c->last_tok_launches;
  if (n_chunks) *n_chunks = c->last_tok_chunks;
  if (total_ms) *total_ms = c->tok_ms;
  return MIND_OK;
}

extern "C" int mind_last_token_stage_ms(mind_ctx *c, float *out_ms, int cap) {
  if (!c || cap < 0 || (cap > 0 && !out_ms)) return MIND_EINVAL;
  for (int i = 0; i < cap && i <= TL_NSTAGE; ++i) out_ms[i] = c->tok_stage_ms[i];
  return TL_NSTAGE + 1;
}

// the layer-wise token stage's launch list for one token launch of `mode` over a run of n_tokens tokens (tl_build_plan, token_lw_kernels.hip)
extern "C" int mind_debug_token_lw_plan(int n_tokens, int mode, int chunk, long long *out_launches, int cap, long long *out_info) {
  if (n_tokens <= 0 || chunk < 0 || !tl_mode_ok(mode) || (cap > 0 && !out_launches) || cap < 0) return MIND_EINVAL;
  if (chunk == 0) chunk = TL_CHUNK;
  std::vector<TlLaunch> plan;
  tl_build_plan(n_tokens, mode, chunk, TL_NCU_PLAN, plan);
  for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) {
    const TlLaunch &L = plan[i];
    long long *o = out_launches + 8 * i;
    o[0] = L.stage; o[1] = L.gx; o[2] = L.gy; o[3] = L.block; o[4] = L.lds; o[5] = L.t0; o[6] = L.n; o[7] = (L.n + TM_TOK - 1) / TM_TOK;
  }
  if (out_info) {
    out_info[0] = chunk; out_info[1] = (long long)tl_arena_bytes(chunk); out_info[2] = (long long)plan.size();
    out_info[3] = (n_tokens + chunk - 1) / chunk;
  }
  return (int)plan.size();
}

// the layer-wise ActorNet's launch list as mind_predict_batch issues it (lw_build_plan, actor_lw_kernels.hip), for a host-side check
extern "C" int mind_debug_actor_lw_plan(int n_actors, int np, int chunk, long long *out_launches, int cap, long long *out_info) {
  if (n_actors <= 0 || chunk < 0 || (np != 1 && np != 3 && np != 6) || (cap > 0 && !out_launches) || cap < 0) return MIND_EINVAL;
  if (chunk == 0) chunk = LW_CHUNK;
  std::vector<LwLaunch> plan;
  lw_build_plan(n_actors, chunk, plan);
  LwStage S[LW_NSTAGE];
  lw_stages(S);
  const int nparts = np == 6 ? 3 : (np == 3 ? 2 : 1);
  for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) {
    const LwLaunch &L = plan[i];
    long long *o = out_launches + 16 * i;
    o[0] = L.stage; o[1] = L.kind; o[2] = L.gx; o[3] = L.gy; o[4] = L.block; o[5] = L.lds; o[6] = L.a0; o[7] = L.n;
    for (int k = 8; k < 16; ++k) o[k] = 0;
    if (L.stage >= 0) {
      const LwStage &st = S[L.stage];
      o[8] = st.cin; o[9] = st.cout; o[10] = st.ksz; o[11] = st.stride; o[12] = st.tin; o[13] = st.tout;
      // fragment bytes the conv workgroup keeps stationary (the parts the arithmetic reads), and whether the stage ends in the output row
      o[14] = L.kind == 1 ? (long long)L.lds / 3 * nparts : 0; o[15] = st.final;
    }
  }
  if (out_info) { out_info[0] = chunk; out_info[1] = (long long)lw_arena_bytes(chunk); out_info[2] = (long long)plan.size(); }
  return (int)plan.size();
}

// -------------------------------------------------------------------------------------------------
// weight packing
// -------------------------------------------------------------------------------------------------
extern "C" int mind_debug_pack_conv_frag(const float *w, int co, int ci, int ksz, uint32_t *out, size_t cap) {
  if (!w || !out || co <= 0 || co % 16 || ci <= 0 || ksz <= 0) return MIND_EINVAL;
  const std::vector<float> t = pack_conv_frag(w, co, ci, ksz);
  if (t.size() > cap) return MIND_EINVAL;
  memcpy(out, t.data(), t.size() * sizeof(float));
  return (int)t.size();
}

// the other packers of weight_pack.h, by name
extern "C" int mind_debug_pack(const char *what, const float *w, int a, int b, int c, float *out, size_t cap) {
  if (!what || !w || !out) return MIND_EINVAL;
  const std::string k = what;
  std::vector<float> t;
  if (k == "afrag" && a >= 128) t = pack_afrag(w, a);
  else if (k == "wk_frag") t = pack_wk_frag(w);
  else if (k == "tok_bfrag" && a >= 128) t = pack_tok_bfrag(w, a);
  else if (k == "bfrag_lo3" && a >= 128) {
    std::vector<float> v(w, w + (size_t)127 * a + 128);
    v.resize((size_t)128 * a, 0.f);
    t = pack_bfrag_lo3(v, a);
  } else if (k == "conv_f32" && a > 0 && a % 16 == 0 && b > 0 && c > 0) t = pack_conv_f32(w, a, b, c);
  else if (k == "center_outputs" && a > 0 && b > 0) {      // w, out: W [a][b], then the bias [a]
    std::vector<float> bias(w + (size_t)a * b, w + (size_t)a * b + a);
    t.assign(w, w + (size_t)a * b);
    center_outputs(t, bias, a, b);
    t.insert(t.end(), bias.begin(), bias.end());
  } else return MIND_EINVAL;
  if (t.size() > cap) return MIND_EINVAL;
  memcpy(out, t.data(), t.size() * sizeof(float));
  return (int)t.size();
}

static void sd_of(SD &sd, const mind_tensor_desc *tensors, int n) {
  for (int i = 0; i < n; ++i)
    if (tensors[i].name && tensors[i].data) sd.m[tensors[i].name] = {tensors[i].data, tensors[i].numel};
}

static int debug_pack_blob(const mind_tensor_desc *tensors, int n, WeightBlob &B, char *msg, int msg_cap) {
  if (!tensors || n <= 0 || (msg_cap > 0 && !msg) || msg_cap < 0) return MIND_EINVAL;
  if (msg_cap > 0) msg[0] = 0;
  SD sd;
  sd_of(sd, tensors, n);
  wp_pack(sd, B);
  if (sd.missing.empty()) return MIND_OK;
  if (msg_cap > 0) snprintf(msg, msg_cap, "%s", sd.missing.c_str());
  return MIND_ENOTFOUND;
}

extern "C" int mind_debug_weight_image(const mind_tensor_desc *tensors, int n, float *blob, size_t blob_cap, char *names, size_t names_cap,
                                       long long *entries, int entries_cap, long long *out_info, char *msg, int msg_cap) {
  if (!out_info) return MIND_EINVAL;
  WeightBlob B;
  const int rc = debug_pack_blob(tensors, n, B, msg, msg_cap);
  if (rc != MIND_OK) return rc;
  std::string all;
  for (const WeightBlob::Entry &e : B.entries) all += e.key + "\n";
  out_info[0] = (long long)B.entries.size(); out_info[1] = (long long)B.host.size(); out_info[2] = (long long)all.size() + 1;
  if (blob && blob_cap >= B.host.size()) memcpy(blob, B.host.data(), B.host.size() * sizeof(float));
  if (names && names_cap > all.size()) memcpy(names, all.c_str(), all.size() + 1);
  if (entries && entries_cap >= (int)B.entries.size())
    for (size_t i = 0; i < B.entries.size(); ++i) { entries[2 * i] = (long long)B.entries[i].off; entries[2 * i + 1] = (long long)B.entries[i].len; }
  return MIND_OK;
}

extern "C" int mind_debug_weight_bind(const mind_tensor_desc *tensors, int n, const char *drop, char *msg, int msg_cap) {
  WeightBlob B;
  const int rc = debug_pack_blob(tensors, n, B, msg, msg_cap);
  if (rc != MIND_OK) return rc;
  if (drop && !B.off.erase(drop)) return MIND_EINVAL;
  WeightTables T;
  std::string missing;
  if (wp_bind(B, B.host.data(), T, &missing)) return MIND_OK;
  if (msg_cap > 0) snprintf(msg, msg_cap, "%s", missing.c_str());
  return MIND_ENOTFOUND;
}

extern "C" int mind_weights_load(mind_ctx *c, const mind_tensor_desc *tensors, int n) {
  if (!c || !tensors || n <= 0) return MIND_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  SD sd;
  sd_of(sd, tensors, n);
  WeightBlob B;       // local: a load that fails here leaves the weights loaded before it in place
  wp_pack(sd, B);
  if (!sd.missing.empty()) return fail(c, MIND_ENOTFOUND, "state_dict tensor missing or wrong size: %s", sd.missing.c_str());
  // the context's curve basis: the contents of dec.T / dec.Tp, in place (same shapes: no key is added, no offset moves)
  if (c->dec_basis != MIND_BASIS_BEZIER) wp_basis_tables(c->dec_basis, B.host.data() + B.off.at("dec.T"), B.host.data() + B.off.at("dec.Tp"));
  c->have_weights = false;     // from here on the tables point into freed memory until the bind below
  HIPCHK(c, c->wdev.alloc(B.host.size() * sizeof(float)));
  HIPCHK(c, hipMemcpy(c->wdev.p, B.host.data(), B.host.size() * sizeof(float), hipMemcpyHostToDevice));
  std::string missing;
  if (!wp_bind(B, (float *)c->wdev.p, c->W, &missing)) return fail(c, MIND_ENOTFOUND, "packed weights hold no entry '%s'", missing.c_str());
  c->W.dec.monomial = c->W.decB.monomial = c->dec_basis == MIND_BASIS_MONOMIAL;
  c->have_weights = true;
  return MIND_OK;
}

// -------------------------------------------------------------------------------------------------
// the decoder's curve basis, and its curves at arbitrary times
// -------------------------------------------------------------------------------------------------
static_assert(MIND_BASIS_BEZIER == WP_BASIS_BEZIER && MIND_BASIS_MONOMIAL == WP_BASIS_MONOMIAL, "the packer's basis numbers are the ABI's");

extern "C" int mind_set_decoder_basis(mind_ctx *c, int basis) {
  if (!c) return MIND_EINVAL;
  if (basis != MIND_BASIS_BEZIER && basis != MIND_BASIS_MONOMIAL) return fail(c, MIND_EINVAL, "mind_set_decoder_basis: unknown basis %d", basis);
  if (c->pa_state.load(std::memory_order_acquire) == 1) return fail(c, MIND_ESTATE, "mind_set_decoder_basis: a plan is running on this context");
  if (c->il_finish) return fail(c, MIND_ESTATE, "mind_set_decoder_basis: a tree-iLQR call begun on this context has not been finished");
  if (basis == c->dec_basis) return MIND_OK;
  if (c->have_weights) {
    // rewrite the two tables where the kernels read them, behind everything queued that reads the old ones
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
    std::vector<float> T(60 * 8), Tp(60 * 7);
    wp_basis_tables(basis, T.data(), Tp.data());
    HIPCHK(c, hipMemcpy(const_cast<float *>(c->W.dec.T), T.data(), T.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(const_cast<float *>(c->W.dec.Tp), Tp.data(), Tp.size() * sizeof(float), hipMemcpyHostToDevice));
    c->W.dec.monomial = c->W.decB.monomial = basis == MIND_BASIS_MONOMIAL;
  }
  c->dec_basis = basis;
  return MIND_OK;
}

extern "C" int mind_get_decoder_basis(mind_ctx *c) { return c ? c->dec_basis : MIND_EINVAL; }

// the arguments mind_curve_eval and mind_debug_curve_basis share
static bool curve_args_ok(int basis, const double *tau, int n_tau) {
  if ((basis != MIND_BASIS_BEZIER && basis != MIND_BASIS_MONOMIAL) || !tau || n_tau < 1) return false;
  for (int t = 0; t < n_tau; ++t)
    if (!(tau[t] >= 0.0 && tau[t] <= 1.0)) return false;      // (a NaN fails both comparisons)
  return true;
}

extern "C" int mind_debug_curve_basis(int basis, const double *tau, int n_tau, float *T, float *Tp) {
  if (!curve_args_ok(basis, tau, n_tau) || !T || !Tp) return MIND_EINVAL;
  wp_basis_rows(basis, tau, n_tau, T, Tp);
  return MIND_OK;
}

extern "C" int mind_curve_eval(mind_ctx *c, int basis, const float *param, long long n_rows, const double *tau, int n_tau, float *reg, float *vel,
                               float *cov_vel) {
  if (!c) return MIND_EINVAL;
  if (basis == -1) basis = c->dec_basis;
  if (!curve_args_ok(basis, tau, n_tau)) return fail(c, MIND_EINVAL, "mind_curve_eval: unknown basis, n_tau < 1, or a tau that is not in [0, 1]");
  if (n_rows < 0 || (!reg && !vel && !cov_vel)) return fail(c, MIND_EINVAL, "mind_curve_eval: n_rows < 0 or no output");
  if (n_rows > MIND_CURVE_MAX_POINTS || n_rows * n_tau > MIND_CURVE_MAX_POINTS)
    return fail(c, MIND_EINVAL, "mind_curve_eval: %lld rows x %d times > %lld points supported", n_rows, n_tau, (long long)MIND_CURVE_MAX_POINTS);
  if (n_rows == 0) return MIND_OK;
  if (!param) return fail(c, MIND_EINVAL, "mind_curve_eval: null param");
  HIPCHK(c, hipSetDevice(c->device));
  // the basis rows of (basis, tau): kept on the device between calls (a tracker samples the same times every cycle)
  const size_t tab_floats = (size_t)n_tau * 15;
  if (c->curve_tab_basis != basis || c->curve_tau.size() != (size_t)n_tau || memcmp(c->curve_tau.data(), tau, (size_t)n_tau * sizeof(double)) != 0) {
    std::vector<float> tab(tab_floats);
    wp_basis_rows(basis, tau, n_tau, tab.data(), tab.data() + (size_t)n_tau * 8);
    c->curve_tab_basis = -1;
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (an earlier call's kernel may still read the old rows; `tab` must outlive the copy)
    int rc;
    if ((rc = ensure(c, c->curve_tab, tab_floats * sizeof(float)))) return rc;
    HIPCHK(c, hipMemcpy(c->curve_tab.p, tab.data(), tab_floats * sizeof(float), hipMemcpyHostToDevice));
    c->curve_tau.assign(tau, tau + n_tau);
    c->curve_tab_basis = basis;
  }
  const float *T = (const float *)c->curve_tab.p, *Tp = T + (size_t)n_tau * 8;
  const int n_pts = (int)(n_rows * n_tau);
  hipLaunchKernelGGL(k_dec_curve, dim3((n_pts + DC_T - 1) / DC_T), dim3(DC_T), dc_lds_bytes(n_tau), c->stream, param, n_pts, n_tau, T, Tp,
                     basis == MIND_BASIS_MONOMIAL ? 1 : 0, reg, vel, cov_vel, dc_rows_per_block(n_tau));
  HIPCHK(c, hipGetLastError());
  return MIND_OK;
}

// -------------------------------------------------------------------------------------------------
// predictor forward
// -------------------------------------------------------------------------------------------------
#include "predict.hip"

// -------------------------------------------------------------------------------------------------
// tree-iLQR host side
// -------------------------------------------------------------------------------------------------
#include "ilqr_host.hip"

// -------------------------------------------------------------------------------------------------
// AIME glue (k7): world-frame modes + topology signatures of a round's scenes
// -------------------------------------------------------------------------------------------------
extern "C" int mind_aime_world(mind_ctx *c, const mind_world_in *in, const mind_world_out *out) {
  if (!c || !in || !out || in->n_scenes <= 0 || !in->actor_off || !in->reg || !in->vel || !in->actor_ctrs || !in->actor_vecs ||
      !in->rot || !in->orig || !in->cov_last || !in->last || !out->world || !out->topo || !out->ego_end)
    return fail(c, MIND_EINVAL, "mind_aime_world: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int B = in->n_scenes, A = in->actor_off[B];
  if (A <= 0) return fail(c, MIND_EINVAL, "mind_aime_world: no agents");
  std::vector<AimeScene> hs(B);
  std::vector<int> ascene(A);
  for (int b = 0; b < B; ++b) {
    AimeScene &S = hs[b];
    S.a0 = in->actor_off[b]; S.a1 = in->actor_off[b + 1]; S.last = in->last[b]; S.cmp = 0; S.pad2 = 0.f;
    if (S.a1 <= S.a0) return fail(c, MIND_EINVAL, "mind_aime_world: scene %d has no agents", b);
    S.r00 = in->rot[4 * b]; S.r01 = in->rot[4 * b + 1]; S.r10 = in->rot[4 * b + 2]; S.r11 = in->rot[4 * b + 3];
    S.ox = in->orig[2 * b]; S.oy = in->orig[2 * b + 1];
    S.theta_g = atan2f(S.r10, S.r00);
    for (int i = S.a0; i < S.a1; ++i) ascene[i] = b;
  }
  const size_t bS = ((size_t)B * sizeof(AimeScene) + 15) & ~(size_t)15, bI = ((size_t)A * sizeof(int) + 15) & ~(size_t)15;
  const size_t bC = ((size_t)A * sizeof(float) + 15) & ~(size_t)15;
  const bool select = in->cls && in->scen_prob && out->sel && out->sel_prob;
  const size_t bP = select ? (((size_t)B * sizeof(float) + 15) & ~(size_t)15) : 0;
  const int n_lane = in->target_lane ? in->n_lane_pts : 0;
  if (in->target_lane && n_lane < 2) return fail(c, MIND_EINVAL, "mind_aime_world: target lane needs >= 2 points");
  int rc;
  if (select && in->lane_check) {
    if (!n_lane) return fail(c, MIND_EINVAL, "mind_aime_world: lane_check needs the target lane");
    for (int b = 0; b < B; ++b)
      if (in->last[b] < 0) return fail(c, MIND_EINVAL, "mind_aime_world: lane_check needs last >= 0 (scene %d)", b);
  }
  if ((rc = ensure(c, c->aime_dev, bS + bI + bC + bP + (size_t)(n_lane > 0 ? n_lane : 1) * 2 * sizeof(float)))) return rc;
  char *base = (char *)c->aime_dev.p;
  {
    // one staged host->device copy for the four small tables
    // (the staging buffer lives in the context and is guarded by an event: the copy is queued behind the predictor's kernels and
    // the host goes on to queue k_aime_world / k_aime_select without waiting for them)
    const size_t tot = bS + bI + bC + bP + (size_t)n_lane * 2 * sizeof(float);
    if (c->aime_stage_busy) { HIPCHK(c, hipEventSynchronize(c->ev_stage)); c->aime_stage_busy = false; }
    std::vector<char> &stage = c->aime_stage;
    stage.assign(tot, 0);
    if (select) memcpy(stage.data() + bS + bI + bC, in->scen_prob, (size_t)B * sizeof(float));
    memcpy(stage.data(), hs.data(), (size_t)B * sizeof(AimeScene));
    memcpy(stage.data() + bS, ascene.data(), (size_t)A * sizeof(int));
    memcpy(stage.data() + bS + bI, in->cov_last, (size_t)A * sizeof(float));
    if (n_lane) memcpy(stage.data() + bS + bI + bC + bP, in->target_lane, (size_t)n_lane * 2 * sizeof(float));
    HIPCHK(c, hipMemcpyAsync(base, stage.data(), tot, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipEventRecord(c->ev_stage, st));
    c->aime_stage_busy = true;
  }
  AimeSmall sm0;                  // (tables in memory)
  memset(&sm0, 0, sizeof(sm0));
  hipLaunchKernelGGL(k_aime_world, dim3(A * AIME_K), dim3(64), 0, st, (const AimeScene *)base, (const int *)(base + bS), in->reg, in->vel,
                     in->actor_ctrs, in->actor_vecs, (const float *)(base + bS + bI), out->world, out->topo, out->ego_end,
                     (const float *)(base + bS + bI + bC + bP), n_lane, sm0);
  if (select)
    hipLaunchKernelGGL(k_aime_select, dim3(B), dim3(64), 0, st, (const AimeScene *)base, in->cls, (const float *)(base + bS + bI + bC),
                       out->topo, out->ego_end, in->lane_check ? 1 : 0, in->dist_thres, out->sel, out->sel_prob, 0.001f, sm0);
  HIPCHK(c, hipGetLastError());
  return MIND_OK;
}

extern "C" int mind_aime_rebase(mind_ctx *c, const mind_rebase_in *in, const mind_rebase_out *out) {
  const bool dev_src = in && in->rows_dev;
  if (!c || !in || !out || in->n_scenes <= 0 || in->n_agents <= 0 || in->n_lanes < 0 ||
      (!dev_src && (!in->pos || !in->ang || !in->vel)) || (dev_src && (!in->parent_slot || !in->row0 || !in->dur)) || !in->types ||
      (in->n_lanes > 0 && (!in->lane_ctrs || !in->lane_vecs)) || !in->target_lane || !in->target_lane_info || in->n_lane_pts < 12 ||
      !out->actors || !out->actor_ctrs || !out->actor_vecs || (in->n_lanes > 0 && (!out->lane_ctrs || !out->lane_vecs)) ||
      !out->tgt_nodes || !out->tgt_rpe || !out->frames)
    return fail(c, MIND_EINVAL, "mind_aime_rebase: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t S = in->n_scenes, a = in->n_agents, l = in->n_lanes, P = in->n_lane_pts;
  if (dev_src) {
    if (in->prev_gen != c->rb_gen || c->rb_gen == 0 || c->rb_a != a)
      return fail(c, MIND_ESTATE, "mind_aime_rebase: the parents' windows (generation %d, %zu agents) are not the previous call's (%d, %zu)",
                  in->prev_gen, a, c->rb_gen, c->rb_a);
    for (size_t s_ = 0; s_ < S; ++s_)
      if (in->parent_slot[s_] < 0 || (size_t)in->parent_slot[s_] >= c->rb_S || in->row0[s_] < 0 || in->dur[s_] < 0 || in->dur[s_] > AIME_T)
        return fail(c, MIND_EINVAL, "mind_aime_rebase: scene %zu: parent slot %d / row %d / dur %d out of range", s_, in->parent_slot[s_],
                    in->row0[s_], in->dur[s_]);
  }
  // staging layout (floats): pos | ang | vel | types | pad | lane_ctrs | lane_vecs | tlane | tinfo | (device source: parent_slot | row0 | dur)
  const size_t n_pos = S * a * 50 * 2, n_ang = S * a * 50, n_types = a * 50 * 7, n_pad = in->pad ? S * a * 50 : 0;
  const size_t o_pos = 0, o_ang = o_pos + n_pos, o_vel = o_ang + n_ang, o_types = o_vel + n_pos, o_pad = o_types + n_types;
  const size_t o_lc = o_pad + n_pad, o_lv = o_lc + 2 * l, o_tl = o_lv + 2 * l, o_ti = o_tl + 2 * P, o_idx = o_ti + 12 * P;
  const size_t total = o_idx + (dev_src ? 3 * S : 0);
  // two arenas, used alternately: the windows of THIS call are the parents' windows of the next one
  DevBuf &cur = c->rebase_dev2[c->rb_cur ^ 1];
  const float *prev = (const float *)c->rebase_dev2[c->rb_cur].p;
  const size_t prev_o_ang = c->rb_S * c->rb_a * 50 * 2, prev_o_vel = prev_o_ang + c->rb_S * c->rb_a * 50;
  int rc;
  if ((rc = ensure(c, cur, total * sizeof(float)))) return rc;
  float *d = (float *)cur.p;
  // the arena is contiguous: small rounds (a few child scenes) go in ONE staged copy; big ones (cfg4: 14 MB of windows) copy the
  // three window arrays straight from the caller's memory and stage only the small tables (types | pad | lane anchors | target
  // lane | its info | indices); with a device source the windows are not uploaded at all
  const bool one_copy = !dev_src && total * sizeof(float) <= ((size_t)1 << 20);
  const size_t s0 = one_copy ? 0 : o_types;
  std::vector<float> small(total - s0);
  if (one_copy) {
    memcpy(small.data() + o_pos, in->pos, n_pos * sizeof(float));
    memcpy(small.data() + o_ang, in->ang, n_ang * sizeof(float));
    memcpy(small.data() + o_vel, in->vel, n_pos * sizeof(float));
  } else if (!dev_src) {
    HIPCHK(c, hipMemcpyAsync(d + o_pos, in->pos, n_pos * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d + o_ang, in->ang, n_ang * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d + o_vel, in->vel, n_pos * sizeof(float), hipMemcpyHostToDevice, st));
  }
  memcpy(small.data() + (o_types - s0), in->types, n_types * sizeof(float));
  if (in->pad) memcpy(small.data() + (o_pad - s0), in->pad, n_pad * sizeof(float));
  if (l) {
    memcpy(small.data() + (o_lc - s0), in->lane_ctrs, 2 * l * sizeof(float));
    memcpy(small.data() + (o_lv - s0), in->lane_vecs, 2 * l * sizeof(float));
  }
  memcpy(small.data() + (o_tl - s0), in->target_lane, 2 * P * sizeof(float));
  memcpy(small.data() + (o_ti - s0), in->target_lane_info, 12 * P * sizeof(float));
  if (dev_src) {
    memcpy(small.data() + (o_idx - s0), in->parent_slot, S * sizeof(int));
    memcpy(small.data() + (o_idx - s0) + S, in->row0, S * sizeof(int));
    memcpy(small.data() + (o_idx - s0) + 2 * S, in->dur, S * sizeof(int));
  }
  HIPCHK(c, hipMemcpyAsync(d + s0, small.data(), small.size() * sizeof(float), hipMemcpyHostToDevice, st));
  if (dev_src) {
    const int *di = (const int *)(d + o_idx);
    hipLaunchKernelGGL(k_aime_windows, dim3((unsigned)(S * a)), dim3(64), 0, st, prev, prev + prev_o_ang, prev + prev_o_vel, in->rows_dev,
                       di, di + S, di + 2 * S, (int)a, d + o_pos, d + o_ang, d + o_vel, 1, (float *)nullptr);
  }
  c->rb_cur ^= 1; c->rb_gen += 1; c->rb_S = S; c->rb_a = a;
  if (out->gen) *out->gen = c->rb_gen;
  RebaseArgs A;
  A.a = (int)a; A.l = (int)l; A.n_lane = (int)P; A.pad_ones = in->pad ? 0 : 1;
  A.pos = d + o_pos; A.ang = d + o_ang; A.vel = d + o_vel; A.types = d + o_types; A.pad = in->pad ? d + o_pad : nullptr;
  A.lane_ctrs0 = d + o_lc; A.lane_vecs0 = d + o_lv; A.tlane = d + o_tl; A.tinfo = d + o_ti;
  A.time_ahead = in->time_ahead; A.min_vel = in->min_vel; A.travel0 = -1.f;
  A.actors = out->actors; A.actor_ctrs = out->actor_ctrs; A.actor_vecs = out->actor_vecs; A.lane_ctrs = out->lane_ctrs;
  A.lane_vecs = out->lane_vecs; A.tgt_nodes = out->tgt_nodes; A.tgt_rpe = out->tgt_rpe; A.frames = out->frames;
  hipLaunchKernelGGL(k_aime_rebase, dim3((unsigned)S, 1 + RB_FEAT_BLOCKS(a)), dim3(RB_THREADS), 5 * a * sizeof(float), st, A);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(st));     // the caller's host arrays may be reused after return
  return MIND_OK;
}

// tests: the decision kernels of a round on GIVEN inputs -- k_aime_select + k_aime_branch (fused = 0) or k_aime_select_branch (fused = 1), with
// the launch shapes of PlanRun's round (aime_plan.hip), the scene tables in memory (by_value = 0) or by value in the kernel arguments (AimeSmall).
extern "C" int mind_debug_aime_decide(mind_ctx *c, int n_scenes, const int32_t *actor_off, const int32_t *cmp, const float *cls, const float *scen_prob,
                                      const float *topo, const float *ego_end, const float *world, int lane_check, float dist_thres,
                                      float prob_floor, int fused, int by_value, float *sel, float *sel_prob, uint32_t *hit) {
  if (!c || n_scenes <= 0 || !actor_off || !cmp || !cls || !scen_prob || !topo || !ego_end || !world || !sel || !sel_prob || !hit)
    return fail(c, MIND_EINVAL, "mind_debug_aime_decide: bad argument");
  const int B = n_scenes;
  std::vector<AimeScene> hs(B);
  for (int b = 0; b < B; ++b) {
    AimeScene &S = hs[b];
    memset(&S, 0, sizeof(S));
    S.a0 = actor_off[b]; S.a1 = actor_off[b + 1]; S.last = AIME_T - 1; S.cmp = cmp[b];
    S.r00 = S.r11 = 1.f;
    if (S.a0 < 0 || S.a1 <= S.a0) return fail(c, MIND_EINVAL, "mind_debug_aime_decide: scene %d has no agents", b);
    if (S.cmp < 0 || S.cmp >= AIME_T) return fail(c, MIND_EINVAL, "mind_debug_aime_decide: scene %d: compare step %d out of range", b, S.cmp);
  }
  AimeSmall sm;
  memset(&sm, 0, sizeof(sm));
  if (by_value) {
    const int a = hs[0].a1 - hs[0].a0;
    if (B > AIME_SMALL) return fail(c, MIND_EINVAL, "mind_debug_aime_decide: tables by value hold at most %d scenes (%d given)", AIME_SMALL, B);
    for (int b = 0; b < B; ++b)
      if (hs[b].a1 - hs[b].a0 != a || hs[b].a0 != b * a)
        return fail(c, MIND_EINVAL, "mind_debug_aime_decide: tables by value need the same agent count in every scene");
    memcpy(sm.s, hs.data(), (size_t)B * sizeof(AimeScene));
    memcpy(sm.prob, scen_prob, (size_t)B * sizeof(float));
    sm.n = B; sm.a = a;
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t bS = ((size_t)B * sizeof(AimeScene) + 15) & ~(size_t)15;
  std::vector<char> stage(bS + (size_t)B * sizeof(float), 0);
  memcpy(stage.data(), hs.data(), (size_t)B * sizeof(AimeScene));
  memcpy(stage.data() + bS, scen_prob, (size_t)B * sizeof(float));
  if (by_value) {
    // the tables in memory must not be what the kernels read: they hold other (in-range) contents -- ego-only scenes, another compare step,
    // probability 0 -- so that a kernel that ignored its by-value tables would answer differently
    for (int b = 0; b < B; ++b) {
      AimeScene S = hs[b];
      S.a1 = S.a0 + 1; S.cmp = (S.cmp + 29) % AIME_T;
      memcpy(stage.data() + (size_t)b * sizeof(AimeScene), &S, sizeof(S));
    }
    memset(stage.data() + bS, 0, (size_t)B * sizeof(float));
  }
  char *dtab = nullptr;
  HIPCHK(c, hipMalloc((void **)&dtab, stage.size()));
  hipError_t e = hipMemcpyAsync(dtab, stage.data(), stage.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const AimeScene *t_sc = (const AimeScene *)dtab;
    const float *t_prob = (const float *)(dtab + bS);
    const float pf_ = prob_floor > 0.f ? prob_floor : 0.001f;
    const int lc = lane_check ? 1 : 0;
    if (fused) {
      hipLaunchKernelGGL(k_aime_select_branch, dim3(B * AIME_K), dim3(64), 0, st, t_sc, cls, t_prob, topo, ego_end, lc, dist_thres, pf_, world, sel, sel_prob,
                         hit, (float *)nullptr, (float *)nullptr, (unsigned *)nullptr, sm, AimeDone{nullptr, nullptr, 0u});
    } else {
      hipLaunchKernelGGL(k_aime_select, dim3(B), dim3(64), 0, st, t_sc, cls, t_prob, topo, ego_end, lc, dist_thres, sel, sel_prob, pf_, sm);
      hipLaunchKernelGGL(k_aime_branch, dim3(B * AIME_K), dim3(64), 0, st, t_sc, (const float *)sel, world, hit, (const float *)sel_prob, (float *)nullptr,
                         (float *)nullptr, (unsigned *)nullptr, sm, AimeDone{nullptr, nullptr, 0u});
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  (void)hipFree(dtab);
  HIPCHK(c, e);
  return MIND_OK;
}

#include "aime_plan.hip"

// ---- MINDPlanner.evaluate_traj_tree (planner.py:180-198) for all candidate trajectory trees of a plan: mean over a tree's nodes of
//      .1 jerk^2 + 5 steer_rate^2 + .01 (v_tgt - v)^2 + .01 dist(target lane).  Host only (a few 10^4 point-segment pairs); float64 with
//      numpy's operation order (per-node terms left to right, the per-tree sum as np.add.reduceat forms it: first element + pairwise
//      sum of the rest, blocks of 8 / 128), so that the strict `<` scan over the candidates sees the costs numpy computes.
namespace {
double np_pairwise(const double *a, long n) {
  if (n < 8) {
    double r = 0.0;
    for (long i = 0; i < n; ++i) r += a[i];
    return r;
  }
  if (n <= 128) {
    double r[8];
    long i;
    for (i = 0; i < 8; ++i) r[i] = a[i];
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  long n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise(a, n2) + np_pairwise(a + n2, n - n2);
}
template <class T>
void eval_nodes(const double *st, const double *ct, long N, const T *lane, int P, double tv, double *per_node) {
  const int S = P - 1;
  std::vector<T> dx(S), dy(S), l2(S);
  for (int q = 0; q < S; ++q) {
    dx[q] = lane[2 * q + 2] - lane[2 * q];
    dy[q] = lane[2 * q + 3] - lane[2 * q + 1];
    l2[q] = dx[q] * dx[q] + dy[q] * dy[q];                      // in the lane's own dtype, as numpy computes it
  }
  // A segment with l2 == 0 divides by zero.  A repeated lane point (dx == dy == 0) has a zero numerator too: numpy's t = 0 / 0 is NaN for
  // EVERY node, and np.min propagates it -- the whole lane prices NaN, whichever segments the scan below would visit.  Where only the
  // float32 sum of squares underflows (dx or dy != 0), t = +-inf clips to 0 / 1 and stays finite, or is NaN for a node whose numerator
  // is exactly zero: such segments are priced for every node before the scan, so the outcome never depends on the pruning.
  bool repeated_point = false;
  std::vector<int> always;
  for (int q = 0; q < S; ++q) {
    if (l2[q] != (T)0) continue;
    if (dx[q] == (T)0 && dy[q] == (T)0) repeated_point = true;
    else always.push_back(q);
  }
  // Only the MINIMUM over the segments is used, so a segment that provably cannot hold it is not priced: segments are grouped in blocks of
  // eight with a bounding circle (centre, radius inflated by 1e-9 relative + 1e-9 m: far above any rounding of the distances involved), and a
  // block -- then a segment, by its own circle -- is skipped when |p - centre| > sqrt(current minimum) + radius.  Every segment that could
  // equal or undercut the running minimum is evaluated with numpy's expression, so the result is the same bits; a trajectory's
  // nodes follow the lane, so the scan starts at the block that held the previous node's minimum.
  constexpr int BS = 8;
  const int NB = (S + BS - 1) / BS;
  std::vector<double> sx_(S), sy_(S), sr_(S), bx(NB), by(NB), br(NB);
  for (int q = 0; q < S; ++q) {
    const double ax = (double)lane[2 * q], ay = (double)lane[2 * q + 1], ex = (double)lane[2 * q + 2], ey = (double)lane[2 * q + 3];
    sx_[q] = 0.5 * (ax + ex); sy_[q] = 0.5 * (ay + ey);
    sr_[q] = 0.5 * sqrt((ex - ax) * (ex - ax) + (ey - ay) * (ey - ay)) * (1.0 + 1e-9) + 1e-9;
  }
  for (int b = 0; b < NB; ++b) {
    const int q0 = b * BS, q1 = std::min(S, q0 + BS);
    double cx = 0.0, cy = 0.0;
    for (int q = q0; q < q1; ++q) { cx += sx_[q]; cy += sy_[q]; }
    cx /= (double)(q1 - q0); cy /= (double)(q1 - q0);
    double r = 0.0;
    for (int q = q0; q < q1; ++q) r = std::max(r, sqrt((sx_[q] - cx) * (sx_[q] - cx) + (sy_[q] - cy) * (sy_[q] - cy)) + sr_[q]);
    bx[b] = cx; by[b] = cy; br[b] = r * (1.0 + 1e-9) + 1e-9;
  }
  int b_prev = 0;
  for (long i = 0; i < N; ++i) {
    const double px = st[6 * i], py = st[6 * i + 1];
    // min over the segments of sqrt(e) = sqrt of the min of e: the correctly rounded square root is monotone, so ONE square root per node
    // gives numpy's bits (np.sqrt per segment, then min) -- the division and the square root share the host's divider unit
    double emin = INFINITY, rmin = INFINITY;
    bool saw_nan = false;
    int b_best = b_prev;
    auto price_segment = [&](int q, int b, bool prune) {
      if (prune && emin < INFINITY) {
        const double cxq = px - sx_[q], cyq = py - sy_[q], lim = rmin + sr_[q];
        if (cxq * cxq + cyq * cyq > lim * lim) return;
      }
      const double sx = (double)lane[2 * q], sy = (double)lane[2 * q + 1], ddx = (double)dx[q], ddy = (double)dy[q];
      double t = ((px - sx) * ddx + (py - sy) * ddy) / (double)l2[q];
      t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
      const double ex = px - (sx + t * ddx), ey = py - (sy + t * ddy);
      const double e = ex * ex + ey * ey;
      if (e < emin) { emin = e; rmin = sqrt(e) * (1.0 + 1e-9) + 1e-9; b_best = b; }
      else if (e != e) saw_nan = true;                            // numpy's min propagates a NaN
    };
    auto price_block = [&](int b) {
      const int q0 = b * BS, q1 = std::min(S, q0 + BS);
      for (int q = q0; q < q1; ++q) price_segment(q, b, true);
    };
    for (int q : always) price_segment(q, q / BS, false);
    price_block(b_prev);
    for (int b = 0; b < NB; ++b) {
      if (b == b_prev) continue;
      if (emin < INFINITY) {
        const double cxb = px - bx[b], cyb = py - by[b], lim = rmin + br[b];
        if (cxb * cxb + cyb * cyb > lim * lim) continue;
      }
      price_block(b);
    }
    b_prev = b_best;
    const double dmin = (saw_nan || repeated_point) ? (double)NAN : sqrt(emin);
    const double c0 = ct[2 * i], c1 = ct[2 * i + 1], dv = tv - st[6 * i + 2];
    per_node[i] = ((0.1 * (c0 * c0) + 5.0 * (c1 * c1)) + 0.01 * (dv * dv)) + 0.01 * dmin;
  }
}
}  // namespace

// get_agent_trajectories' array part (planners/mind/utils.py:245-342 of the reference: per track the observed flags, positions and headings
// of unobserved steps taken from the nearest earlier observed one -- the first observed one before it --, velocities zero there, the type
// one-hot on observed steps) for all tracks at once; host arithmetic, plain copies and float64 -> float32 casts.
extern "C" int mind_fill_tracks(const double *raw /*[a,T,6]: observed, x, y, heading, vx, vy*/, int a, int T, const int32_t *slot /*[a]*/,
                                float *pos /*[a,T,2]*/, float *ang /*[a,T]*/, float *vel /*[a,T,2]*/, int16_t *typ /*[a,T,7]*/,
                                int16_t *have /*[a,T]*/) {
  if (!raw || !slot || !pos || !ang || !vel || !typ || !have || a < 0 || T <= 0) return MIND_EINVAL;
  for (int i = 0; i < a; ++i) {
    const double *r = raw + (size_t)i * T * 6;
    int first = 0;
    for (int t = 0; t < T; ++t)
      if (r[t * 6] != 0.0) { first = t; break; }       // np.argmax(have): the first observed step (0 when none is)
    int src = -1;
    for (int t = 0; t < T; ++t) {
      const bool h = r[t * 6] != 0.0;
      if (h) src = t;
      const int f = src < 0 ? first : src;
      const bool hf = r[f * 6] != 0.0;                  // (a track without any observed step fills with zeros, as np.where(have, raw, 0) does)
      const size_t o = (size_t)i * T + t;
      pos[2 * o] = hf ? (float)r[f * 6 + 1] : 0.f;
      pos[2 * o + 1] = hf ? (float)r[f * 6 + 2] : 0.f;
      ang[o] = hf ? (float)r[f * 6 + 3] : 0.f;
      vel[2 * o] = h ? (float)r[t * 6 + 4] : 0.f;
      vel[2 * o + 1] = h ? (float)r[t * 6 + 5] : 0.f;
      have[o] = h ? 1 : 0;
      for (int k = 0; k < 7; ++k) typ[o * 7 + k] = (h && k == slot[i]) ? 1 : 0;
    }
  }
  return MIND_OK;
}

extern "C" int mind_eval_traj_trees(const double *states, const double *ctrls, const int32_t *counts, int n_trees, const void *lane,
                                    int lane_is_f32, int n_lane_pts, double target_vel, double *out) {
  if (!states || !ctrls || !counts || n_trees <= 0 || !lane || n_lane_pts < 2 || !out) return MIND_EINVAL;
  long N = 0;
  for (int t = 0; t < n_trees; ++t) { if (counts[t] <= 0) return MIND_EINVAL; N += counts[t]; }
  std::vector<double> per(N);
  // the nodes are priced independently (a node = one distance-to-polyline scan): big plans -- the deep stress trees hold 177 k trajectory
  // nodes -- are spread over a few host threads; the per-tree sums below keep numpy's order either way
  auto run = [&](long lo, long hi) {
    if (lane_is_f32) eval_nodes<float>(states + 6 * lo, ctrls + 2 * lo, hi - lo, (const float *)lane, n_lane_pts, target_vel, per.data() + lo);
    else eval_nodes<double>(states + 6 * lo, ctrls + 2 * lo, hi - lo, (const double *)lane, n_lane_pts, target_vel, per.data() + lo);
  };
  const long nth = std::min<long>(std::min<long>(8, (long)std::max(1u, std::thread::hardware_concurrency())), N / 8192);
  if (nth <= 1) run(0, N);
  else {
    std::vector<std::thread> th;
    for (long k = 0; k < nth; ++k) th.emplace_back(run, N * k / nth, N * (k + 1) / nth);
    for (std::thread &t : th) t.join();
  }
  long o = 0;
  for (int t = 0; t < n_trees; ++t) {
    const long n = counts[t];
    out[t] = (n > 1 ? per[o] + np_pairwise(per.data() + o + 1, n - 1) : per[o]) / (double)n;
    o += n;
  }
  return MIND_OK;
}

// ---- debug taps (tests only): run only the first n fusion layers; read back internal buffers
// the kernel-side sin / cos / tan on an array (tests: bitwise equality with the oracle's build of the same header)
__global__ void k_debug_trig(const double *__restrict__ x, int n, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double v = i < n ? x[i] : 0.0;          // (the wave-uniform small-argument path needs every lane of the wave in the call)
  double s, c, t, c2;
  mind_sincos(v, &s, &c);
  mind_tan_cos(v, &t, &c2);
  if (i < n) { out[4 * i] = s; out[4 * i + 1] = c; out[4 * i + 2] = t; out[4 * i + 3] = c2; }
}
extern "C" int mind_debug_trig(mind_ctx *c, const double *x, int n, double *out) {
  if (!c || !x || !out || n <= 0) return MIND_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  double *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, (size_t)n * 5 * sizeof(double)));
  hipError_t e = hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_debug_trig, dim3((n + 63) / 64), dim3(64), 0, c->stream, d, n, d + n);
    e = hipStreamSynchronize(c->stream);
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + n, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(c, MIND_EHIP, "mind_debug_trig: %s", hipGetErrorString(e));
  return MIND_OK;
}

// the decoder's scene part alone, in a given form, on the caller's token rows (tests, tools/dec_chain_forms.py)
extern "C" int mind_debug_dec_scene(mind_ctx *c, const float *rows, int n_scenes, int form, float *Cout, float *cls, int reps, float *ms) {
  if (!c || !rows || !Cout || !cls || n_scenes <= 0 || n_scenes > 4096 || !(form == 0 || dc_valid_g(form)) || reps < 1 || reps > 1024) return MIND_EINVAL;
  if (!c->have_weights) return fail(c, MIND_ESTATE, "weights not loaded");
  HIPCHK(c, hipSetDevice(c->device));
  const int B = n_scenes;
  const size_t nx = (size_t)B * 128, nc = (size_t)B * 768, nk = (size_t)B * 6;
  DevBuf d;                       // x [B,128] | Cout [B,768] | cls [B,6] | cls_row [B]
  if (d.alloc((nx + nc + nk) * sizeof(float) + (size_t)B * sizeof(int)) != hipSuccess) return fail(c, MIND_ENOMEM, "mind_debug_dec_scene: hipMalloc failed");
  float *dx = d.as<float>(), *dC = dx + nx, *dk = dC + nc;
  int *drow = (int *)(dk + nk);
  std::vector<int> row(B);
  for (int b = 0; b < B; ++b) row[b] = b;
  HIPCHK(c, hipMemcpy(dx, rows, nx * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(drow, row.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
  Event e0, e1;
  if (ms && (e0.create() != hipSuccess || e1.create() != hipSuccess)) return fail(c, MIND_EHIP, "mind_debug_dec_scene: no events");
  for (int it = 0; it < reps; ++it) {
    if (ms) HIPCHK(c, hipEventRecord(e0, c->stream));
    if (form == 0)
      hipLaunchKernelGGL(k_dec_scene, dim3(B), dim3(DT), mind_dec_scene_lds_bytes(), c->stream, (const float *)dx, (const int *)drow, dC, dk, c->W.dec);
    else if (int rc = dec_chain_run(c, form, B, dx, drow, dC, dk, c->stream))
      return rc;
    if (ms) {
      HIPCHK(c, hipEventRecord(e1, c->stream));
      HIPCHK(c, hipEventSynchronize(e1));
      HIPCHK(c, hipEventElapsedTime(&ms[it], e0, e1));
    }
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(Cout, dC, nc * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(cls, dk, nk * sizeof(float), hipMemcpyDeviceToHost));
  return MIND_OK;
}

extern "C" int mind_debug_set_layers(mind_ctx *c, int n) {
  if (!c || n < 0 || n > 6) return MIND_EINVAL;
  c->debug_layers = n;
  return MIND_OK;
}
extern "C" int64_t mind_debug_read(mind_ctx *c, const char *name, float *host, int64_t max_floats) {
  if (!c || !name) return MIND_EINVAL;
  const void *src = nullptr;
  int64_t n = 0;
  std::string k = name;
  if (k == "x") { src = c->x.p; n = (int64_t)c->last_ntok * 128; }
  else if (k == "ST") { src = c->ST.p; n = (int64_t)c->last_ntok * 256; }
  else if (k == "QK") { src = c->QK.p; n = (int64_t)c->last_ntok * 1024; }
  else if (k == "edge") { src = c->edge.p; n = c->last_edge_pairs * 128; }
  else if (k == "part") { src = c->part.p; n = (int64_t)c->last_slots * PART_STRIDE; }
  else if (k == "actor_feat") { src = c->actor_feat.p; n = (int64_t)c->last_A * 128; }
  else if (k == "tokpos") { src = c->tokpos.p; n = (int64_t)c->last_ntok * 4; }
  else if (k == "cmode") { src = c->cmode.p; n = (int64_t)c->last_B * 768; }
  else if (k == "tgt_emb") { src = c->tgt_emb.p; n = (int64_t)c->last_B * 128; }
  else if (k == "tgt_feat") { src = c->tgt_feat.p; n = (int64_t)c->last_B * 128; }
  else if (k == "pl_root") { src = c->pl_root.p; n = (int64_t)(c->pl_root.cap / sizeof(float)); }    // the last plan's root scene (RootLayout, aime_book.h)
  else if (k == "il_spec") {        // the derivative speculator in the last tree-iLQR launch: {passes it was asked in, results the master took}
    if (!host) return 2;
    if (max_floats < 2) return MIND_EINVAL;
    host[0] = (float)c->il_spec_req; host[1] = (float)c->il_spec_hit;
    return 2;
  }
  else if (k.rfind("il_", 0) == 0 && c->il_dbg[5]) {
    // float64 arrays of tree 0 of the last tree-iLQR call, returned as raw bytes (2 floats per double)
    const size_t M = c->il_dbg[5];
    int w = -1; size_t per = 0;
    if (k == "il_L") { w = 0; per = 1; } else if (k == "il_Lx") { w = 1; per = 6; } else if (k == "il_Lxx") { w = 2; per = 36; }
    else if (k == "il_Fx") { w = 3; per = 36; } else if (k == "il_xs") { w = 4; per = 6; }
    if (w < 0) return MIND_EINVAL;
    src = (const char *)c->ilqr_dev.p + c->il_dbg[w];
    n = (int64_t)(M * per * 2);
  }
  else return MIND_EINVAL;
  if (!host) return n;
  if (n > max_floats) n = max_floats;
  if (hipStreamSynchronize(c->stream) != hipSuccess) return MIND_EHIP;
  if (k == "edge" && c->last_edge_tiled) {
    // k_pair_t keeps the tensor as [scene][column j][tile][chunk b 8][lane 64][4]: hand back the logical [scene][j][i][128]
    long long pt = 0;
    for (int N : c->last_scene_n) pt += (long long)N * (((N + 15) / 16) * 16);
    const bool eb = c->last_edge_bf16;      // plain bf16 arithmetic: [k-group 4][lane 64][4 dwords of two bf16], 64 dwords per pair
    std::vector<float> raw((size_t)pt * (eb ? 64 : 128));
    if (hipMemcpy(raw.data(), src, raw.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return MIND_EHIP;
    int64_t o = 0;
    size_t sb = 0;
    for (int N : c->last_scene_n) {
      const int rows = ((N + 15) / 16) * 16;
      for (int j = 0; j < N; ++j)
        for (int i = 0; i < N; ++i)
          for (int f = 0; f < 128 && o < n; ++f, ++o) {
            const int t = i >> 4, pp = i & 15, b = f >> 4, qq = (f >> 2) & 3, r = f & 3;
            const size_t tile0 = sb + (size_t)j * rows + (size_t)t * 16;
            if (!eb) host[o] = raw[tile0 * 128 + ((b * 64 + qq * 16 + pp) * 4 + r)];
            else {
              uint32_t w;
              memcpy(&w, &raw[tile0 * 64 + (((b >> 1) * 64 + qq * 16 + pp) * 4 + 2 * (b & 1) + (r >> 1))], 4);
              w = (r & 1) ? (w & 0xffff0000u) : (w << 16);
              memcpy(&host[o], &w, 4);
            }
          }
      sb += (size_t)N * rows;
    }
    return n;
  }
  if (hipMemcpy(host, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return MIND_EHIP;
  return n;
}

// ---- the closed loop of one scene behind one call per step (host code: the interpreter's share of a planning cycle)
#include "loop.hip"

// ---- the clearance audit of plans and episodes (outside every planning cycle)
#include "audit_host.hip"

// ---- forecast scoring against recorded futures (outside every planning cycle)
#include "forecast_host.hip"

// ---- the road audit of plans and episodes (outside every planning cycle)
#include "road_host.hip"

// ---- the time-to-collision audit of episodes (outside every planning cycle)
#include "ttc_host.hip"

// ---- the lane audit of plans and episodes (outside every planning cycle)
#include "lane_host.hip"
