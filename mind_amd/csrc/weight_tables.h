// The pointer tables the predictor kernels take by value: one struct per network and weight packing, every pointer into the packed device
// blob that mind_weights_load uploads.  wp_bind (weight_pack.h) fills them; the kernel files read them.  Plain C++: no HIP header, so the host
// code that fills the tables compiles (and is tested) without a device.
#pragma once

typedef unsigned int u32;

// ---- LaneNet (encdec_kernels.hip)
struct LaneW {
  const float *pW, *pb, *pg, *pbe;  // proj 16->128 (+LN)
  // aggre blocks 0/1: fc1.0, fc1.3, fc2.0 (256->128), fc2.3, norm
  const float *f10W[2], *f10b[2], *f10g[2], *f10be[2];
  const float *f13W[2], *f13b[2], *f13g[2], *f13be[2];
  const float *f20W[2], *f20b[2], *f20g[2], *f20be[2];
  const float *f23W[2], *f23b[2], *f23g[2], *f23be[2];
  const float *ng[2], *nbe[2];
};

// ---- ActorNet.  ds / gd / bd are null in the residual blocks that have no downsample (the second block of every group, the output block).
// VALU form (encdec_kernels.hip): conv weights stored [ci][dk][co]
struct ResW { const float *c1, *g1, *b1, *c2, *g2, *b2, *ds, *gd, *bd; };
struct ActorW {
  ResW res[9];                 // groups.{0..3}.{0,1}, output
  const float *latW[4], *latG[4], *latB[4];
};

// bf16 hi / mid / lo MFMA fragments (actor_mfma_kernels.hip, actor_lw_kernels.hip)
struct AmRes { const u32 *c1, *c2, *ds; const float *g1, *b1, *g2, *b2, *gd, *bd; };
struct AmLat { const u32 *w; const float *g, *b; };
struct AmW {                                // packed conv fragments + GroupNorm affine, same order as ActorW
  AmRes res[9];
  AmLat lat[4];
};

// fp32 MFMA fragments (actor_f32_kernels.hip)
struct AfRes { const float *c1, *c2, *ds; const float *g1, *b1, *g2, *b2, *gd, *bd; };
struct AfLat { const float *w; const float *g, *b; };
struct AfW {                                // packed conv fragments + GroupNorm affine, same order as ActorW / AmW
  AfRes res[9];
  AfLat lat[4];
};

// ---- fusion layers, pair kernels (fusion_kernels.hip, pair_*_kernels.hip)
// per-layer small vectors, staged in LDS (floats): 7 x 128
//  0: gamma_m 1: beta_m 2: b_p 3: gamma_p 4: beta_p 5: gamma_e 6: beta_e
#define VT_GM 0
#define VT_BM 128
#define VT_BP 256
#define VT_GP 384
#define VT_BEP 512
#define VT_GE 640
#define VT_BE 768
#define VT_SIZE 896

// [L]: proj_memory (e) and proj_edge (p) of fusion layer L.  The last layer has no proj_edge: its p entries are null.
struct PairW {
  const float *WAe[6], *WAp[6];   // fp32 MFMA A fragments (k_pair)
  const u32 *WBe[6], *WBp[6];     // bf16 hi / lo fragments of the same matrices (pair_bf16_kernels.hip)
  const u32 *WLe[6], *WLp[6];     // the third part of the exact three-way split (hi + mid + lo; mid = the two-way split's lo): k_pair_t6
  const float *vtab[6];           // VT_* vectors
  const float *rtab;              // rpe table (all layers)
};

// ---- fusion layers, token kernels.  Table [L] of 7: epilogue of layer L-1 (L>=1) + prologue of layer L (L<=5); [0] = init
struct TokWeights {               // fusion_kernels.hip
  // epilogue of layer L (may be null when init)
  const float *WvT, *bv, *WoT, *bo, *g2, *b2, *W1T, *b1, *W2T, *bb2, *g3, *b3;
  // prologue of layer L+1 (may be null for the last layer)
  const float *WsT, *WtT, *bm, *WqT, *bq, *Wk;
  // init projections
  const float *WpaT, *bpa, *gpa, *bepa, *WplT, *bpl, *gpl, *bepl;
};

struct TokWeightsM {   // A-fragment packings (pack_afrag) of the matrices TokWeights holds transposed (token_mfma_kernels.hip)
  const float *Wv, *Wo, *W1a, *W1b, *W2a, *W2b;     // epilogue of layer L-1 (W1: output halves; W2: input halves)
  const float *Ws, *Wt, *Wq, *Wkf;                  // prologue of layer L (Wkf: per head [8][ob 8][lane 64][4], see pack_wk_frag)
  const float *Wpa, *Wpl;                           // init projections
};

// ---- SceneDecoder
struct DecW {                     // encdec_kernels.hip
  const float *rpeW, *rpeb, *rpeg, *rpebe;                       // proj_rpe 20(->pad 20)->128
  const float *t0W, *t0b, *t0g, *t0be, *t3W, *t3b, *t3g, *t3be;  // proj_tgt
  const float *c0W, *c0b, *c0g, *c0be, *c3W, *c3b, *c3g, *c3be;  // ctx_proj 128->384->768
  const float *a0W, *a0b, *a0g, *a0be, *a3W, *a3b, *a3g, *a3be;  // actor_proj
  const float *inW[2], *inb[2], *outW[2], *outb[2], *l1W[2], *l1b[2], *l2W[2], *l2b[2];
  const float *n1g[2], *n1b[2], *n2g[2], *n2b[2];
  const float *k0W, *k0b, *k0g, *k0be, *k3W, *k3b, *k3g, *k3be, *k6W, *k6b;  // cls head
  const float *r0W, *r0b, *r0g, *r0be, *r3W, *r3b, *r3g, *r3be, *r6W, *r6b;  // reg head
  const float *T, *Tp;                                                           // [60][8], [60][7]: the basis the context is set to (mind_set_decoder_basis)
  int monomial;                                                                  // the vel formula: 0 = Tp diff(P) / 6 (Bezier), 1 = Tp P[1:] / 6 (network.py:519 / :530)
};

struct DmW {                      // actor part of the decoder as bf16 fragments (dec_mfma_kernels.hip)
  const u32 *a0, *a3, *r0, *r3, *r6;              // packed fragments
  const float *a0b, *a0g, *a0be, *a3b, *a3g, *a3be, *r0b, *r0g, *r0be, *r3b, *r3g, *r3be, *r6b;
  const float *T, *Tp;                            // the bases [60][8], [60][7] and the vel formula, as in DecW
  int monomial;
};

// everything mind_ctx holds of the loaded weights
struct WeightTables {
  LaneW lane;
  ActorW actor;
  AmW actorB;            // the same convolutions as bf16 hi / mid / lo MFMA fragments
  AfW actorF;            // ... and as fp32 MFMA A fragments
  PairW pair;
  TokWeights tok[7];
  TokWeightsM tokM[7];   // the same matrices as fp32 MFMA A fragments (k_token_mfma<0>)
  TokWeightsM tokB[7];   // ... and as bf16 hi / lo A fragments (k_token_mfma<1>: scenes of >= tok_bf_min_n tokens)
  DecW dec;
  DmW decB;
};
