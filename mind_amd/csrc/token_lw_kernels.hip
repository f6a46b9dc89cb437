// The token stage layer-wise: k_token_mfma<0>'s arithmetic (token_mfma_kernels.hip) as one launch per STAGE over a chunk of tokens, for
// rounds of thousands of tokens.  k_token_mfma gives 16 tokens to a workgroup, which streams the 64 KB of A fragments of every
// projection (about twelve per launch) and keeps 97 KB of LDS: one four-wave workgroup per CU, waiting on fragment and partial-sum
// loads.  A 128 x 128 projection's fragments are exactly what the four waves of a workgroup hold in registers (TmFrag: 64 VGPRs per
// lane), so here a workgroup loads the fragments of ITS stage once per launch and sweeps 16-token tiles past them (grid sized from the
// CU count, tile = blockIdx.x, + gridDim.x, ...); a tile passes through 8 - 25 KB of LDS, several workgroups share a CU, and the
// activations between stages live in an arena of one chunk of tokens (o 128 | x1 128 | h 256 | q 128 floats per token).
//
//   stage 0  k_tl_init     x = relu(LN(proj_actor | proj_lane (feature))), cls row zero            (mode & 1)
//   stage 1  k_tl_merge_v  softmax merge of the column partials + V projection -> o               (mode & 2)
//   stage 2  k_tl_proj_ln<1>  x1 = LN2(x + W_o o + b_o)
//   stage 3  k_tl_proj     h = relu(W_1 x1 + b_1): blockIdx.y = output half
//   stage 4  k_tl_proj_ln<2>  x = LN3(x1 + W_2 h + b_2): the two input halves chained on one accumulator
//   stage 5  k_tl_proj     S = W_s x, T = W_t x + b_m, q = W_q x + b_q: blockIdx.y = matrix          (mode & 4)
//   stage 6  k_tl_kq       folded K query + the QK formats of mode & 16 / mode & 32
//
// Nothing is restated: every projection is tm_mma<0> on TmFrag fragments (the merge stage feeds the same MFMA sequence -- K in the order
// s4 = 0..7, w = 0..3 -- from registers: its B operand is the merged partial sum itself, so no mb tile and no LDS at all), the
// LayerNorms are tm_layernorm on a [16][TM_LDX] tile, the merge weights, bias adds, ReLU, * 0.25f and the QK packing are
// k_token_mfma<0>'s expressions in its order.  A token's result depends on nothing but the token, so tiles, chunks and the position in
// the launch do not show in the bits.
//
// included by mind_hip.hip behind token_mfma_kernels.hip (TmFrag, tm_load, tm_mma, tm_layernorm, TM_*)
#define TL_T 256
#define TL_CHUNK 32768       // tokens per chunk ("tok_lw_chunk" 0): 80 MiB of arena
#define TL_ROW 640           // arena floats per token
#define TL_NSTAGE 7
#define TL_NCU_PLAN 256      // CU count mind_debug_token_lw_plan sizes its grids with (the MI355X's; mind_predict_batch uses the device's)

// workgroups per CU a stage's grid is sized for (from the registers and LDS of each kernel)
static const int tl_wg_per_cu[TL_NSTAGE] = {2, 2, 3, 4, 2, 4, 4};

// a [16][COLS] tile of row-major global rows -> LDS rows of stride ld (rows >= nt: zeros)
template <int COLS>
__device__ __forceinline__ void tl_tile_in(float *dst, int ld, const float *__restrict__ src, int nt, int tid) {
  constexpr int C4 = COLS / 4;
  for (int e = tid; e < TM_TOK * C4; e += TL_T) {
    const int t = e / C4, c = (e % C4) * 4;
    tm_f4 v = {0, 0, 0, 0};
    if (t < nt) v = *reinterpret_cast<const tm_f4 *>(src + (size_t)t * COLS + c);
    *reinterpret_cast<tm_f4 *>(dst + t * ld + c) = v;
  }
}
__device__ __forceinline__ void tl_tile_out(float *__restrict__ dst, const float *src, int ld, int nt, int tid) {
  for (int e = tid; e < nt * 32; e += TL_T) {
    const int t = e >> 5, c = (e & 31) * 4;
    *reinterpret_cast<tm_f4 *>(dst + (size_t)t * 128 + c) = *reinterpret_cast<const tm_f4 *>(src + t * ld + c);
  }
}

// ---- stage 0: FusionNet's input projections (network.py:313-314, 323-324): both matrices stationary, the token's type picks the row
__global__ __launch_bounds__(TL_T) void k_tl_init(const TokMeta *__restrict__ meta, int n_tok, const float *__restrict__ actor_feat,
                                                  const float *__restrict__ lane_feat, float *__restrict__ x, TokWeights W, const float *__restrict__ Wpa,
                                                  const float *__restrict__ Wpl) {
  __shared__ __attribute__((aligned(16))) float tmp[TM_TOK * TM_LDX], xs[TM_TOK * TM_LDX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ob0 = 2 * wave, tk = lane & 15;
  TmFrag Fa, Fl;
  tm_load(Fa, Wpa, ob0, lane);
  tm_load(Fl, Wpl, ob0, lane);
  const int ntiles = (n_tok + TM_TOK - 1) / TM_TOK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tok0 = tile * TM_TOK, nt = min(TM_TOK, n_tok - tok0);
    for (int e = tid; e < TM_TOK * 128; e += TL_T) {
      const int t = e >> 7, col = e & 127;
      float f = 0.f;
      if (t < nt) {
        const TokMeta m = meta[tok0 + t];
        if (m.type == 0) f = actor_feat[(size_t)m.src * 128 + col];
        else if (m.type == 1) f = lane_feat[(size_t)m.src * 128 + col];
      }
      tmp[t * TM_LDX + col] = f;
    }
    __syncthreads();
    const int ty = tk < nt ? meta[tok0 + tk].type : 2;
    tm_f4 aa[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, al[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    tm_mma<0>(aa, Fa, ob0, tmp + tk * TM_LDX, 0, lane);
    tm_mma<0>(al, Fl, ob0, tmp + tk * TM_LDX, 0, lane);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = TM_FEAT(ob0 + t, i);
        xs[tk * TM_LDX + f] = ty == 0 ? aa[t][i] + W.bpa[f] : al[t][i] + W.bpl[f];
      }
    __syncthreads();
    {
      const int row = tid >> 4, prt = tid & 15;
      const int tyr = row < nt ? meta[tok0 + row].type : 2;
      tm_layernorm(xs, TM_LDX, tyr == 0 ? W.gpa : W.gpl, tyr == 0 ? W.bepa : W.bepl, true, tid);
      if (tyr == 2) {
#pragma unroll
        for (int k = 0; k < 8; ++k) xs[row * TM_LDX + prt * 8 + k] = 0.f;
      }
    }
    __syncthreads();
    tl_tile_out(x + (size_t)tok0 * 128, xs, TM_LDX, nt, tid);
    __syncthreads();
  }
}

// ---- stage 1: o = W_v,h mbar_h + b_v, mbar_h = sum_s (exp(m_s - M) / L) part[slot0 + s][head h]: output block ob = head ob, so a lane's
// B operand of block ob is its token's merged sum of head ob -- built in registers from the partial slots (float4 loads, 64 B per token,
// head and k-step), no LDS, no barrier.  The weights are k_token_mfma's: e = expf(m_s - M), L += e l_s in slot order, e * (1 / L).
__global__ __launch_bounds__(TL_T) void k_tl_merge_v(const TokMeta *__restrict__ meta, int n_tok, int mode, const float *__restrict__ part,
                                                     float *__restrict__ o, const float *__restrict__ Wv, const float *__restrict__ bv) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ob0 = 2 * wave, tk = lane & 15, q4 = 4 * (lane >> 4);
  TmFrag F;
  tm_load(F, Wv, ob0, lane);
  const int ntiles = (n_tok + TM_TOK - 1) / TM_TOK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tok = tile * TM_TOK + tk;
    const bool ok = tok < n_tok;
    int ns = 0, slot0 = 0;
    if (ok) {
      const TokMeta m = meta[tok];
      ns = ((mode & 8) && !(m.flags & 1)) ? 0 : m.nsplit;      // (last layer: lane tokens are not consumed, their sum stays zero)
      slot0 = m.slot0;
    }
    const float *p0 = part + (size_t)slot0 * PART_STRIDE;
    tm_f4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int hd = ob0 + t;
      float M = -INFINITY;
      for (int s = 0; s < ns; ++s) M = fmaxf(M, p0[(size_t)s * PART_STRIDE + hd]);
      float L = 0.f;
      for (int s = 0; s < ns; ++s) {
        const float *ps = p0 + (size_t)s * PART_STRIDE;
        const float e = expf(ps[hd] - M);
        L += e * ps[8 + hd];
      }
      const float inv = 1.0f / L;
      tm_f4 b[8];
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4) b[s4] = tm_f4{0, 0, 0, 0};
      for (int s = 0; s < ns; ++s) {
        const float *ps = p0 + (size_t)s * PART_STRIDE;
        float wgt = expf(ps[hd] - M);
        wgt *= inv;
        const tm_f4 *pv = reinterpret_cast<const tm_f4 *>(ps + 16 + hd * 128 + q4);
        tm_f4 v[8];
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4) v[s4] = pv[4 * s4];
#pragma unroll
        for (int s4 = 0; s4 < 8; ++s4)
#pragma unroll
          for (int k = 0; k < 4; ++k) b[s4][k] = fmaf(wgt, v[s4][k], b[s4][k]);
      }
#pragma unroll
      for (int s4 = 0; s4 < 8; ++s4)
#pragma unroll
        for (int w = 0; w < 4; ++w)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(t ? F.a1[s4][w] : F.a0[s4][w], b[s4][w], acc[t], 0, 0, 0);
    }
    if (ok) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        tm_f4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int f = TM_FEAT(ob0 + t, i); r[i] = acc[t][i] + bv[f]; }
        *reinterpret_cast<tm_f4 *>(o + (size_t)tok * 128 + TM_FEAT(ob0 + t, 0)) = r;
      }
    }
  }
}

// ---- stages 2 and 4: out = LN(res + W in + bias); KH = 2: a 256-wide input as two chained halves (Wa, Wb) on one accumulator
template <int KH>
__global__ __launch_bounds__(TL_T) void k_tl_proj_ln(const float *__restrict__ in, const float *__restrict__ res, float *__restrict__ out, int n_tok,
                                                     const float *__restrict__ Wa, const float *__restrict__ Wb, const float *__restrict__ bias,
                                                     const float *__restrict__ g, const float *__restrict__ be) {
  constexpr int LDI = KH == 2 ? TM_LDT : TM_LDX;
  __shared__ __attribute__((aligned(16))) float it[TM_TOK * LDI], xs[TM_TOK * TM_LDX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ob0 = 2 * wave, tk = lane & 15;
  TmFrag Fa, Fb;
  tm_load(Fa, Wa, ob0, lane);
  if (KH == 2) tm_load(Fb, Wb, ob0, lane);
  const int ntiles = (n_tok + TM_TOK - 1) / TM_TOK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tok0 = tile * TM_TOK, nt = min(TM_TOK, n_tok - tok0);
    tl_tile_in<128 * KH>(it, LDI, in + (size_t)tok0 * 128 * KH, nt, tid);
    tl_tile_in<128>(xs, TM_LDX, res + (size_t)tok0 * 128, nt, tid);
    __syncthreads();
    tm_f4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    tm_mma<0>(acc, Fa, ob0, it + tk * LDI, 0, lane);
    if (KH == 2) tm_mma<0>(acc, Fb, ob0, it + tk * LDI + 128, 0, lane);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int f = TM_FEAT(ob0 + t, i); xs[tk * TM_LDX + f] += acc[t][i] + bias[f]; }
    __syncthreads();
    tm_layernorm(xs, TM_LDX, g, be, false, tid);
    __syncthreads();
    tl_tile_out(out + (size_t)tok0 * 128, xs, TM_LDX, nt, tid);
    __syncthreads();
  }
}

// ---- stages 3 and 5: up to three independent 128 x 128 projections of one input, blockIdx.y = which: out_y[tok][f] = W_y in (+ bias_y)
// (ReLU for the FFN's first matrix); out_y has row stride ld_y
struct TlProj {
  const float *W0, *W1, *W2, *b0, *b1, *b2;
  float *o0, *o1, *o2;
  int ld0, ld1, ld2, relu;
};
__global__ __launch_bounds__(TL_T) void k_tl_proj(const float *__restrict__ in, int n_tok, TlProj P) {
  __shared__ __attribute__((aligned(16))) float it[TM_TOK * TM_LDX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ob0 = 2 * wave, tk = lane & 15;
  const int y = blockIdx.y;
  const float *Wf = y == 0 ? P.W0 : (y == 1 ? P.W1 : P.W2);
  const float *bias = y == 0 ? P.b0 : (y == 1 ? P.b1 : P.b2);
  float *out = y == 0 ? P.o0 : (y == 1 ? P.o1 : P.o2);
  const int ld = y == 0 ? P.ld0 : (y == 1 ? P.ld1 : P.ld2);
  TmFrag F;
  tm_load(F, Wf, ob0, lane);
  float bv[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[t][i] = bias ? bias[TM_FEAT(ob0 + t, i)] : 0.f;
  const int ntiles = (n_tok + TM_TOK - 1) / TM_TOK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tok0 = tile * TM_TOK, nt = min(TM_TOK, n_tok - tok0);
    tl_tile_in<128>(it, TM_LDX, in + (size_t)tok0 * 128, nt, tid);
    __syncthreads();
    tm_f4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    tm_mma<0>(acc, F, ob0, it + tk * TM_LDX, 0, lane);
    if (tk < nt) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        tm_f4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = acc[t][i];
          if (bias) v = v + bv[t][i];           // (S has no bias: the accumulator as it is, -0 included)
          r[i] = P.relu ? fmaxf(v, 0.f) : v;
        }
        *reinterpret_cast<tm_f4 *>(out + (size_t)(tok0 + tk) * ld + TM_FEAT(ob0 + t, 0)) = r;
      }
    }
    __syncthreads();
  }
}

// ---- stage 6: qk[hd][f] = sum_d q[hd*16+d] W_k[hd*16+d][f] / 4: the sixteen fragments of this wave's two output blocks and eight
// heads stationary (64 VGPRs), four MFMAs per head and block; QK in the format of the pair kernel that reads it (mode & 16, mode & 32)
__global__ __launch_bounds__(TL_T) void k_tl_kq(const float *__restrict__ q, float *__restrict__ QK, int n_tok, int mode, const float *__restrict__ Wkf) {
  __shared__ __attribute__((aligned(16))) float qt[TM_TOK * TM_LDX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ob0 = 2 * wave, tk = lane & 15;
  const tm_f4 *Wk4 = reinterpret_cast<const tm_f4 *>(Wkf);
  tm_f4 A0[8], A1[8];
#pragma unroll
  for (int hd = 0; hd < 8; ++hd) { A0[hd] = Wk4[((size_t)hd * 8 + ob0) * 64 + lane]; A1[hd] = Wk4[((size_t)hd * 8 + ob0 + 1) * 64 + lane]; }
  const int ntiles = (n_tok + TM_TOK - 1) / TM_TOK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tok0 = tile * TM_TOK, nt = min(TM_TOK, n_tok - tok0);
    const bool tk_ok = tk < nt;
    tl_tile_in<128>(qt, TM_LDX, q + (size_t)tok0 * 128, nt, tid);
    __syncthreads();
#pragma unroll
    for (int hd = 0; hd < 8; ++hd) {
      const tm_f4 b = *reinterpret_cast<const tm_f4 *>(qt + tk * TM_LDX + hd * 16 + 4 * (lane >> 4));
      tm_f4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
      const tm_f4 a0 = A0[hd], a1 = A1[hd];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[w], b[w], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[w], b[w], acc[1], 0, 0, 0);
      }
      if (!tk_ok) continue;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int col = TM_FEAT(ob0 + t, i);
          const float v = acc[t][i] * 0.25f;
          if (mode & 16) {
            // k_token_mfma's hi / lo (/ third) parts in the A-operand order of the bf16 pair kernels
            const int g = col >> 5, qq = (col >> 2) & 3, ii = 4 * ((col >> 4) & 1) + (col & 3);
            const int idx = ((g * 32) + hd * 4 + qq) * 8 + ii;
            const u32 h = pk_bf16(v, v) & 0xffffu;
            const float r1 = v - bf_lo_f32(h);
            const u32 l = pk_bf16(r1, 0.f) & 0xffffu;
            unsigned short *qs = reinterpret_cast<unsigned short *>(QK + (size_t)(tok0 + tk) * ((mode & 32) ? 1536 : 1024));
            qs[idx] = (unsigned short)h;
            qs[1024 + idx] = (unsigned short)l;
            if (mode & 32) qs[2048 + idx] = (unsigned short)(pk_bf16(r1 - bf_lo_f32(l), 0.f) & 0xffffu);
          } else {
            QK[(size_t)(tok0 + tk) * 1024 + hd * 128 + col] = v;
          }
        }
    }
    __syncthreads();
  }
}

// -------------------------------------------------------------------------------------------------
// host side: the launch list of one token launch (mode) over a run of n_tokens tokens
// -------------------------------------------------------------------------------------------------
struct TlLaunch { int stage, gx, gy, block, lds, t0, n; };

static size_t tl_arena_bytes(int chunk) { return (size_t)chunk * TL_ROW * sizeof(float); }

// the mode sets the predictor issues: 1|4 (init), 2|4 (layers 0-4), 2|8 (last layer), each with the QK format bits 16 / 16|32
static bool tl_mode_ok(int mode) {
  const int m = mode & 15, q = mode & ~15;
  if (m != (1 | 4) && m != (2 | 4) && m != (2 | 8)) return false;
  return q == 0 || q == 16 || q == 48;
}

static int tl_stage_lds(int stage) {
  const int x = TM_TOK * TM_LDX * (int)sizeof(float), t = TM_TOK * TM_LDT * (int)sizeof(float);
  return stage == 0 ? 2 * x : stage == 1 ? 0 : stage == 2 ? 2 * x : stage == 4 ? t + x : x;
}

// per chunk the stages of `mode` in order (a chunk is finished before the next one starts: they share the arena)
static void tl_build_plan(int n_tokens, int mode, int chunk, int n_cu, std::vector<TlLaunch> &out) {
  out.clear();
  for (int t0 = 0; t0 < n_tokens; t0 += chunk) {
    const int n = n_tokens - t0 < chunk ? n_tokens - t0 : chunk;
    const int ntiles = (n + TM_TOK - 1) / TM_TOK;
    for (int s = 0; s < TL_NSTAGE; ++s) {
      const bool on = s == 0 ? (mode & 1) : s <= 4 ? (mode & 2) : (mode & 4);
      if (!on) continue;
      const int gy = s == 3 ? 2 : s == 5 ? 3 : 1;
      int cap = tl_wg_per_cu[s] * n_cu / gy;
      if (cap < 1) cap = 1;
      out.push_back({s, ntiles < cap ? ntiles : cap, gy, TL_T, tl_stage_lds(s), t0, n});
    }
  }
}

// one launch of the list; the pointers are the RUN's (token 0 of the run), arena = one chunk.  Returns < 0 for a stage without a kernel
static int tl_launch(const TlLaunch &L, hipStream_t s, int mode, const TokMeta *meta, const float *actor_feat, const float *lane_feat, float *x,
                     const float *part, float *ST, float *QK, size_t qk_stride, const TokWeights &W, const TokWeightsM &WM, float *arena, int chunk) {
  float *o = arena, *x1 = arena + (size_t)chunk * 128, *h = arena + (size_t)chunk * 256, *q = arena + (size_t)chunk * 512;
  const dim3 grid(L.gx, L.gy), block(L.block);
  const TokMeta *m_ = meta + L.t0;
  float *x_ = x + (size_t)L.t0 * 128, *ST_ = ST + (size_t)L.t0 * 256, *QK_ = QK + (size_t)L.t0 * qk_stride;
  switch (L.stage) {
    case 0: hipLaunchKernelGGL(k_tl_init, grid, block, 0, s, m_, L.n, actor_feat, lane_feat, x_, W, WM.Wpa, WM.Wpl); break;
    case 1: hipLaunchKernelGGL(k_tl_merge_v, grid, block, 0, s, m_, L.n, mode, part, o, WM.Wv, W.bv); break;
    case 2: hipLaunchKernelGGL(k_tl_proj_ln<1>, grid, block, 0, s, (const float *)o, (const float *)x_, x1, L.n, WM.Wo, WM.Wo, W.bo, W.g2, W.b2); break;
    case 3: {
      const TlProj P = {WM.W1a, WM.W1b, nullptr, W.b1, W.b1 + 128, nullptr, h, h + 128, nullptr, 256, 256, 0, 1};
      hipLaunchKernelGGL(k_tl_proj, grid, block, 0, s, (const float *)x1, L.n, P);
      break;
    }
    case 4: hipLaunchKernelGGL(k_tl_proj_ln<2>, grid, block, 0, s, (const float *)h, (const float *)x1, x_, L.n, WM.W2a, WM.W2b, W.bb2, W.g3, W.b3); break;
    case 5: {
      const TlProj P = {WM.Ws, WM.Wt, WM.Wq, nullptr, W.bm, W.bq, ST_, ST_ + 128, q, 256, 256, 128, 0};
      hipLaunchKernelGGL(k_tl_proj, grid, block, 0, s, (const float *)x_, L.n, P);
      break;
    }
    case 6: hipLaunchKernelGGL(k_tl_kq, grid, block, 0, s, (const float *)q, QK_, L.n, mode, WM.Wkf); break;
    default: return -1;
  }
  return 0;
}
