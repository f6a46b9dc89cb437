// Layer-wise batched ActorNet: the arithmetic of k_actor_mfma<NP> (actor_mfma_kernels.hip), spread over one launch per layer and
// chunk of actors instead of one workgroup per actor -- for rounds of thousands of actors, where every actor's workgroup pulling the
// complete 9.1 MB of weight fragments through its CU's L2 port is what the per-actor kernel spends its time on.
//
// Every Conv1d is the same GEMM  out[co][col] = sum_k Wm[co][k] X[k][col]  with the columns running over (actor, t) of a chunk:
//   * k_lw_conv<NP, LGC, KSZ, STRIDE, MT>: WEIGHT-STATIONARY.  Workgroup (x, y) copies the fragments of the MT m-tiles MT y .. MT y + MT - 1
//     (WeightTables::actorB, the pack_conv_frag layout, untouched: [m-tile][k-step][hi / mid / lo][lane][4]) into LDS once and its 16 waves
//     sweep 16-column tiles past them.  MT = 4 where the layer has >= 128 output channels and 4 .. 12 k-steps (four m-tiles fit: 4 x 12 x
//     3 KB = 144 KB; below four k-steps the k loop is fully unrolled and the fragments of four m-tiles, hoisted out of the tile loop, would
//     spill), MT = 2 otherwise (the 256-input-channel layers: 2 x 24 x 3 KB = 144 KB): a column block is fetched Cout / (16 MT)
//     times, the layer's fragments once per column block (grid x).  The B operand is the
//     split image of the previous stage in the scratch arena, in the LDS row format of k_actor_mfma (time-major rows of three bf16
//     planes, AM_RSD(C) dwords): the eight k-slots of a lane are one 16-byte load per plane, used for every m-tile.  A column is
//     (actor a = col / Tout, t = col % Tout): rows outside [0, Tin) of the column's OWN actor are zeros, so tiles that hold several
//     actors (T = 12, 6) never see a neighbour's samples.  Per output element the k-step order and the two accumulator chains (acc,
//     corr, summed at the end) are am_conv's: the raw fp32 outputs, written [t][Cout] per actor, are the bits k_actor_mfma<NP> holds
//     in its accumulators.
//   * k_lw_gn<NP>: one workgroup of 16 waves per actor loads those raw outputs into the accumulator registers in am_conv's
//     thread-to-element mapping and calls am_gn itself (same block sums: wave sum, then the 16 waves in order; same mean / centred
//     variance / affine / residual / x2 upsample / ReLU expressions), with its outputs pointed at the arena (next split image or fp32
//     FPN level) or, for the last stage, at actor_feat.  No atomics, no reduction whose order depends on the grid.
//   * k_lw_split: the input [A, 14, 48] -> the padded 16-channel split image, the prologue of k_actor_mfma.
// Same file-level compile settings as actor_mfma_kernels.hip (both are included into mind_hip.hip): the path is bit-identical to
// k_actor_mfma<NP> by construction, for every chunk size and grid.
//
// Arena: per actor the LDS carve of k_actor_mfma (AM_XIN .. AM_RED: 28 224 dwords, with the same aliasing of dead buffers) plus one raw
// conv output (128 x 48 fp32), LW_STRIDE = 34 368 dwords = 137 472 bytes; LW_CHUNK = 1024 actors per chunk = 134.25 MiB, allocated at first
// use, independent of A.  A stage touches its input image, the raw buffer and its output image only (<= 100 KB per actor, <= 98 MiB per
// chunk at the 128 x 48 stages, 20-45 MiB at the others), which with the 9.1 MB of fragments stays inside the 256 MiB Infinity Cache.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#define LW_T 1024
#define LW_WAVES 16
#define LW_RAW AM_RED                        // raw conv output of the current stage: [Tout][Cout] fp32
#define LW_STRIDE (AM_RED + 128 * 48)        // dwords per actor
#define LW_CHUNK 1024                        // actors per chunk (default)
#define LW_CONV_WGS 512                      // conv grids are capped near two workgroups per CU; a workgroup's waves loop over its tiles
#define LW_NSTAGE 26

template <int NP, int LGC, int KSZ, int STRIDE, int LW_MT /*m-tiles (16 output channels each) per workgroup*/>
__global__ __launch_bounds__(LW_T) void k_lw_conv(u32 *__restrict__ arena, int n_actors, int in_off, int Tin, const u32 *__restrict__ Wf,
                                                  int Cout, int Tout) {
  constexpr int CP = 1 << LGC, RSD = AM_RSD(CP), PLANE = CP / 2, PAD = (KSZ - 1) / 2;
  constexpr int KS = (KSZ * CP + 31) / 32;
  constexpr int NPART = NP == 6 ? 3 : (NP == 3 ? 2 : 1);
  extern __shared__ __attribute__((aligned(16))) u32 lw_sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int mt0 = blockIdx.y * LW_MT;
  // the fragments of this workgroup's m-tiles (contiguous in the packed array), the parts this arithmetic reads
  {
    const u32x4 *src = (const u32x4 *)(Wf + (size_t)mt0 * KS * 768);
    u32x4 *dst = (u32x4 *)lw_sm;
    for (int i = tid; i < LW_MT * KS * 192; i += LW_T)
      if ((i >> 6) % 3 < NPART) dst[i] = src[i];
  }
  __syncthreads();
  const int ncols = n_actors * Tout;
  const int ntiles = (ncols + 15) >> 4;
  for (int nt = blockIdx.x * LW_WAVES + wave; nt < ntiles; nt += gridDim.x * LW_WAVES) {
    const int col = nt * 16 + r;
    const bool valid = col < ncols;
    const int a = valid ? col / Tout : 0;
    const int t = col - a * Tout;
    const u32 *in = arena + (size_t)a * LW_STRIDE + in_off;
    f32x4 acc[LW_MT], corr[LW_MT];
#pragma unroll
    for (int m = 0; m < LW_MT; ++m) { acc[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; corr[m] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    // (unrolled by two only: the fragment loads do not depend on the tile, and a fully unrolled k loop has them all hoisted into registers)
#pragma unroll 2
    for (int ks = 0; ks < KS; ++ks) {
      const int k0 = ks * 32 + q * 8;
      const int dk = k0 >> LGC, ci = k0 & (CP - 1);
      const int row = t * STRIDE + dk - PAD;
      u32x4 bh = {0u, 0u, 0u, 0u}, bm = {0u, 0u, 0u, 0u}, bl = {0u, 0u, 0u, 0u};
      if (dk < KSZ && valid && row >= 0 && row < Tin) {
        const u32 *bp = in + row * RSD + (ci >> 1);
        bh = *(const u32x4 *)bp;
        if (NP >= 3) bm = *(const u32x4 *)(bp + PLANE);
        if (NP == 6) bl = *(const u32x4 *)(bp + 2 * PLANE);
      }
#pragma unroll
      for (int m = 0; m < LW_MT; ++m) {
        const u32 *wp = lw_sm + (size_t)(m * KS + ks) * 768 + lane * 4;
        const u32x4 ah = *(const u32x4 *)wp;
        u32x4 am, al;
        if (NP >= 3) am = *(const u32x4 *)(wp + 256);
        if (NP == 6) al = *(const u32x4 *)(wp + 512);
        // (the MFMA sequence of am_conv, per m-tile)
        acc[m] = MFMA_BF(ah, bh, acc[m]);
        if (NP >= 3) {
          if (NP == 6) {
            corr[m] = MFMA_BF(al, bh, corr[m]);
            corr[m] = MFMA_BF(ah, bl, corr[m]);
            corr[m] = MFMA_BF(am, bm, corr[m]);
          }
          corr[m] = MFMA_BF(am, bh, corr[m]);
          corr[m] = MFMA_BF(ah, bm, corr[m]);
        }
      }
    }
    if (valid) {
      float *raw = (float *)(arena + (size_t)a * LW_STRIDE + LW_RAW) + t * Cout + q * 4;
#pragma unroll
      for (int m = 0; m < LW_MT; ++m) {
        if (NP >= 3) acc[m] += corr[m];
        *(f32x4 *)(raw + (mt0 + m) * 16) = acc[m];
      }
    }
  }
}

// GroupNorm + epilogue of one stage, one actor per workgroup: am_gn on the raw conv outputs of the arena.  *_off: dword offsets in the
// actor's arena block, < 0 = absent; gout: actor_feat row of the chunk's first actor (last stage only)
template <int NP>
__global__ __launch_bounds__(AM_T) void k_lw_gn(u32 *__restrict__ arena, int n_actors, int Cout, int Tout, const float *__restrict__ g,
                                                const float *__restrict__ b, int resid_off, int up_off, int relu, int outs_off, int outf_off,
                                                float *__restrict__ gout) {
  __shared__ float red[64];
  const int a = blockIdx.x;
  if (a >= n_actors) return;
  u32 *base = arena + (size_t)a * LW_STRIDE;
  const float *raw = (const float *)(base + LW_RAW);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int ntt = (Tout + 15) >> 4;
  const int tiles = (Cout >> 4) * ntt;
  f32x4 acc[AM_MAXT];
#pragma unroll
  for (int i = 0; i < AM_MAXT; ++i) {
    acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int ti = wave + AM_WAVES * i;
    if (ti >= tiles) continue;
    const int mt = ti / ntt, nt = ti - mt * ntt;
    const int t = nt * 16 + r;
    if (t < Tout) acc[i] = *(const f32x4 *)(raw + t * Cout + mt * 16 + q * 4);
  }
  am_gn<NP>(acc, Cout, Tout, g, b, resid_off >= 0 ? base + resid_off : nullptr, up_off >= 0 ? (const float *)(base + up_off) : nullptr, relu != 0,
            outs_off >= 0 ? base + outs_off : nullptr, outf_off >= 0 ? (float *)(base + outf_off) : nullptr,
            gout ? gout + (size_t)a * 128 : nullptr, red);
}

// input [14][48] of every actor of the chunk -> split image [48] x AM_RSD(16), channels 14, 15 zero (the prologue of k_actor_mfma)
__global__ __launch_bounds__(384) void k_lw_split(const float *__restrict__ actors, int n_actors, u32 *__restrict__ arena) {
  const int a = blockIdx.x, tid = threadIdx.x;
  if (a >= n_actors) return;
  const int t = tid >> 3, c = (tid & 7) * 2;
  const float v0 = c < 14 ? actors[((size_t)a * 14 + c) * 48 + t] : 0.f;
  const float v1 = c + 1 < 14 ? actors[((size_t)a * 14 + c + 1) * 48 + t] : 0.f;
  u32 *p = arena + (size_t)a * LW_STRIDE + AM_XIN + t * AM_RSD(16) + (c >> 1);
  const u32 h = pk_bf16(v0, v1);
  const float r0 = v0 - bf_lo_f32(h), r1 = v1 - bf_hi_f32(h);
  const u32 m = pk_bf16(r0, r1);
  p[0] = h; p[8] = m; p[16] = pk_bf16(r0 - bf_lo_f32(m), r1 - bf_hi_f32(m));
}

// -------------------------------------------------------------------------------------------------
// host side: the 26 stages, the launch list of a call, the launches
// -------------------------------------------------------------------------------------------------
struct LwStage {
  int lgci, cin, cout, ksz, stride, tin, tout;     // the convolution (cin: real input channels; 1 << lgci: padded)
  int in_off;                                      // its input split image
  int wsel;                                        // weights: 4 * Res1d index + (0 c1, 1 ds, 2 c2), or 100 + lateral index
  int resid_off, up_off, relu, outs_off, outf_off, final;   // the GroupNorm epilogue (offsets < 0: absent)
};

static void lw_stages(LwStage *S) {
  const int O0 = AM_O0, O1 = O0 + AM_BUF, O2 = O1 + AM_BUF, O3 = O2 + AM_BUF, TA = O3 + AM_BUF, TB = TA + AM_BUF, TC = TB + AM_BUF;
  int n = 0;
  auto res = [&](int idx, int lgci, int cin, int lgco, int stride, bool ds, int in, int tin, int out) {
    const int cout = 1 << lgco, tout = tin / stride;
    S[n++] = {lgci, cin, cout, 3, stride, tin, tout, in, 4 * idx + 0, -1, -1, 1, TB, -1, 0};
    if (ds) S[n++] = {lgci, cin, cout, 1, stride, tin, tout, in, 4 * idx + 1, -1, -1, 0, TC, -1, 0};
    S[n++] = {lgco, cout, cout, 3, 1, tout, tout, TB, 4 * idx + 2, ds ? TC : in, -1, 1, out, -1, 0};
  };
  res(0, 4, 14, 5, 1, true, AM_XIN, 48, TA);
  res(1, 5, 32, 5, 1, false, TA, 48, O0);
  res(2, 5, 32, 6, 2, true, O0, 48, TA);
  res(3, 6, 64, 6, 1, false, TA, 24, O1);
  res(4, 6, 64, 7, 2, true, O1, 24, TA);
  res(5, 7, 128, 7, 1, false, TA, 12, O2);
  res(6, 7, 128, 8, 2, true, O2, 12, TA);
  res(7, 8, 256, 8, 1, false, TA, 6, O3);
  // FPN top-down: fp32 levels 3 -> TA, 2 -> TB, 1 -> O2..O3 (dead by then), level 0 -> FA as a split image
  S[n++] = {8, 256, 128, 3, 1, 6, 6, O3, 103, -1, -1, 0, -1, TA, 0};
  S[n++] = {7, 128, 128, 3, 1, 12, 12, O2, 102, -1, TA, 0, -1, TB, 0};
  S[n++] = {6, 64, 128, 3, 1, 24, 24, O1, 101, -1, TB, 0, -1, O2, 0};
  S[n++] = {5, 32, 128, 3, 1, 48, 48, O0, 100, -1, O2, 0, AM_FA, -1, 0};
  // output Res1d(128, 128) at T = 48: conv1's output in O0..O3 (dead), the last time column of conv2's to actor_feat
  S[n++] = {7, 128, 128, 3, 1, 48, 48, AM_FA, 4 * 8 + 0, -1, -1, 1, O0, -1, 0};
  S[n++] = {7, 128, 128, 3, 1, 48, 48, O0, 4 * 8 + 2, AM_FA, -1, 1, -1, -1, 1};
}

// m-tiles per conv workgroup (the blocking per stage, see the header)
static int lw_stage_mt(const LwStage &st) {
  const int ks = (st.ksz * (1 << st.lgci) + 31) / 32;
  return (st.cout >= 128 && ks >= 4 && ks <= 12) ? 4 : 2;
}

struct LwLaunch { int stage, kind /*0 split, 1 conv, 2 GroupNorm*/, gx, gy, block, lds, a0, n; };

static size_t lw_arena_bytes(int chunk) { return (size_t)chunk * LW_STRIDE * sizeof(u32); }

// the launches of one call, in issue order: per chunk the split, then conv + GroupNorm of the 26 stages
static void lw_build_plan(int n_actors, int chunk, std::vector<LwLaunch> &out) {
  LwStage S[LW_NSTAGE];
  lw_stages(S);
  out.clear();
  for (int a0 = 0; a0 < n_actors; a0 += chunk) {
    const int n = n_actors - a0 < chunk ? n_actors - a0 : chunk;
    out.push_back({-1, 0, n, 1, 384, 0, a0, n});
    for (int s = 0; s < LW_NSTAGE; ++s) {
      const LwStage &st = S[s];
      const int ks = (st.ksz * (1 << st.lgci) + 31) / 32;
      const int mt = lw_stage_mt(st);
      const int gy = (st.cout / 16) / mt;
      const int ntiles = (n * st.tout + 15) / 16;
      int gx = (ntiles + LW_WAVES - 1) / LW_WAVES;
      const int cap = LW_CONV_WGS / gy > 1 ? LW_CONV_WGS / gy : 1;
      if (gx > cap) gx = cap;
      out.push_back({s, 1, gx, gy, LW_T, mt * ks * 768 * (int)sizeof(u32), a0, n});
      out.push_back({s, 2, n, 1, AM_T, 0, a0, n});
    }
  }
}

// (LGC, KSZ, STRIDE, MT) of the 26 stages
#define LW_FOR_CONVS(X, NPV)                                                                                                        \
  X(NPV, 4, 3, 1, 2) X(NPV, 4, 1, 1, 2) X(NPV, 5, 3, 1, 2) X(NPV, 5, 3, 2, 2) X(NPV, 5, 1, 2, 2) X(NPV, 6, 3, 1, 2)  \
  X(NPV, 6, 3, 1, 4) X(NPV, 6, 3, 2, 4) X(NPV, 6, 1, 2, 2) X(NPV, 7, 3, 1, 4) X(NPV, 7, 3, 2, 4) X(NPV, 7, 1, 2, 4) X(NPV, 8, 3, 1, 2)

// the conv kernels' LDS (up to 144 KB) needs the attribute once per process and device
static void lw_set_attributes() {
#define LW_ATTR(NPV, LGC, KSZ, STR, MT)                                                                                                  \
  (void)hipFuncSetAttribute((const void *)k_lw_conv<NPV, LGC, KSZ, STR, MT>, hipFuncAttributeMaxDynamicSharedMemorySize,                  \
                            MT * ((KSZ * (1 << LGC) + 31) / 32) * 768 * (int)sizeof(u32));
  LW_FOR_CONVS(LW_ATTR, 6)
  LW_FOR_CONVS(LW_ATTR, 3)
  LW_FOR_CONVS(LW_ATTR, 1)
#undef LW_ATTR
}

template <int NP>
static int lw_launch_conv(const LwLaunch &L, const LwStage &st, hipStream_t s, u32 *arena, const u32 *Wf) {
#define LW_CASE(NPV, LGC, KSZ, STR, MT)                                                                                                    \
  if (st.lgci == LGC && st.ksz == KSZ && st.stride == STR && lw_stage_mt(st) == MT) {                                                      \
    hipLaunchKernelGGL((k_lw_conv<NPV, LGC, KSZ, STR, MT>), dim3(L.gx, L.gy), dim3(L.block), (size_t)L.lds, s, arena, L.n, st.in_off, st.tin, Wf, \
                       st.cout, st.tout);                                                                                                  \
    return 0;                                                                                                                              \
  }
  LW_FOR_CONVS(LW_CASE, NP)
#undef LW_CASE
  return -1;      // a stage without a kernel: an error, never another path
}

// every launch of the list on stream s; actors [A,14,48] and out [A,128] are the call's.  Returns the number of launches, < 0 on a stage
// without an instantiation
template <int NP>
static int lw_run(const std::vector<LwLaunch> &plan, hipStream_t s, u32 *arena, const float *actors, float *out, const AmW &W) {
  LwStage S[LW_NSTAGE];
  lw_stages(S);
  for (const LwLaunch &L : plan) {
    if (L.kind == 0) {
      hipLaunchKernelGGL(k_lw_split, dim3(L.gx), dim3(L.block), 0, s, actors + (size_t)L.a0 * 14 * 48, L.n, arena);
      continue;
    }
    const LwStage &st = S[L.stage];
    const u32 *Wf;
    const float *g, *b;
    if (st.wsel >= 100) {
      const AmLat &l = W.lat[st.wsel - 100];
      Wf = l.w; g = l.g; b = l.b;
    } else {
      const AmRes &R = W.res[st.wsel >> 2];
      const int which = st.wsel & 3;
      Wf = which == 0 ? R.c1 : (which == 1 ? R.ds : R.c2);
      g = which == 0 ? R.g1 : (which == 1 ? R.gd : R.g2);
      b = which == 0 ? R.b1 : (which == 1 ? R.bd : R.b2);
    }
    if (L.kind == 1) {
      if (lw_launch_conv<NP>(L, st, s, arena, Wf)) return -1;
    } else {
      hipLaunchKernelGGL(k_lw_gn<NP>, dim3(L.gx), dim3(L.block), 0, s, arena, L.n, st.cout, st.tout, g, b, st.resid_off, st.up_off, st.relu,
                         st.outs_off, st.outf_off, st.final ? out + (size_t)L.a0 * 128 : (float *)nullptr);
    }
  }
  return (int)plan.size();
}
