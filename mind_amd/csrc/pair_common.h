// What the RelaFusionLayer pair kernels share -- k_pair (fusion_kernels.hip), k_pair_bf (pair_bf16_kernels.hip), k_pair_t
// (pair_tile_kernels.hip), k_pair_t6 (pair_tile6_kernels.hip) -- and nothing launchable: types and lane geometry, the LDS layout and the
// helpers of the bf16 kernels, and one text per phase that the kernels run alike.  Each kernel file keeps its own GEMM, data movement,
// ablation switches and tile loop.
//
// The phase functions are inlined into kernels that sit at their register budget.  Scalars travel by value, arrays by reference
// (frag8 &, float (&)[4]), and no parameter is __restrict__: with these the kernels compile to the instructions they had with the text
// inline, up to register moves and wait counts (tools/asm_compare.py, profiles/pair_common_asm.txt, which also lists the one exception).
// A helper is simplified on its own before it is inlined, without what the kernel knows about its arguments (p < 16, q < 4, the
// alignment of `lds`): where that changed the address arithmetic the phase is a macro (PAIR_WAVE_LDS, PAIR_STORE_PARTIAL_DIRECT),
// takes ready-made pointers (pair_stage_quarter) or keeps the kernels' alignment by a typedef (pair_stage_tables); where it changed
// the BITS (which product of a*b + c*d is contracted into the fma) it is a macro too (PAIR_EDGE0).  Same mnemonics do not mean same
// bits: tests/test_gpu_pair_bits.py is the check for that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#include "weight_tables.h"   // u32, VT_*, TokWeights
#include "launch_clock.h"    // LcSlot, lc_stamp_in / lc_stamp_out: the kernels' last argument (null: not timed)

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u32 pk_bf16(float a, float b) {   // {bf16(a) in bits 0..15, bf16(b) in bits 16..31}, RNE
  f32x2_t v = {a, b};
  return __builtin_bit_cast(u32, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ float bf_lo_f32(u32 pk) { return __builtin_bit_cast(float, pk << 16); }
__device__ __forceinline__ float bf_hi_f32(u32 pk) { return __builtin_bit_cast(float, pk & 0xffff0000u); }

#define PART_STRIDE 1040  // 8 (m) + 8 (l) + 8*128 (sum p*mem)

struct PairJob {
  long long edge_base;  // first pair index of the scene's edge tensor (pairs, not floats); pair (i, j) lives at edge_base + j * N + i
  int N;                // tokens in scene (a + l + 1)
  int j;                // column (query token)
  int t0, t1;           // i-tile range [t0, t1), 32 rows each
  int tok_base;         // first token of the scene in the flat token arrays
  int slot;             // partial-result slot
  int flags;            // bit0: column is an actor or the cls token
  int scene;
  long long edge_base_t;  // the same for the tile-native layout of k_pair_t (pair_tile_kernels.hip): columns padded to whole 16-row tiles
};

// Eight waves (two per SIMD) share the two weight matrices: while one wave of a SIMD is in its LayerNorm / softmax /
// staging phases the other one keeps the MFMA busy.  Everything per-wave is sized so that the workgroup fits
// the 160 KB of LDS: the staging buffer holds a QUARTER tile (16 pairs x 32 features).
#define PAIR_WAVES 8
#define PAIR_THREADS (PAIR_WAVES * 64)
#define STAGE_FLOATS 512              // 16 rows x 8 chunks of 16 bytes

#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// Hide a value's provenance from the optimiser: address arithmetic derived from it is recomputed
// where it is used (cheap VALU) instead of being hoisted out of the tile loop as hundreds of
// loop-invariant VGPRs (LDS offsets > 64 KB do not fit the DS immediate field).
#define OPAQUE(x) asm volatile("" : "+v"(x))

// Lane geometry (16 pairs per tile, v_mfma_f32_16x16x4_f32):
//   p = lane & 15 : pair (row i = i0 + p of column j),  q = lane >> 4 : feature quarter
//   a lane holds 8 x f32x4: chunk blk (0..7) = features 16*blk + 4*q + (0..3)  == the MFMA C/D layout
//   (col = lane&15, row = 4*(lane>>4) + reg) of output block blk, and == the B operand of k-group
//   blk (k-slot (s, q) <-> feature 16*(s>>2) + 4*q + (s&3)).
typedef f32x4 frag8[8];

__device__ __forceinline__ float red_quad(float v) {  // sum over the 4 lanes of a pair
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float red_max16(float v) {
  v = fmaxf(v, __shfl_xor(v, 8, 64));
  v = fmaxf(v, __shfl_xor(v, 4, 64));
  v = fmaxf(v, __shfl_xor(v, 2, 64));
  v = fmaxf(v, __shfl_xor(v, 1, 64));
  return v;
}
__device__ __forceinline__ float red_sum16(float v) {
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

// LayerNorm over the 128 features of each pair (two-pass, biased variance, eps 1e-5).
__device__ __forceinline__ void ln_pairs(frag8 &a, const float *vtq, int off_g, int off_b, bool relu) {
  float s = 0.f;
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int w = 0; w < 4; ++w) s += a[b][w];
  s = red_quad(s);
  const float mean = s * (1.0f / 128.0f);
  float v = 0.f;
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float d = a[b][w] - mean;
      v = fmaf(d, d, v);
    }
  v = red_quad(v);
  const float rstd = 1.0f / sqrtf(v * (1.0f / 128.0f) + 1e-5f);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const f32x4 gm = *(const f32x4 *)(vtq + off_g + 16 * b);
    const f32x4 bt = *(const f32x4 *)(vtq + off_b + 16 * b);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float y = (a[b][w] - mean) * rstd * gm[w] + bt[w];
      if (relu) y = fmaxf(y, 0.f);
      a[b][w] = y;
    }
    if (b & 1) SCHED_FENCE();
  }
}

// swizzled float offset of 16-byte chunk c (0..7) in a 128-byte staging row r (0..15): the 16 lanes of a
// ds_read_b128 pass (rows 0..15, one chunk each) and of a ds_write_b128 pass (2 rows x 8 chunks) hit 16
// distinct 16-byte bank groups (the row-major kernels, k_pair and k_pair_bf)
__device__ __forceinline__ int sw_pos(int r, int c) { return (r * 8 + (c ^ ((r >> 1) & 7))) * 4; }

// phase timers of the row-major kernels (-DMIND_PAIR_TRACE: printed by workgroup 0)
#ifdef MIND_PAIR_TRACE
#define PT_DECL long long pt_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; long long pt_t = clock64();
#define PT_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define PT(i) do { long long n_ = clock64(); pt_[i] += n_ - pt_t; pt_t = n_; } while (0)
#else
#define PT_DECL
#define PT_DRAIN()
#define PT(i)
#endif

// ---- the bf16 kernels (k_pair_bf, k_pair_t, k_pair_t6): LDS layout, MFMA, operand split, two-way split GEMM, mean-free LayerNorm

// the staging buffers are private to a wave and one wave's DS instructions execute in order: no s_waitcnt between the passes
// over a buffer, only a compiler barrier (draining the LDS queue there measured no difference: DESIGN 4)
#define PBF_FENCE() asm volatile("" ::: "memory")

#define LB_WE 0                                       // [part 2][ob 8][g 4][lane 64][4 dwords] = 16384 dwords (64 KB)
#define LB_WP 16384
#define LB_STAGE 32768                                // 8 waves x 512 dwords
#define LB_PTAB (LB_STAGE + PAIR_WAVES * STAGE_FLOATS)   // 8 waves x 128: p[head 8][pair 16]
#define LB_SVEC (LB_PTAB + PAIR_WAVES * 128)          // 8 waves x 128: S[j]
#define LB_VT (LB_SVEC + PAIR_WAVES * 128)            // 896
#define LB_RT (LB_VT + VT_SIZE)                       // 1024 (layer 0)
#define LB_TOTAL (LB_RT + 1024)                       // 40832 dwords = 163328 bytes

#define PT_TILE_FLOATS 2048                           // a tile chunk of the tile-native edge tensor (k_pair_t, k_pair_t6): 16 pairs x 128 features

#define MFMA_BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0)

// split the lane's 8 chunks into the four k-groups' B operands: hi[g], lo[g] (lo only for NP == 3)
template <int NP>
__device__ __forceinline__ void split_frag(const frag8 &x, u32x4 (&hi)[4], u32x4 (&lo)[4]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const f32x4 v = x[2 * g + c];
      const u32 h0 = pk_bf16(v[0], v[1]), h1 = pk_bf16(v[2], v[3]);
      hi[g][2 * c] = h0;
      hi[g][2 * c + 1] = h1;
      if (NP == 3) {
        lo[g][2 * c] = pk_bf16(v[0] - bf_lo_f32(h0), v[1] - bf_hi_f32(h0));
        lo[g][2 * c + 1] = pk_bf16(v[2] - bf_lo_f32(h1), v[3] - bf_hi_f32(h1));
      }
    }
    SCHED_FENCE();
  }
}

// acc[ob] += sum_g W[ob][g] . B[g]   (W = hi + lo fragments in LDS at `wa`: [part][ob][g][lane][4 dwords]).
// Eight steps (g, output-block quad): per step 4 x NP MFMAs that rotate over four accumulators (dependent MFMAs are
// four issues apart); the hi fragments are double-buffered in registers, the lo fragments are reloaded for the next
// step as soon as the lo.hi products of this one are issued.
template <int NP>
__device__ __forceinline__ void gemm_bf(frag8 &acc, const u32 *wa, const u32x4 (&bhi)[4], const u32x4 (&blo)[4], int lane) {
  int lo_ = lane * 4;
  OPAQUE(lo_);
  const u32 *wl = wa + lo_;
  u32x4 ah[2][4], al[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ah[0][k] = *(const u32x4 *)(wl + ((k * 4 + 0) * 256));
    if (NP == 3) al[k] = *(const u32x4 *)(wl + 8192 + ((k * 4 + 0) * 256));
  }
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    const int g = st >> 1, o0 = (st & 1) * 4, cur = st & 1, nxt = cur ^ 1;
    const int gn = (st + 1) >> 1, on = ((st + 1) & 1) * 4;
#ifdef MIND_GEMM_NO_RELOAD      // (timing-only build of tools/micro/pair_bench: the weight fragments of the first step serve all eight)
#pragma unroll
    for (int k = 0; k < 4; ++k) { ah[nxt][k] = ah[cur][k]; asm volatile("" : "+v"(ah[nxt][k])); }
#else
    if (st < 7) {
#pragma unroll
      for (int k = 0; k < 4; ++k) ah[nxt][k] = *(const u32x4 *)(wl + (((on + k) * 4 + gn) * 256));
    }
#endif
    if (NP == 3) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[o0 + k] = MFMA_BF(al[k], bhi[g], acc[o0 + k]);
      SCHED_FENCE();
#ifndef MIND_GEMM_NO_RELOAD
      if (st < 7) {
#pragma unroll
        for (int k = 0; k < 4; ++k) al[k] = *(const u32x4 *)(wl + 8192 + (((on + k) * 4 + gn) * 256));
      }
#endif
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[o0 + k] = MFMA_BF(ah[cur][k], bhi[g], acc[o0 + k]);
    if (NP == 3) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[o0 + k] = MFMA_BF(ah[cur][k], blo[g], acc[o0 + k]);
    }
    SCHED_FENCE();
  }
}

// LayerNorm of a shift-free input (the mean was folded into the weights): y = x / sqrt(mean(x^2) + eps) * g + b
__device__ __forceinline__ void ln_nomean(frag8 &a, const float *vtq, int off_g, int off_b) {
  float v = 0.f;
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int w = 0; w < 4; ++w) v = fmaf(a[b][w], a[b][w], v);
  v = red_quad(v);
  const float rstd = 1.0f / sqrtf(v * (1.0f / 128.0f) + 1e-5f);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const f32x4 gm = *(const f32x4 *)(vtq + off_g + 16 * b);
    const f32x4 bt = *(const f32x4 *)(vtq + off_b + 16 * b);
#pragma unroll
    for (int w = 0; w < 4; ++w) a[b][w] = fmaxf(fmaf(a[b][w] * rstd, gm[w], bt[w]), 0.f);
    if (b & 1) SCHED_FENCE();
  }
}

// ================================================================================================================================
// Shared phases
// ================================================================================================================================

// Stage the two weight matrices (PER 16-byte loads per thread and matrix; the second one not under update_mode 2) and the vector / rpe
// tables into LDS at the given float offsets, once per workgroup.  All loads of a matrix are requested before the first LDS write (a
// load -> wait -> write loop costs 16 L2 round trips per workgroup, a quarter of a small launch).  Ends with the workgroup barrier.
// (The LDS writes keep the 4-byte alignment of the kernels' `extern __shared__ float lds[]`, which is what they had as text inside the kernels:
// pairs of 4-byte stores.  16-byte stores here are a change of the kernels' code, to be measured as one.)
typedef f32x4 lds_f32x4 __attribute__((aligned(4)));
template <int PER, int MODE>
__device__ __forceinline__ void pair_stage_tables(float *lds, int tid, const void *We, const void *Wp, const float *vtab, const float *rtab,
                                                  int update_mode, int o_we, int o_wp, int o_vt, int o_rt) {
  {
    f32x4 te[PER], tp[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) te[k] = ((const f32x4 *)We)[tid + k * PAIR_THREADS];
    if (update_mode != 2) {
#pragma unroll
      for (int k = 0; k < PER; ++k) tp[k] = ((const f32x4 *)Wp)[tid + k * PAIR_THREADS];
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) ((lds_f32x4 *)(lds + o_we))[tid + k * PAIR_THREADS] = te[k];
    if (update_mode != 2) {
#pragma unroll
      for (int k = 0; k < PER; ++k) ((lds_f32x4 *)(lds + o_wp))[tid + k * PAIR_THREADS] = tp[k];
    }
  }
  for (int i = tid; i < VT_SIZE; i += PAIR_THREADS) lds[o_vt + i] = vtab[i];
  if (MODE == 0)
    for (int i = tid; i < 1024; i += PAIR_THREADS) lds[o_rt + i] = rtab[i];
  __syncthreads();
}

// Layer 0: edge0 = ReLU(LN(W_r rpe + b_r)) of pair (IC, J_) into EF, zeros on the cls row / column (network.py:326-330).  The relative pose
// encoding comes from the scene's rpe tensor (RPE_PTRS) or from the two tokens' poses (PJ = pose of token J_, planners/mind/utils.py:193-242);
// RT = the rpe table in LDS at the lane's feature quarter (table + 32 q).
// A macro, not a function: a*b + c*d has two contractions into one fma, and inside an inlined function the compiler rounded the other product
// of the pose arithmetic -- the same instructions, registers and histogram, other bits in the last place (tests/test_gpu_pair_bits.py caught it).
#define PAIR_EDGE0(EF, RT, TOKPOS, RPE_PTRS, PJ, SCENE, TOK_BASE, J_, N_, IC)                                                                         \
  {                                                                                                                                                   \
    const float *rt = (RT);                                                                                                                           \
    float r5[5];                                                                                                                                      \
    const bool is_cls = ((IC) == (N_) - 1) || ((J_) == (N_) - 1);                                                                                     \
    if ((RPE_PTRS) != nullptr) {                                                                                                                      \
      const float *rp = (RPE_PTRS)[(SCENE)];                                                                                                          \
      const int n1 = (N_) - 1;                                                                                                                        \
      const size_t o = is_cls ? 0 : ((size_t)(IC) * n1 + (J_));                                                                                       \
      _Pragma("unroll") for (int k = 0; k < 5; ++k) r5[k] = rp[(size_t)k * n1 * n1 + o];                                                              \
    } else {                                                                                                                                          \
      const f32x4 ti = *(const f32x4 *)((TOKPOS) + (size_t)((TOK_BASE) + (IC)) * 4);                                                                  \
      const float dx = (PJ)[0] - ti[0], dy = (PJ)[1] - ti[1];                                                                                         \
      const float dist = sqrtf(dx * dx + dy * dy);                                                                                                    \
      const float nj = sqrtf((PJ)[2] * (PJ)[2] + (PJ)[3] * (PJ)[3]);                                                                                  \
      const float ni = sqrtf(ti[2] * ti[2] + ti[3] * ti[3]);                                                                                          \
      const float den1 = nj * ni + 1e-10f;                                                                                                            \
      const float den2 = nj * dist + 1e-10f;                                                                                                          \
      r5[0] = ((PJ)[2] * ti[2] + (PJ)[3] * ti[3]) / den1;                                                                                             \
      r5[1] = ((PJ)[2] * ti[3] - (PJ)[3] * ti[2]) / den1;                                                                                             \
      r5[2] = ((PJ)[2] * dx + (PJ)[3] * dy) / den2;                                                                                                   \
      r5[3] = ((PJ)[2] * dy - (PJ)[3] * dx) / den2;                                                                                                   \
      r5[4] = dist * 2.0f / 100.0f;                                                                                                                   \
    }                                                                                                                                                 \
    _Pragma("unroll") for (int b = 0; b < 8; ++b) {                                                                                                   \
      const float *c = rt + b * 128;                                                                                                                  \
      f32x4 acc = *(const f32x4 *)(c + 20);  /* bias */                                                                                               \
      _Pragma("unroll") for (int k = 0; k < 5; ++k) {                                                                                                 \
        const f32x4 wk = *(const f32x4 *)(c + 4 * k);                                                                                                 \
        _Pragma("unroll") for (int w = 0; w < 4; ++w) acc[w] = fmaf(wk[w], r5[k], acc[w]);                                                            \
      }                                                                                                                                               \
      (EF)[b] = acc;                                                                                                                                  \
    }                                                                                                                                                 \
    float s = 0.f;                                                                                                                                    \
    _Pragma("unroll") for (int b = 0; b < 8; ++b)                                                                                                     \
      _Pragma("unroll") for (int w = 0; w < 4; ++w) s += (EF)[b][w];                                                                                  \
    s = red_quad(s);                                                                                                                                  \
    const float mean = s * (1.0f / 128.0f);                                                                                                           \
    float v = 0.f;                                                                                                                                    \
    _Pragma("unroll") for (int b = 0; b < 8; ++b)                                                                                                     \
      _Pragma("unroll") for (int w = 0; w < 4; ++w) { const float d = (EF)[b][w] - mean; v = fmaf(d, d, v); }                                         \
    v = red_quad(v);                                                                                                                                  \
    const float rstd = 1.0f / sqrtf(v * (1.0f / 128.0f) + 1e-5f);                                                                                     \
    _Pragma("unroll") for (int b = 0; b < 8; ++b) {                                                                                                   \
      const float *c = rt + b * 128;                                                                                                                  \
      const f32x4 gm = *(const f32x4 *)(c + 24);                                                                                                      \
      const f32x4 bt = *(const f32x4 *)(c + 28);                                                                                                      \
      _Pragma("unroll") for (int w = 0; w < 4; ++w) {                                                                                                 \
        const float y = fmaxf(((EF)[b][w] - mean) * rstd * gm[w] + bt[w], 0.f);                                                                       \
        (EF)[b][w] = is_cls ? 0.f : y;                                                                                                                \
      }                                                                                                                                               \
    }                                                                                                                                                 \
  }

// A wave's pointers into the LB_* layout, and its indices into the transposed staging image of a 32-feature quarter of the memory
// tile: [feature 32][pair 16] dwords, the four pair-quads of a row XOR-swizzled so that both the ds_write_b32 pass and the
// ds_read_b128 pass are conflict-free
//   write (tw_base): lane (p, q) owns features 16 b2 + 4 q + r (quad code of those rows = q)
//   read  (tr_base): lane (n, q') fetches pairs 4 q' .. 4 q' + 3 of feature 16 b2 + n
// Declared into the kernel's scope by a macro: as a struct returned from a function, or with the two indices from functions of (p, q),
// the kernels' address set-up compiles to other instructions (the callee is simplified on its own before it is inlined).
#define PAIR_WAVE_LDS(lds, wave, p, q)                                                                                              \
  float *stage = (lds) + LB_STAGE + (wave) * STAGE_FLOATS;      /* transposition image of the sum_p_mem pass */                       \
  float *ptab = (lds) + LB_PTAB + (wave) * 128;                                                                                     \
  float *svec = (lds) + LB_SVEC + (wave) * 128;                                                                                     \
  const float *vt = (lds) + LB_VT;                                                                                                  \
  const u32 *wbe = (const u32 *)((lds) + LB_WE);                                                                                    \
  const u32 *wbp = (const u32 *)((lds) + LB_WP);                                                                                    \
  const int cq_w = (0x1320 >> (4 * (q))) & 3;                 /* c = [0, 2, 3, 1] */                                                  \
  const int cq_r = (0x1320 >> (4 * (((p) >> 2) & 3))) & 3;                                                                          \
  const int tw_base = (4 * (q)) * 16 + ((((p) >> 2) ^ cq_w) * 4) + ((p) & 3);                                                       \
  const int tr_base = (p) * 16 + (((q) ^ cq_r) * 4);                                                                                \
  u32 *stq_w = (u32 *)stage + tw_base;                                                                                              \
  const u32 *stq_r = (const u32 *)stage + tr_base;

// Online softmax over i, one tile: lanes of quarter q (and q ^ 2) own heads 4 (q & 1) .. + 3 of pair p; sa = the tile's scores.  Leaves
// the probabilities in ptab[head][pair] and rescales the running sum p.mem of this lane's heads (rows 4q..4q+3 of the accumulator
// blocks), skipped when no running maximum of the wave moved (wave-uniform branch).
__device__ __forceinline__ void pair_softmax_step(f32x4 sa, bool valid, int lq, int lp, float (&m_run)[4], float (&l_part)[4], frag8 &mbar,
                                                  float *ptab) {
  float pr[4], scl[4];
  bool grew = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float sv = valid ? sa[r] : -INFINITY;
    const float mx = red_max16(sv);
    const float m_new = fmaxf(m_run[r], mx);
    grew = grew || (m_new != m_run[r]);
    scl[r] = __expf(m_run[r] - m_new);
    pr[r] = valid ? __expf(sv - m_new) : 0.f;
    l_part[r] = l_part[r] * scl[r] + pr[r];
    m_run[r] = m_new;
  }
  PBF_FENCE();
  if (lq < 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ptab[(4 * lq + r) * 16 + lp] = pr[r];
  }
  if (__any(grew)) {
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) mbar[b][r] *= scl[r];
  }
  PBF_FENCE();
}

// One 32-feature quarter (= k-group) of the memory tile through the wave's transposition image: the lane's bf16 pairs X and Y go in as
// (X | Y << 16) dwords, k-slot (q', i) <-> (pair 4 q' + (i >> 1), part i & 1); f0 / f1 = the B operands of feature blocks 2 g, 2 g + 1
// (HAS_Y false: y is not read, the high halves are zero)
template <bool HAS_Y>
__device__ __forceinline__ void pair_stage_quarter(u32 *stq_w, const u32 *stq_r, const u32x4 &x, const u32x4 &y, u32x4 &f0, u32x4 &f1) {
#pragma unroll
  for (int b2 = 0; b2 < 2; ++b2)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const u32 X = x[2 * b2 + rr];
      const u32 Y = HAS_Y ? y[2 * b2 + rr] : 0u;
      stq_w[(16 * b2 + 2 * rr) * 16] = (X & 0xffffu) | (Y << 16);
      stq_w[(16 * b2 + 2 * rr + 1) * 16] = (X >> 16) | (Y & 0xffff0000u);
    }
  PBF_FENCE();
  f0 = *(const u32x4 *)(stq_r);
  f1 = *(const u32x4 *)(stq_r + 256);
  PBF_FENCE();
}

// Column partial m[8], l[8], mbar[8][128] to `po`, through the wave's idle LDS images so that it leaves as nine coalesced 16-byte stores per
// lane instead of forty 4-byte ones from half the lanes (in order behind the job's last LDS reads; a wave's LDS accesses keep their order)
__device__ __forceinline__ void pair_store_partial(float *po, float *stage, float *ptab, const float (&m_run)[4], const float (&l_part)[4],
                                                   const frag8 &mbar, int lane, int p, int q) {
  float lsum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) lsum[r] = red_sum16(l_part[r]);
  if (p == 0 && q < 2) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { ptab[4 * q + r] = m_run[r]; ptab[8 + 4 * q + r] = lsum[r]; }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {      // heads 4 h .. 4 h + 3 fill the 512-float transposition image
    if (q == h) {
#pragma unroll
      for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) stage[r * 128 + 16 * b + p] = mbar[b][r];
    }
    PBF_FENCE();
    const f32x4 v0 = *(const f32x4 *)(stage + lane * 4), v1 = *(const f32x4 *)(stage + 256 + lane * 4);
    *(f32x4 *)(po + 16 + h * 512 + lane * 4) = v0;
    *(f32x4 *)(po + 16 + h * 512 + 256 + lane * 4) = v1;
    PBF_FENCE();
  }
  if (lane < 4) *(f32x4 *)(po + lane * 4) = *(const f32x4 *)(ptab + lane * 4);
  PBF_FENCE();
}

// The same partial stored straight from the registers (k_pair_bf; k_pair_t's timing switch).  A macro: as a function, k_pair_bf's address
// arithmetic compiles to other instructions (the callee is simplified on its own, without the ranges of p and q, before it is inlined).
#define PAIR_STORE_PARTIAL_DIRECT(po, m_run, l_part, mbar, p, q)                                                                    \
  {                                                                                                                                 \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                                 \
      const float l = red_sum16((l_part)[r]);                                                                                       \
      if ((p) == 0 && (q) < 2) { (po)[4 * (q) + r] = (m_run)[r]; (po)[8 + 4 * (q) + r] = l; }                                       \
    }                                                                                                                               \
    if ((q) < 2) {                                                                                                                  \
      _Pragma("unroll") for (int b = 0; b < 8; ++b)                                                                                 \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) (po)[16 + (4 * (q) + r) * 128 + 16 * b + (p)] = (mbar)[b][r];                 \
    }                                                                                                                               \
  }

// Job walk of the tile-native kernels: the wave's record is read one job ahead (a scalar load and its latency per job otherwise).  J = this
// job, Jn = the wave's next one (Jc for the next call), has_next = there is one and it is not a padding job; false for a padding job (pair_jobs.h)
__device__ __forceinline__ bool pair_job_next(const PairJob *jobs, int n_jobs, int job, int stride, PairJob &Jc, PairJob &J, PairJob &Jn, bool &has_next) {
  J = Jc;
  const int jn = job + stride;
  const bool in_range = jn < n_jobs;
  Jn = jobs[in_range ? jn : job];
  Jc = Jn;
  has_next = in_range && Jn.t1 > Jn.t0;
  return J.t1 > J.t0;
}
// first float of column j of a scene's tile-native edge tensor: columns padded to whole 16-row tiles, 2^ESH dwords per pair
template <int ESH>
__device__ __forceinline__ float *pair_tile_col(float *edge, long long edge_base_t, int j, int N) {
  return edge + (((size_t)edge_base_t + (size_t)j * (((N + 15) >> 4) * 16)) << ESH);
}
