// RelaFusionLayer pair kernel on the bf16 MFMA (v_mfma_f32_16x16x32_bf16), fp32-accurate by operand splitting.
//
// Reference semantics: planners/mind/networks/network.py:165-232 (same math as k_pair in fusion_kernels.hip, whose
// algebraic folds -- rank-decomposed proj_memory, K projection folded into the query, V projection folded out of the
// sum -- are kept; the LDS layout LB_*, split_frag, gemm_bf, ln_nomean and the phases shared with the tile-native kernels live in
// pair_common.h).  What changes is the arithmetic of every contraction:
//
//   NP == 3 ("bf16x3"): both operands of a product are split into bf16 hi + lo parts (x = hi + lo + O(2^-17 |x|)) and
//       the three significant partial products hi.hi + hi.lo + lo.hi are accumulated in fp32 on the bf16 MFMA:
//       3 MFMAs of 16 cycles instead of 8 fp32 MFMAs of 32 cycles for the same 16x16x32 block = 5.3 x the fp32-MFMA
//       rate at ~2^-17 relative error per product (measured against the oracle: tests/test_gpu_predictor.py,
//       emulated on the CPU in tests/diag/bf16_split_emulation.py: 7e-6 m on `reg` vs 3e-6 for fp32 itself).
//   NP == 1 ("bf16"): hi parts only (plain bf16 operands, fp32 accumulate): the "stress" arithmetic of BASELINE
//       config 5; misses the 1e-3 m parity bar (3.7e-3 m, same emulation) and is therefore never the default.
//
// Layout algebra (16 pairs per tile, pair p = lane & 15, q = lane >> 4):
//   * a lane holds a pair's 128 features as 8 x f32x4: chunk blk = features 16 blk + 4 q + (0..3) = the MFMA C/D
//     layout (col = lane & 15, row = 4 (lane >> 4) + reg) of output block blk.
//   * B operand of k-group g (32 k-slots; a lane supplies slots 8 q .. 8 q + 7): slot (q, i) <-> feature
//     16 (2 g + (i >> 2)) + 4 q + (i & 3), i.e. chunks 2 g and 2 g + 1 of the lane, packed to bf16 pairs.  The weight
//     fragments are stored in the same slot order (pack_bfrag, mind_hip.hip), so the C/D layout of one GEMM is the B
//     layout of the next: edge -> memory -> proj_edge chain through registers.
//   * LayerNorm means are folded into the weights on the host ((I - 11^T/128) W: LayerNorm is invariant to a shift
//     along the features), so LN1 / LN2 only need the sum of squares.
//   * sum_i p_i mem_i runs on the MFMA too: the memory tile is transposed through LDS as (hi, lo) bf16 pairs, k-slot
//     (q', i) <-> (pair 4 q' + (i >> 1), part i & 1), and contracted with the duplicated probabilities
//     A[head][slot] = p[head][pair]; rows 8..15 of the 16-row A operand are zero (8 heads).
//   * the edge tensor is stored [scene][j][i][128]: a column job streams contiguous memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pair_common.h"   // LDS layout LB_*, MFMA_BF, split_frag, gemm_bf, ln_nomean, the phases shared with the other pair kernels

// tuning switches (A/B-measured on the MI355X): where the next tile's edge rows and this tile's folded query
// are requested
#ifndef PBF_PREFETCH_TOP
#define PBF_PREFETCH_TOP 0      // 1: next tile's edge rows requested right after this tile's rows left the load registers (measured: no difference)
#endif
#ifndef PBF_QK_FIRST
#define PBF_QK_FIRST 1
#endif

// MODE 0: layer 0, edge built in-kernel from the relative pose encoding; MODE 1: layers 1..5, edge read from HBM.
// update_mode as in k_pair.
template <int MODE, int NP>
__global__ __launch_bounds__(PAIR_THREADS, 1) void k_pair_bf(const PairJob *__restrict__ jobs, int n_jobs, float *__restrict__ edge,
                                                             const float *__restrict__ ST, const float *__restrict__ QK,
                                                             float *__restrict__ part, const u32 *__restrict__ WBe,
                                                             const u32 *__restrict__ WBp, const float *__restrict__ vtab,
                                                             const float *__restrict__ rtab, const float *__restrict__ tokpos,
                                                             const float *const *__restrict__ rpe_ptrs, int update_mode, LcSlot *clk) {
  lc_stamp_in(clk);
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int p = lane & 15;
  const int q = lane >> 4;

  pair_stage_tables<(NP == 3 ? 4096 : 2048) / PAIR_THREADS, MODE>(lds, tid, WBe, WBp, vtab, rtab, update_mode, LB_WE, LB_WP, LB_VT, LB_RT);      // (the lo halves are only needed by the split arithmetic)
  PAIR_WAVE_LDS(lds, wave, p, q)
  PT_DECL

  for (int job = wave * gridDim.x + blockIdx.x; job < n_jobs; job += gridDim.x * PAIR_WAVES) {
    const PairJob J = jobs[job];
    if (update_mode == 2 && !(J.flags & 1)) continue;
    if (J.t1 <= J.t0) continue;                  // padding job of the XCD-aware order
    const bool do_update = (update_mode == 0) || (update_mode == 1 && (J.flags & 1));
    const int N = J.N;
    const int j = J.j;
    float *ecol = edge + (((size_t)J.edge_base + (size_t)j * N) << 7);      // this column's pairs are contiguous: [i][128]
    PBF_FENCE();
    if (lane < 32) *(f32x4 *)(svec + lane * 4) = *(const f32x4 *)(ST + (size_t)(J.tok_base + j) * 256 + lane * 4);
    float m_run[4], l_part[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { m_run[k] = -INFINITY; l_part[k] = 0.f; }
    // A operand of the folded query (W_k^T q / 4), written by k_token as bf16 hi / lo fragments: row = head (8 used of
    // 16), k-slot order of the B operand; fetched per tile right before the scores (it would cost 32 registers to keep)
    const u32 *qs = (const u32 *)(QK + (size_t)(J.tok_base + j) * 1024) + ((lane & 7) * 4 + q) * 4;
    const bool qrow = (lane & 15) < 8;
    frag8 mbar;      // [blk][r]: head 4 q + r (q < 2), feature 16 blk + p
#pragma unroll
    for (int b = 0; b < 8; ++b) mbar[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float pj[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 0) {
      const f32x4 t = *(const f32x4 *)(tokpos + (size_t)(J.tok_base + j) * 4);
      pj[0] = t[0]; pj[1] = t[1]; pj[2] = t[2]; pj[3] = t[3];
    }
    // first edge tile of the job (later ones are requested one tile ahead)
    f32x4 raw[8];
#define PBF_LOAD_RAW(ROW0, LANEV)                                                                       \
  _Pragma("unroll") for (int qt = 0; qt < 4; ++qt) _Pragma("unroll") for (int n = 0; n < 2; ++n) {     \
    int irow = (ROW0) + 8 * n + ((LANEV) >> 3);                                                         \
    irow = irow < N ? irow : N - 1;                                                                     \
    raw[2 * qt + n] = *(const f32x4 *)(ecol + ((size_t)irow << 7) + qt * 32 + ((LANEV)&7) * 4);        \
  }
    if (MODE == 1) { PBF_LOAD_RAW(J.t0 * 16, lane) }
    PBF_FENCE();

    for (int tile = J.t0; tile < J.t1; ++tile) {
      const int i0 = tile * 16;
      int lq = q, lp = p, ll = lane;
      OPAQUE(lq); OPAQUE(lp); OPAQUE(ll);
      const float *vtq = vt + lq * 4;
      const int i = i0 + p;
      const bool valid = i < N;
      const int ic = valid ? i : (N - 1);
      // accumulator of the first GEMM starts from T[i] (+ S[j] below): requested now, consumed after the edge staging
      frag8 mem;
      {
        const float *Ti = ST + (size_t)(J.tok_base + ic) * 256 + 128 + lq * 4;
#pragma unroll
        for (int b = 0; b < 8; ++b) mem[b] = *(const f32x4 *)(Ti + 16 * b);
      }
      PT(7);                 // (trace) tile top: address setup + issue of the T loads
      PT_DRAIN();
      PT(8);                 // (trace) wait for every outstanding global access: T rows, prefetched edge rows, earlier stores
      frag8 ef;
      if (MODE == 1) {
        // ---- edge tile -> registers through the swizzled staging buffer (full 128-byte row segments)
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
#pragma unroll
          for (int n = 0; n < 2; ++n) *(f32x4 *)(stage + sw_pos(8 * n + (ll >> 3), ll & 7)) = raw[2 * qt + n];
          PBF_FENCE();
#pragma unroll
          for (int b2 = 0; b2 < 2; ++b2) ef[2 * qt + b2] = *(const f32x4 *)(stage + sw_pos(lp, 4 * b2 + lq));
          PBF_FENCE();
        }
        if (PBF_PREFETCH_TOP && tile + 1 < J.t1) { PBF_LOAD_RAW(i0 + 16, ll) }
      } else {
        // ---- layer 0: edge0 = ReLU(LN(W_r rpe + b_r)), zeros on the cls row / column (network.py:326-330)
        PAIR_EDGE0(ef, lds + LB_RT + lq * 32, tokpos, rpe_ptrs, pj, J.scene, J.tok_base, j, N, ic)
      }

      // ---- memory = ReLU(LN(W_e e + S[j] + T[i]))   (network.py:197-199, rank-decomposed, mean folded away)
      PT(0);
      u32x4 mhi[4], mlo[4];
      {
        u32x4 ehi[4], elo[4];
        split_frag<NP>(ef, ehi, elo);
        const float *svq = svec + lq * 4;
#pragma unroll
        for (int b = 0; b < 8; ++b) mem[b] += *(const f32x4 *)(svq + 16 * b);
        SCHED_FENCE();
        gemm_bf<NP>(mem, wbe, ehi, elo, lane);
      }
      PT(1);
      ln_nomean(mem, vtq, VT_GM, VT_BM);
      SCHED_FENCE();
      split_frag<NP>(mem, mhi, mlo);
      PT(2);

      u32x4 qhi[4], qlo[4];
#define PBF_LOAD_QK()                                                                              \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                  \
    qhi[g] = *(const u32x4 *)(qs + g * 128);                                                       \
    if (NP == 3) qlo[g] = *(const u32x4 *)(qs + (4 + g) * 128);                                    \
  }
      // ---- edge update e' = LN_e(e + ReLU(LN(W_p mem + b_p)))   (network.py:201-202)
      if (do_update) {
        frag8 up;
#pragma unroll
        for (int b = 0; b < 8; ++b) up[b] = *(const f32x4 *)(vtq + VT_BP + 16 * b);
        gemm_bf<NP>(up, wbp, mhi, mlo, lane);
        PT(3);
        ln_nomean(up, vtq, VT_GP, VT_BEP);
#pragma unroll
        for (int b = 0; b < 8; ++b) up[b] += ef[b];
        ln_pairs(up, vtq, VT_GE, VT_BE, false);
        SCHED_FENCE();
        // store through the staging buffer: full 128-byte row segments
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
#pragma unroll
          for (int b2 = 0; b2 < 2; ++b2) *(f32x4 *)(stage + sw_pos(lp, 4 * b2 + lq)) = up[2 * qt + b2];
          PBF_FENCE();
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            const int r = 8 * n + (ll >> 3);
            const int cp = ll & 7;
            const f32x4 v = *(const f32x4 *)(stage + sw_pos(r, cp));
            if (i0 + r < N) *(f32x4 *)(ecol + ((size_t)(i0 + r) << 7) + qt * 32 + cp * 4) = v;
          }
          PBF_FENCE();
        }
      }
      SCHED_FENCE();
      PT(4);
      // ---- the folded query first, THEN the next tile's edge rows: the memory counter retires in order, so the wait for the query
      //      fragments below leaves the eight edge-row loads issued behind them in flight (vmcnt(8)) through the whole attention
      //      phase; requested the other way round, that wait drained the prefetch the moment it was issued
#if PBF_QK_FIRST
      PBF_LOAD_QK()
      asm volatile("" ::: "memory");
#endif
#if PBF_QK_FIRST
      // (unconditional: behind a branch the compiler must assume the loads were NOT issued and waits for everything; the job's last tile
      // asks for its own rows again -- L2 hits that nobody reads)
      if (MODE == 1 && !PBF_PREFETCH_TOP) { const int nrow0 = tile + 1 < J.t1 ? i0 + 16 : i0; PBF_LOAD_RAW(nrow0, ll) }
#else
      if (MODE == 1 && !PBF_PREFETCH_TOP && tile + 1 < J.t1) { PBF_LOAD_RAW(i0 + 16, ll) }
#endif
      // ---- attention scores: S^T[head, pair] = QK_j[head, :] . mem^T[:, pair]; the memory tile is already the B operand
      f32x4 sa = (f32x4){0.f, 0.f, 0.f, 0.f}, sb = sa, sc = sa;
      {
        PT(9);               // (trace) next-tile prefetch issue
#if !PBF_QK_FIRST
        PBF_LOAD_QK()
#endif
        PT_DRAIN();
        PT(10);              // (trace) wait for the folded-query fragments (and the edge stores / prefetch queued before them)
        if (!qrow) {
#pragma unroll
          for (int g = 0; g < 4; ++g) { qhi[g] = (u32x4){0u, 0u, 0u, 0u}; qlo[g] = (u32x4){0u, 0u, 0u, 0u}; }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          sa = MFMA_BF(qhi[g], mhi[g], sa);
          if (NP == 3) {
            sb = MFMA_BF(qhi[g], mlo[g], sb);
            sc = MFMA_BF(qlo[g], mhi[g], sc);
          }
        }
      }
      if (NP == 3) sa += sb + sc;       // lane (p, q): rows 4q..4q+3 = heads 4q..4q+3 of pair p (q < 2)
      // ---- online softmax over i: lanes of quarter q own heads 4q..4q+3
      pair_softmax_step(sa, valid, lq, lp, m_run, l_part, mbar, ptab);
      // A operand: p[head = lane & 15][pairs 4q .. 4q+3], each duplicated over the (hi, lo) parts of the memory rows
      PT(5);
      u32x4 pah, pal;
      {
        f32x4 pv = *(const f32x4 *)(ptab + (lp & 7) * 16 + 4 * lq);
        if (lp >= 8) pv = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const u32 h = pk_bf16(pv[d], pv[d]);
          pah[d] = h;
          if (NP == 3) {
            const float rlo = pv[d] - bf_lo_f32(h);
            pal[d] = pk_bf16(rlo, rlo);
          }
        }
      }
      // ---- mbar[head][f] += sum_pairs p[head][pair] * mem[pair][f] on the MFMA, the memory tile transposed through the
      //      staging buffer one 32-feature quarter (= k-group g) at a time as (hi | lo << 16) dwords
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x4 f0, f1;
        pair_stage_quarter<NP == 3>(stq_w, stq_r, mhi[g], mlo[g], f0, f1);
        mbar[2 * g] = MFMA_BF(pah, f0, mbar[2 * g]);
        mbar[2 * g + 1] = MFMA_BF(pah, f1, mbar[2 * g + 1]);
        if (NP == 3) {
          mbar[2 * g] = MFMA_BF(pal, f0, mbar[2 * g]);
          mbar[2 * g + 1] = MFMA_BF(pal, f1, mbar[2 * g + 1]);
        }
      }
      PT(6);
    }  // tiles

    // ---- column partial: m[8], l[8], mbar[8][128]
    float *po = part + (size_t)J.slot * PART_STRIDE;
    PAIR_STORE_PARTIAL_DIRECT(po, m_run, l_part, mbar, p, q)
  }
#ifdef MIND_PAIR_TRACE
  if (blockIdx.x == 0 && tid == 0)
    printf("[k_pair_bf<%d,%d> um=%d] cycles: tile-top issue %lld | WAIT global (T, edge prefetch, stores) %lld | stage+split %lld | gemm1 %lld | LN1+split %lld | gemm2 %lld | "
           "LN2/3+store %lld | prefetch issue %lld | WAIT query frags (+stores) %lld | scores+softmax %lld | sum_p_mem %lld\n",
           MODE, NP, update_mode, pt_[7], pt_[8], pt_[0], pt_[1], pt_[2], pt_[3], pt_[4], pt_[9], pt_[10], pt_[5], pt_[6]);
#endif
  lc_stamp_out(clk);
}

#define PAIR_BF_INST(M, NPV)                                                                                           \
  template __global__ void k_pair_bf<M, NPV>(const PairJob *, int, float *, const float *, const float *, float *,     \
                                             const u32 *, const u32 *, const float *, const float *, const float *,    \
                                             const float *const *, int, LcSlot *);
PAIR_BF_INST(0, 3)
PAIR_BF_INST(1, 3)
PAIR_BF_INST(0, 1)
PAIR_BF_INST(1, 1)

extern "C" size_t mind_pair_bf_lds_bytes() { return (size_t)LB_TOTAL * sizeof(float); }
