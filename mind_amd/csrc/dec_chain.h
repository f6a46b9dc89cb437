// Index rules of the decoder scene part's launch chain (k_dec_chain1..4, encdec_kernels.hip): which workgroup owns which outputs and K parts of the
// three big stages, how a workgroup's threads are dealt over its items, and how many workgroups per scene a call takes.  No HIP call, no
// device code: the kernels, pred_choose and a host test program read the same functions.
//
// The chain computes what the one-workgroup kernel k_dec_scene computes, bit for bit.  There a big stage is a dense_quads call in a workgroup
// of 1 024 threads with 24 576 floats of partial sums: the K range is cut into KP parts of Kc inputs, a part's sum of one (row, output) is one
// chain of fused multiply-adds in ascending k starting at 0, and the output is bias + part 0 + part 1 + ... in that order.  Here the same
// chains are dealt over the G workgroups of a scene and, inside a workgroup, over (K part, row group, output) items:
//   c3 (384 -> 768, 1 row,  KP 4,  Kc 96): workgroup wg owns the outputs [768 wg / G, 768 (wg + 1) / G) with all four parts           (kernel 1)
//   l1 (128 -> 1536, 6 rows, KP 2, Kc 64): workgroup wg owns the outputs [1536 wg / G, 1536 (wg + 1) / G) with both parts              (kernels 2, 3)
//   l2 (1536 -> 128, 6 rows, KP 32, Kc 48): part kp reads l1's outputs [48 kp, 48 kp + 48), so workgroup wg owns the parts
//      [32 wg / G, 32 (wg + 1) / G) -- exactly the parts that read its own l1 slice -- with all 128 outputs; the 32 partial sums of an output
//      meet in global memory and the NEXT kernel of the chain adds them up: a kernel boundary, no barrier.
#pragma once

#define DC_THREADS 1024          // threads of k_dec_scene (DT): the K split below is the one dense_quads takes there
#define DC_PART_FLOATS 24576     // floats of its partial-sum area (DEC_SCENE_PART)
#define DC_ROWS 6                // mode tokens

struct DcStage { int K, NOUT, R, KP, Kc; };

// dense_quads' K split (encdec_kernels.hip) for R rows, K inputs, NOUT outputs in a workgroup of nthr threads with part_floats floats of partials
constexpr int dc_quads_kp(int R, int K, int NOUT, int nthr, int part_floats) {
  int KP = 1;
  while (KP * 2 * (NOUT >> 2) <= nthr && KP * 2 * R * NOUT <= part_floats && KP * 2 <= (K >> 2)) KP *= 2;
  return KP;
}
constexpr int dc_quads_kc(int K, int KP) { return ((K / 4 + KP - 1) / KP) * 4; }

constexpr DcStage DC_C3 = {384, 768, 1, 4, 96};
constexpr DcStage DC_L1 = {128, 1536, DC_ROWS, 2, 64};
constexpr DcStage DC_L2 = {1536, 128, DC_ROWS, 32, 48};
constexpr bool dc_stage_ok(const DcStage &s) {
  return s.KP == dc_quads_kp(s.R, s.K, s.NOUT, DC_THREADS, DC_PART_FLOATS) && s.Kc == dc_quads_kc(s.K, s.KP) && s.KP * s.Kc == s.K;
}
static_assert(dc_stage_ok(DC_C3) && dc_stage_ok(DC_L1) && dc_stage_ok(DC_L2), "the chain restates dense_quads' K split of the three big stages");
static_assert(DC_L2.K == DC_L1.NOUT && DC_L1.NOUT == DC_L2.KP * DC_L2.Kc, "an l2 part reads a 48-wide slice of l1's outputs");

// workgroups per scene: the largest of 32 / 16 / 8 that leaves every workgroup of the launch a compute unit of its own (a workgroup takes a whole
// unit's LDS); 0: no chain -- more than n_cu / 8 scenes run the one-workgroup kernel.  Nothing waits for a peer, so residency is a matter of
// speed only.
constexpr int dc_choose_g(int n_scenes, int n_cu) {
  if (n_scenes <= 0) return 0;
  for (int G = 32; G >= 8; G >>= 1)
    if ((long long)n_scenes * G <= n_cu) return G;
  return 0;
}
constexpr bool dc_valid_g(int G) { return G == 8 || G == 16 || G == 32; }

// what workgroup wg of G computes of a stage: outputs [o_lo, o_lo + no) of the parts [kp_lo, kp_lo + nkp)
struct DcSlice { int o_lo, no, kp_lo, nkp; };
constexpr DcSlice dc_slice_c3(int wg, int G) { return {DC_C3.NOUT / G * wg, DC_C3.NOUT / G, 0, DC_C3.KP}; }
constexpr DcSlice dc_slice_l1(int wg, int G) { return {DC_L1.NOUT / G * wg, DC_L1.NOUT / G, 0, DC_L1.KP}; }
constexpr DcSlice dc_slice_l2(int wg, int G) { return {0, DC_L2.NOUT, DC_L2.KP / G * wg, DC_L2.KP / G}; }

// rows per thread: the fewest (a divisor of R) with which the slice's items fit one pass over the workgroup's threads
constexpr int dc_rows_per_thread(int R, int nkp, int no) {
  for (int rpt = 1; rpt < R; ++rpt)
    if (R % rpt == 0 && nkp * (R / rpt) * no <= DC_THREADS) return rpt;
  return R;
}
constexpr int dc_items(int R, int rpt, int nkp, int no) { return nkp * (R / rpt) * no; }

// item -> (part within the slice, first row, output within the slice); the output runs fastest: a wave reads consecutive weights
struct DcItem { int kpl, r0, ol; };
constexpr DcItem dc_item(int item, int R, int rpt, int no) { return {item / (no * (R / rpt)), (item / no) % (R / rpt) * rpt, item % no}; }

// floats per scene of the chain's global buffers: y [768] | C of the two encoder layers [2][6][128] | l2 partials of the two layers [2][32][6][128]
#define DC_Y_FLOATS 768
#define DC_C_FLOATS (DC_ROWS * 128)
#define DC_P_FLOATS (32 * DC_ROWS * 128)
#define DC_SCENE_FLOATS (DC_Y_FLOATS + 2 * DC_C_FLOATS + 2 * DC_P_FLOATS)
