// Host check of mind_amd/csrc/dec_chain.h (built and run by tests/test_dec_chain_host.py, plain and under ASan + UBSan): the index rules of the
// decoder scene part's launch chain, for G = 8 / 16 / 32 workgroups per scene and its three stage shapes.  Prints one line per failed
// check and "checks <n> failures <m>"; exit status 1 when anything failed.
#include <cstdio>
#include <vector>

#include "../mind_amd/csrc/dec_chain.h"

static int n_checks = 0, n_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++n_checks;                                           \
    if (!(cond)) { ++n_fail; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

// every (K part, row, output) of the stage is produced exactly once over the G workgroups and their items; an item stays inside its slice
static void coverage(const char *name, const DcStage &st, DcSlice (*slice)(int, int), int G) {
  std::vector<int> seen((size_t)st.KP * st.R * st.NOUT, 0);
  for (int wg = 0; wg < G; ++wg) {
    const DcSlice sl = slice(wg, G);
    const int rpt = dc_rows_per_thread(st.R, sl.nkp, sl.no), items = dc_items(st.R, rpt, sl.nkp, sl.no);
    CHECK(st.R % rpt == 0 && items <= DC_THREADS && items > 0, "%s G %d wg %d: %d rows per thread, %d items", name, G, wg, rpt, items);
    CHECK(sl.o_lo >= 0 && sl.o_lo + sl.no <= st.NOUT && sl.kp_lo >= 0 && sl.kp_lo + sl.nkp <= st.KP, "%s G %d wg %d: slice out of range", name, G, wg);
    for (int item = 0; item < items; ++item) {
      const DcItem it = dc_item(item, st.R, rpt, sl.no);
      const bool in = it.kpl >= 0 && it.kpl < sl.nkp && it.r0 >= 0 && it.r0 + rpt <= st.R && it.ol >= 0 && it.ol < sl.no;
      CHECK(in, "%s G %d wg %d item %d -> part %d row %d output %d", name, G, wg, item, it.kpl, it.r0, it.ol);
      if (!in) continue;
      for (int j = 0; j < rpt; ++j) ++seen[((size_t)(sl.kp_lo + it.kpl) * st.R + it.r0 + j) * st.NOUT + sl.o_lo + it.ol];
    }
  }
  long bad = 0;
  for (int v : seen) bad += v != 1;
  CHECK(bad == 0, "%s G %d: %ld of %zu (part, row, output) not produced exactly once", name, G, bad, seen.size());
}

int main() {
  // the K split the header assumes is dense_quads' for 1 024 threads and 24 576 partial floats
  const DcStage stages[3] = {DC_C3, DC_L1, DC_L2};
  const int want[3][2] = {{4, 96}, {2, 64}, {32, 48}};
  for (int s = 0; s < 3; ++s) {
    const int kp = dc_quads_kp(stages[s].R, stages[s].K, stages[s].NOUT, 1024, 24576), kc = dc_quads_kc(stages[s].K, kp);
    CHECK(kp == stages[s].KP && kc == stages[s].Kc && kp == want[s][0] && kc == want[s][1], "stage %d: KP %d Kc %d", s, kp, kc);
  }
  for (int G : {8, 16, 32}) {
    CHECK(dc_valid_g(G), "G %d", G);
    CHECK(768 % G == 0 && 1536 % G == 0 && 32 % G == 0, "G %d: slices not exact", G);
    coverage("c3", DC_C3, dc_slice_c3, G);
    coverage("l1", DC_L1, dc_slice_l1, G);
    coverage("l2", DC_L2, dc_slice_l2, G);
    // a workgroup's l2 parts read only its own l1 slice: part kp reads l1's outputs [48 kp, 48 kp + 48)
    for (int wg = 0; wg < G; ++wg) {
      const DcSlice l1 = dc_slice_l1(wg, G), l2 = dc_slice_l2(wg, G);
      CHECK(l2.kp_lo * DC_L2.Kc == l1.o_lo && l2.nkp * DC_L2.Kc == l1.no, "G %d wg %d: l2 parts [%d, +%d) against l1 outputs [%d, +%d)", G, wg, l2.kp_lo,
            l2.nkp, l1.o_lo, l1.no);
      for (int kp = l2.kp_lo; kp < l2.kp_lo + l2.nkp; ++kp)
        CHECK(kp * DC_L2.Kc >= l1.o_lo && (kp + 1) * DC_L2.Kc <= l1.o_lo + l1.no, "G %d wg %d part %d reads outside the slice", G, wg, kp);
    }
  }
  CHECK(!dc_valid_g(0) && !dc_valid_g(4) && !dc_valid_g(64) && !dc_valid_g(24), "forms other than 8 / 16 / 32");
  // the G rule: the largest of 32 / 16 / 8 with scenes x G <= n_cu, else no chain
  const int scenes[6] = {1, 5, 8, 9, 32, 33}, g256[6] = {32, 32, 32, 16, 8, 0}, g32[6] = {32, 0, 0, 0, 0, 0};
  for (int i = 0; i < 6; ++i) {
    CHECK(dc_choose_g(scenes[i], 256) == g256[i], "%d scenes on 256 CUs -> %d", scenes[i], dc_choose_g(scenes[i], 256));
    CHECK(dc_choose_g(scenes[i], 32) == g32[i], "%d scenes on 32 CUs -> %d", scenes[i], dc_choose_g(scenes[i], 32));
  }
  for (int n_cu : {32, 104, 256, 304})
    for (int n = 1; n <= 64; ++n) {
      const int G = dc_choose_g(n, n_cu);
      CHECK(G == 0 ? n * 8 > n_cu : (dc_valid_g(G) && n * G <= n_cu && (G == 32 || n * 2 * G > n_cu)), "%d scenes on %d CUs -> %d", n, n_cu, G);
    }
  CHECK(dc_choose_g(0, 256) == 0 && dc_choose_g(-3, 256) == 0, "no scenes");
  std::printf("checks %d failures %d\n", n_checks, n_fail);
  return n_fail ? 1 : 0;
}
