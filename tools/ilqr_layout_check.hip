// Stand-alone check of il_layout (mind_amd/csrc/ilqr_choice.h), host code only: lays out the device arena of tree-iLQR calls with and without a
// scoring request and asserts that every region is disjoint from the others, aligned as its kind is (doubles 16 bytes, floats and ints 16
// bytes) and inside the reported size, and that a call without a scoring request lays out exactly as one whose shape never heard of it.
// Meant for a sanitizer build, on a machine without a GPU (no HIP call is made):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/ilqr_layout_check.hip -o ilqr_layout_check && ./ilqr_layout_check
#include "../mind_amd/csrc/ilqr_kernels.hip"
#include "../mind_amd/csrc/ilqr_choice.h"
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <string>

struct Region { std::string name; size_t lo, hi; };

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (trees %d, candidates %d)\n", __FILE__, __LINE__, #cond, n_trees, n_cand); exit(1); } } while (0)

static std::vector<int32_t> tree_parents(int M) {      // a trunk of M / 2 nodes, the rest hanging off its end in two chains
  std::vector<int32_t> p(M);
  const int trunk = std::max(1, M / 2);
  for (int i = 0; i < M; ++i) p[i] = i == 0 ? -1 : (i < trunk ? i - 1 : (i == trunk || i == trunk + (M - trunk) / 2 + 1 ? trunk - 1 : i - 1));
  return p;
}

static size_t check_case(const std::vector<int> &Ms, const std::vector<int> &agents, int n_cand, bool gen, bool use_exo) {
  const int n_trees = (int)Ms.size();
  IlqrTuning tun;
  std::vector<IlTables> tab(n_trees);
  int maxM = 0;
  long Mtot = 0;
  for (int t = 0; t < n_trees; ++t) {
    const std::vector<int32_t> par = tree_parents(Ms[t]);
    CHECK(il_tree_tables(par.data(), Ms[t], tun.ilqr_chunk, tab[t]) == -1);
    maxM = std::max(maxM, Ms[t]); Mtot += Ms[t];
  }
  const IlqrChoice ch = il_choose(tun, 256, n_trees, maxM, Mtot, gen, n_cand > 0);
  const int W = gen ? 9 : 256, H = gen ? 8 : 256;
  const IlShape shape{W, H, gen ? 0 : 40, 0, n_trees, agents.data(), gen, use_exo, false, 100, n_cand};
  IlArena A;
  il_layout(shape, ch, tab.data(), A);
  // every doubles region as bytes of the arena: the uploaded ones from 0, the produced ones from o_work
  std::vector<Region> R;
  const auto addD = [&](const char *name, size_t o, size_t n, int t) {
    if (!n) return;
    CHECK(o % 2 == 0);                                               // 16-byte aligned inside its region
    const bool in = o < A.nd_in;
    CHECK(in ? o + n <= A.nd_in : o + n <= A.nd);
    const size_t b = in ? o * 8 : A.o_work + (o - A.nd_in) * 8;
    R.push_back({std::string(name) + "[" + std::to_string(t) + "]", b, b + n * 8});
  };
  const size_t rows = (size_t)n_cand * (size_t)Mtot;
  addD("gx", A.o_gx, W, -1); addD("gy", A.o_gy, H, -1); addD("lane", A.o_lane, (size_t)shape.n_lane_pts * 2 + 2, -1);
  addD("quad", A.o_quad, gen ? 2 : (size_t)W * H, -1);
  addD("score us", A.o_scu, rows * 2, -1); addD("score xs", A.o_scx, rows * 6, -1); addD("score L", A.o_scl, rows, -1);
  addD("score J", A.o_scj, (size_t)n_cand * n_trees, -1);
  CHECK(n_cand == 0 || A.o_scu < A.nd_in);                           // the candidates travel with the one upload
  CHECK(n_cand == 0 || (A.o_scx >= A.nd_in && A.o_scl >= A.nd_in && A.o_scj >= A.nd_in));
  const size_t ns = (size_t)ch.nslot;
  for (int t = 0; t < n_trees; ++t) {
    const IlTreeOff &L = A.tree[t];
    const size_t M = Ms[t], a = agents[t];
    addD("us", L.us, 2 * M, t); addD("nodew", L.nodew, gen ? M * IL_NW : 0, t); addD("xs", L.xs, 6 * M, t); addD("stats", L.stats, 2 * IL_NSTAT, t);
    addD("trace", L.trace, (size_t)2 * shape.trace_cap * IL_TRACE_W, t);
    addD("relag", L.relag, use_exo ? M * IL_RA : 0, t); addD("Fx", L.Fx, 36 * M, t); addD("L", L.L, M, t); addD("Lx", L.Lx, 6 * M, t); addD("Lxx", L.Lxx, 36 * M, t);
    addD("k", L.k, ns * 2 * M, t); addD("K", L.K, ns * 12 * M, t); addD("Vx", L.Vx, ns * 6 * M, t); addD("Vxx", L.Vxx, ns * 36 * M, t);
    addD("xsn", L.xsn, ns * 60 * M, t); addD("usn", L.usn, ns * 20 * M, t); addD("Ln", L.Ln, ns * 10 * M, t);
    const auto addF = [&](const char *name, size_t o, size_t n) {
      if (!n) return;
      CHECK(o % 4 == 0 && o + n <= A.nf);
      R.push_back({std::string(name) + "[" + std::to_string(t) + "]", A.bytesIn + o * 4, A.bytesIn + (o + n) * 4});
    };
    addF("prob", L.prob, M); addF("mean", L.mean, M * a * 2); addF("cov", L.cov, M * a);
    const auto addI = [&](const char *name, size_t o, size_t n) {
      if (!n) return;
      CHECK(o % 4 == 0 && o + n <= A.ni);
      R.push_back({std::string(name) + "[" + std::to_string(t) + "]", A.bytesIn + A.bytesF + o * 4, A.bytesIn + A.bytesF + (o + n) * 4});
    };
    addI("parent", L.parent, M); addI("lnodes", L.lnodes, M); addI("cstart", L.cstart, M + 1); addI("clist", L.clist, M); addI("rel", L.rel, M);
    addI("lstart", L.lstart, tab[t].lvl_start.size()); addI("sstart", L.sstart, tab[t].seg_start.size()); addI("snodes", L.snodes, M);
    addI("slstart", L.slstart, tab[t].slvl_start.size()); addI("slsegs", L.slsegs, tab[t].slvl_segs.size()); addI("segrec", L.segrec, tab[t].seg_rec.size());
    addI("fsstart", L.fsstart, tab[t].fs_start.size()); addI("fsitems", L.fsitems, tab[t].fs_items.size()); addI("fsq1", L.fsq1, tab[t].fs_q1.size());
    addI("fsnstart", L.fsnstart, tab[t].fs_nstart.size()); addI("fsnodes", L.fsnodes, M);
    if (gen) R.push_back({"field[" + std::to_string(t) + "]", L.field, L.field + M * W * H * 8});
  }
  R.push_back({"structs", A.o_structs, A.o_structs + (size_t)n_trees * sizeof(IlqrTreeDev)});
  R.push_back({"consts", A.o_consts, A.o_consts + 2 * sizeof(IlqrConst)});
  CHECK(A.bytesIn == A.nd_in * 8 && A.o_structs == A.bytesIn + A.bytesF + A.bytesI && A.o_consts % 16 == 0 && A.o_work % 16 == 0 && A.total % 16 == 0);
  CHECK(A.o_consts >= A.o_structs + (size_t)n_trees * sizeof(IlqrTreeDev) && A.o_work >= A.o_consts + 2 * sizeof(IlqrConst));
  std::sort(R.begin(), R.end(), [](const Region &x, const Region &y) { return x.lo < y.lo; });
  for (size_t i = 0; i < R.size(); ++i) {
    CHECK(R[i].lo % 16 == 0 && R[i].hi <= A.total);
    if (i + 1 < R.size() && R[i].hi > R[i + 1].lo) {
      fprintf(stderr, "regions %s [%zu, %zu) and %s [%zu, %zu) overlap\n", R[i].name.c_str(), R[i].lo, R[i].hi, R[i + 1].name.c_str(), R[i + 1].lo, R[i + 1].hi);
      exit(1);
    }
  }
  // the image of the arena's uploaded part and a produced part of the reported size: every region written end to end under the sanitizer
  std::vector<unsigned char> img(A.total, 0);
  for (const Region &r : R) memset(img.data() + r.lo, 0x5a, r.hi - r.lo);
  // without the request the same trees lay out as a shape that leaves n_cand at its default: byte for byte what a plain call gets
  if (n_cand > 0) {
    IlShape plain{W, H, gen ? 0 : 40, 0, n_trees, agents.data(), gen, use_exo, false, 100};
    IlArena B, S;
    il_layout(plain, ch, tab.data(), B);
    plain.n_cand = 0;
    il_layout(plain, ch, tab.data(), S);
    CHECK(B.total == S.total && B.nd == S.nd && B.nd_in == S.nd_in && B.o_work == S.o_work && memcmp(B.tree.data(), S.tree.data(), n_trees * sizeof(IlTreeOff)) == 0);
    CHECK(B.o_scu == B.nd_in && B.o_scx == B.nd && B.o_scl == B.nd && B.o_scj == B.nd);      // empty regions: nothing moved
    CHECK(A.total > B.total);
  }
  return A.total;
}

int main() {
  const std::vector<int> mixed = {19, 1, 150};
  size_t tot = 0;
  for (const bool gen : {false, true})
    for (const bool exo : {false, true}) {
      if (gen && exo) continue;
      tot += check_case({1}, {gen ? 1 : 3}, 1, gen, exo);
      tot += check_case(mixed, gen ? std::vector<int>{1, 1, 1} : std::vector<int>{4, 1, 12}, 65, gen, exo);
      tot += check_case({150, 150, 150, 150, 150}, gen ? std::vector<int>{1, 1, 1, 1, 1} : std::vector<int>{16, 16, 16, 16, 16}, 1398, gen, exo);
      tot += check_case(mixed, gen ? std::vector<int>{1, 1, 1} : std::vector<int>{4, 1, 12}, 0, gen, exo);
    }
  printf("ilqr_layout_check: ok (%zu bytes laid out)\n", tot);
  return 0;
}
