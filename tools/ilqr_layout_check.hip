// Stand-alone check of il_layout (mind_amd/csrc/ilqr_choice.h), host code only: lays out the device arena of tree-iLQR calls with and without a
// scoring, a gains or a policy-rollout request and asserts that every region is disjoint from the others, aligned as its kind is (doubles 16 bytes, floats and ints 16
// bytes) and inside the reported size, and that a call without such a request lays out exactly as one whose shape never heard of it.
// Meant for a sanitizer build, on a machine without a GPU (no HIP call is made):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/ilqr_layout_check.hip -o ilqr_layout_check && ./ilqr_layout_check
#include "../mind_amd/csrc/ilqr_kernels.hip"
#include "../mind_amd/csrc/ilqr_choice.h"
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <string>

struct Region { std::string name; size_t lo, hi; };

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s failed (trees %d, candidates %d, request %d)\n", __FILE__, __LINE__, #cond, n_trees, n_cand, req); exit(1); } } while (0)

static std::vector<int32_t> tree_parents(int M) {      // a trunk of M / 2 nodes, the rest hanging off its end in two chains
  std::vector<int32_t> p(M);
  const int trunk = std::max(1, M / 2);
  for (int i = 0; i < M; ++i) p[i] = i == 0 ? -1 : (i < trunk ? i - 1 : (i == trunk || i == trunk + (M - trunk) / 2 + 1 ? trunk - 1 : i - 1));
  return p;
}

// req: 0 a scoring call of n_cand candidates (a plain solve when n_cand == 0), 1 a gains call, 2 a policy-rollout call of n_cand candidates
// dealt to blocks of `cb`
static size_t check_case(const std::vector<int> &Ms, const std::vector<int> &agents, int n_cand, bool gen, bool use_exo, int req = 0, int cb = 64) {
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
  const IlqrChoice ch = il_choose(tun, 256, n_trees, maxM, Mtot, gen, n_cand > 0 || req != 0);
  const int W = gen ? 9 : 256, H = gen ? 8 : 256;
  IlShape shape{W, H, gen ? 0 : 40, 0, n_trees, agents.data(), gen, use_exo, false, 100, req == 0 ? n_cand : 0};
  const int n_blk = req == 2 ? (n_cand + cb - 1) / cb : 0;
  shape.gains = req == 1; shape.n_pol = req == 2 ? n_cand : 0; shape.n_pol_blk = n_blk;
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
  const size_t rows = req == 0 ? (size_t)n_cand * (size_t)Mtot : 0;
  addD("gx", A.o_gx, W, -1); addD("gy", A.o_gy, H, -1); addD("lane", A.o_lane, (size_t)shape.n_lane_pts * 2 + 2, -1);
  addD("quad", A.o_quad, gen ? 2 : (size_t)W * H, -1);
  addD("score us", A.o_scu, rows * 2, -1); addD("score xs", A.o_scx, rows * 6, -1); addD("score L", A.o_scl, rows, -1);
  addD("score J", A.o_scj, req == 0 ? (size_t)n_cand * n_trees : 0, -1);
  CHECK(rows == 0 || A.o_scu < A.nd_in);                             // the candidates travel with the one upload
  CHECK(rows == 0 || (A.o_scx >= A.nd_in && A.o_scl >= A.nd_in && A.o_scj >= A.nd_in));
  if (req == 1) {
    const size_t M = (size_t)Mtot;
    addD("gains mu", A.o_gmu, n_trees, -1); addD("gains k", A.o_gk, 2 * M, -1); addD("gains K", A.o_gK, 12 * M, -1); addD("gains dV", A.o_gdv, M, -1);
    addD("gains Vx", A.o_gvx, 6 * M, -1); addD("gains Vxx", A.o_gvxx, 36 * M, -1); addD("gains xs", A.o_gxs, 6 * M, -1); addD("gains L", A.o_gl, M, -1);
    addD("gains J", A.o_gj, n_trees, -1); addD("gains bad_node", A.o_gbad, n_trees, -1);
    CHECK(A.o_gmu < A.nd_in && A.o_gk >= A.nd_in && A.o_gj >= A.nd_in);
    // the outputs lie back to back in the order the one read-back takes them apart
    const size_t ev = ((size_t)M + 1) & ~(size_t)1, evt = ((size_t)n_trees + 1) & ~(size_t)1;
    CHECK(A.o_gK == A.o_gk + 2 * M && A.o_gdv == A.o_gK + 12 * M && A.o_gvx == A.o_gdv + ev && A.o_gvxx == A.o_gvx + 6 * M && A.o_gxs == A.o_gvxx + 36 * M);
    CHECK(A.o_gl == A.o_gxs + 6 * M && A.o_gj == A.o_gl + ev && A.o_gbad == A.o_gj + evt);
  }
  if (req == 2) {
    const size_t M = (size_t)Mtot, pr = (size_t)n_cand * M;
    addD("policy k", A.o_pk, 2 * M, -1); addD("policy K", A.o_pK, 12 * M, -1); addD("policy alpha", A.o_pal, n_cand, -1); addD("policy dx0", A.o_pdx, 6 * (size_t)n_cand, -1);
    addD("policy xnom", A.o_pxn, 6 * (size_t)n_blk * M, -1); addD("policy xs", A.o_pxs, 6 * pr, -1); addD("policy us", A.o_pus, 2 * pr, -1);
    addD("policy L", A.o_pl, pr, -1); addD("policy J", A.o_pj, (size_t)n_cand * n_trees, -1);
    CHECK(A.o_pk < A.nd_in && A.o_pK < A.nd_in && A.o_pal < A.nd_in && A.o_pdx < A.nd_in);
    CHECK(A.o_pxn >= A.nd_in && A.o_pxs >= A.nd_in && A.o_pus >= A.nd_in && A.o_pl >= A.nd_in && A.o_pj >= A.nd_in);
  }
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
  if (n_cand > 0 || req != 0) {
    IlShape plain{W, H, gen ? 0 : 40, 0, n_trees, agents.data(), gen, use_exo, false, 100};
    IlArena B, S;
    il_layout(plain, ch, tab.data(), B);
    plain.n_cand = 0;
    il_layout(plain, ch, tab.data(), S);
    CHECK(B.total == S.total && B.nd == S.nd && B.nd_in == S.nd_in && B.o_work == S.o_work && memcmp(B.tree.data(), S.tree.data(), n_trees * sizeof(IlTreeOff)) == 0);
    CHECK(B.o_scu == B.nd_in && B.o_scx == B.nd && B.o_scl == B.nd && B.o_scj == B.nd);      // empty regions: nothing moved
    CHECK(B.o_gmu == B.nd_in && B.o_pk == B.nd_in && B.o_pK == B.nd_in && B.o_pal == B.nd_in && B.o_pdx == B.nd_in);
    CHECK(B.o_gk == B.nd && B.o_gK == B.nd && B.o_gdv == B.nd && B.o_gvx == B.nd && B.o_gvxx == B.nd && B.o_gxs == B.nd && B.o_gl == B.nd && B.o_gj == B.nd && B.o_gbad == B.nd);
    CHECK(B.o_pxn == B.nd && B.o_pxs == B.nd && B.o_pus == B.nd && B.o_pl == B.nd && B.o_pj == B.nd);
    CHECK(B.ni == A.ni && B.nf == A.nf);
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
      // a gains call; policy-rollout calls of one candidate, of 65 in blocks of 64 / 7 / 1, and of the most a call admits
      tot += check_case({1}, {gen ? 1 : 3}, 0, gen, exo, 1);
      tot += check_case(mixed, gen ? std::vector<int>{1, 1, 1} : std::vector<int>{4, 1, 12}, 0, gen, exo, 1);
      tot += check_case({1}, {gen ? 1 : 3}, 1, gen, exo, 2);
      for (const int cb : {64, 7, 1}) tot += check_case(mixed, gen ? std::vector<int>{1, 1, 1} : std::vector<int>{4, 1, 12}, 65, gen, exo, 2, cb);
      tot += check_case({150, 150, 150, 150, 150}, gen ? std::vector<int>{1, 1, 1, 1, 1} : std::vector<int>{16, 16, 16, 16, 16}, 1398, gen, exo, 2, 4);
    }
  printf("ilqr_layout_check: ok (%zu bytes laid out)\n", tot);
  return 0;
}
