// What a tree-iLQR call decides before it touches the device: the solver's knobs (IlqrTuning, tuning.h), the launch form (il_choose -> IlqrChoice), the
// index tables of one cost tree (il_tree_tables -> IlTables) and where everything lies in the device arena (il_layout -> IlArena, il_stage_ints).
// No HIP call, no context: ilqr_host.hip's steps switch on these records and read no knob themselves; tests read the first three through
// mind_debug_ilqr_plan.  Included by mind_hip.hip behind ilqr_kernels.hip (IL_SLOTS, IL_SPEC, IL_THREADS, the sizes of its structs).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "tuning.h"

// The launch of one call.  form 0: one workgroup per tree (k_ilqr<GEN, 0>; always in the generic mode, and what a cost evaluation reports);
// form 1: wide trees, G workgroups share a tree's items (k_ilqr<false, 1>); form 2: narrow trees, a master + GS - 1 followers take a tree's
// Levenberg-Marquardt slots, + `spec` derivative speculators (k_ilqr<false, 2>)
struct IlqrChoice {
  int form = 0;
  int G = 1, GS = 1, spec = 0;
  int nslot = IL_SPEC;          // sets of per-slot arrays (gains, value functions, candidates: ~146 doubles per node and slot) in the arena
  int grid = 0;                 // workgroups of the launch
  int wgs_per_tree = 1;         // mind_last_ilqr_stats' workgroups_per_tree
  bool host_out = false;        // the kernel writes xs, us and the statistics to the host staging itself at its end
  bool early = false;           // ... and marks every tree when it is complete: the caller may look at it before the launch has ended (mind_loop)
  bool starve_followers = false;      // "ilqr_test_starve" in form 2: the followers leave at once, as if they were never scheduled
};

static IlqrChoice il_choose(const IlqrTuning &t, int n_cu, int n_trees, int max_nodes, long total_nodes, bool gen, bool eval) {
  IlqrChoice ch;
  const int blocks8 = ((n_trees + 7) / 8) * 8;
  int G = t.ilqr_wgs;
  // trees of tens of thousands of nodes (the deep stress trees: 29.5 k) keep twice the workgroups busy: 55 -> 35 ms per launch at 32 per tree,
  // while the cfg4 trees (6.5 k nodes) are best at 16-24 (profiles/r03an_*)
  if (G > 1 && G < t.ilqr_wgs_big && max_nodes >= t.ilqr_big_min) G = t.ilqr_wgs_big;
  while (G > 1 && blocks8 * G > n_cu) G >>= 1;     // every workgroup of the launch must be resident (1 per CU)
  const bool multi = !gen && !eval && G > 1 && max_nodes >= t.ilqr_multi_min;
  // (ilqr_wgs == 1 is the caller's "stay on few CUs": the speculative warm start beside the predictor)
  int GS = (multi || gen || eval || t.ilqr_wgs <= 1) ? 1 : t.ilqr_slots;
  while (GS > 1 && blocks8 * GS > n_cu) --GS;
  const bool slots = GS > 1;
  ch.form = multi ? 1 : slots ? 2 : 0;
  ch.G = multi ? G : 1;
  ch.GS = GS;
  // the derivative speculator: one more workgroup per tree, only where the whole launch stays resident with it
  ch.spec = slots && t.ilqr_spec_deriv && GS < 31 && blocks8 * (GS + 1) <= n_cu ? 1 : 0;
  // what this launch can use -- the followers' slots (GS, after the residency loop above) or the master's own speculation (IL_SPEC), not
  // IL_SLOTS for every narrow-tree launch
  ch.nslot = slots ? std::max(GS, IL_SPEC) : IL_SPEC;
  // a follower that is not resident yet is simply not used (IlSlotCtl.alive): form 2 needs no co-residency.  ilqr_test_starve in form 1: the
  // last eight workgroups are withheld, as if the device could not hold the whole launch -- their peers wait at the first barrier, raise the
  // abort word and the call falls back to form 0
  ch.grid = ch.form == 2 ? blocks8 * (GS + ch.spec) : ch.form == 1 ? blocks8 * G - (t.ilqr_test_starve ? 8 : 0) : n_trees;
  ch.wgs_per_tree = ch.form == 1 ? G : ch.form == 2 ? GS + ch.spec : 1;
  ch.starve_followers = ch.form == 2 && t.ilqr_test_starve;
  ch.host_out = !eval && t.ilqr_host_out_max > 0 && total_nodes <= t.ilqr_host_out_max;
  // per-tree completion words only for a launch that cannot abort
  ch.early = ch.host_out && !multi && !gen;
  return ch;
}

// Candidates per workgroup of a scoring launch (k_ilqr_score: one workgroup per cost tree and block of candidates, a lane per candidate in its
// state recursion).  A full wave of 64 while that still leaves two workgroups per CU; halved otherwise, down to 4 -- a block's waves price
// nodes x candidates items, so smaller blocks spread a small call over more CUs
static int il_score_block(const IlqrTuning &t, int n_cu, int n_trees, int n_cand) {
  if (t.ilqr_score_block > 0) return t.ilqr_score_block;
  int cb = 64;
  while (cb > 4 && (long)n_trees * ((n_cand + cb - 1) / cb) < 2L * n_cu) cb >>= 1;
  return cb;
}

// Index tables of one cost tree, as the kernels read them (IlqrTreeDev), + the scratch they are built with: kept in the context, so that a
// planning cycle does not allocate a hundred small vectors
struct IlTables {
  std::vector<int> lvl_start, lvl_nodes;        // [nl + 1], [M]: nodes sorted by depth
  std::vector<int> child_start, child_list;     // [M + 1], [max(M - 1, 1)]
  std::vector<int> seg_start, seg_nodes;        // [nseg + 1], [M]: chain segments (maximal single-child paths), root -> leaf inside a segment
  std::vector<int> slvl_start, slvl_segs;       // [nsl + 1], [nseg]: segments grouped by depth in the segment tree
  std::vector<int> seg_rec;                     // [nseg][16]
  std::vector<int> fs_start, fs_items, fs_q1, fs_nstart, fs_nodes;      // forward steps: [nfs + 1], [items][8], [items], [nfs + 1], [M]
  int nl = 0, nseg = 0, nsl = 0, maxls = 0, nfs = 0;
  std::vector<int> depth, fill, child_fill, seg_of, seg_depth, slvl_fill;     // scratch
};

// Builds `out` for the tree parent[0..M) with forward steps of at most `ilqr_chunk` nodes (0: whole segments).  Node 0 must have parent -1
// and node i > 0 a parent below i: returns the first node that has not, -1 when the tree is sound.
static int il_tree_tables(const int32_t *parent, int M, int ilqr_chunk, IlTables &out) {
  IlTables &T = out;
  // levels need the depth first
  T.depth.assign(M, 0);
  int maxd = 0;
  for (int i = 0; i < M; ++i) {
    const int p = parent[i];
    if (i == 0 ? p != -1 : (p < 0 || p >= i)) return i;
    T.depth[i] = i == 0 ? 0 : T.depth[p] + 1;
    maxd = std::max(maxd, T.depth[i]);
  }
  T.nl = maxd + 1;
  T.lvl_start.assign(maxd + 2, 0);
  for (int i = 0; i < M; ++i) T.lvl_start[T.depth[i] + 1]++;
  for (int d = 0; d <= maxd; ++d) T.lvl_start[d + 1] += T.lvl_start[d];
  T.lvl_nodes.resize(M);
  T.fill.assign(maxd + 1, 0);
  for (int i = 0; i < M; ++i) T.lvl_nodes[T.lvl_start[T.depth[i]] + T.fill[T.depth[i]]++] = i;
  T.child_start.assign(M + 1, 0);
  for (int i = 1; i < M; ++i) T.child_start[parent[i] + 1]++;
  for (int i = 0; i < M; ++i) T.child_start[i + 1] += T.child_start[i];
  T.child_list.assign(M > 1 ? M : 1, 0);
  T.child_fill.assign(M, 0);
  for (int i = 1; i < M; ++i) T.child_list[T.child_start[parent[i]] + T.child_fill[parent[i]]++] = i;
  // chain segments: a node starts a segment if it is node 0 or its parent has >= 2 children
  const auto nchild = [&T](int i) { return T.child_start[i + 1] - T.child_start[i]; };
  T.seg_of.assign(M, -1); T.seg_depth.clear();
  T.seg_start.clear(); T.seg_nodes.clear();
  for (int i = 0; i < M; ++i) {
    if (!(i == 0 || nchild(parent[i]) >= 2)) continue;
    const int sidx = (int)T.seg_start.size();
    T.seg_start.push_back((int)T.seg_nodes.size());
    T.seg_depth.push_back(i == 0 ? 0 : T.seg_depth[T.seg_of[parent[i]]] + 1);
    for (int n = i;; n = T.child_list[T.child_start[n]]) {
      T.seg_of[n] = sidx;
      T.seg_nodes.push_back(n);
      if (nchild(n) != 1) break;
    }
  }
  T.seg_start.push_back((int)T.seg_nodes.size());
  const int nseg = (int)T.seg_depth.size();
  int maxsd = 0;
  for (int d : T.seg_depth) maxsd = std::max(maxsd, d);
  T.slvl_start.assign(maxsd + 2, 0);
  for (int d : T.seg_depth) T.slvl_start[d + 1]++;
  for (int d = 0; d <= maxsd; ++d) T.slvl_start[d + 1] += T.slvl_start[d];
  T.slvl_segs.resize(nseg);
  T.slvl_fill.assign(maxsd + 1, 0);
  for (int s = 0; s < nseg; ++s) T.slvl_segs[T.slvl_start[T.seg_depth[s]] + T.slvl_fill[T.seg_depth[s]]++] = s;
  T.nseg = nseg; T.nsl = maxsd + 1;
  T.maxls = 1;
  for (int d = 0; d <= maxsd; ++d) T.maxls = std::max(T.maxls, T.slvl_start[d + 1] - T.slvl_start[d]);
  // segment record of the backward sweep (16 ints): positions [s0, s1) of seg_nodes, last / first node, the node before the last, the
  // last node's child count, where its children start in child_list and the first six of them -- one round trip instead of the walk
  // segment -> positions -> node -> child range -> children
  T.seg_rec.assign((size_t)nseg * 16, 0);
  for (int s = 0; s < nseg; ++s) {
    int *r = T.seg_rec.data() + (size_t)s * 16;
    const int s0 = T.seg_start[s], s1 = T.seg_start[s + 1], last = T.seg_nodes[s1 - 1];
    r[0] = s0; r[1] = s1; r[2] = last; r[3] = T.seg_nodes[s0]; r[4] = T.seg_nodes[s1 - 2 >= s0 ? s1 - 2 : s1 - 1];
    r[5] = nchild(last); r[6] = T.child_start[last];
    for (int e = 0; e < 6 && e < r[5]; ++e) r[8 + e] = T.child_list[T.child_start[last] + e];
  }
  // forward steps of the line search: the segments of a level, cut into chunks of ilqr_chunk nodes when only a few chains run
  // side by side (the other waves then price the nodes the previous step reached); wide levels stay whole
  const int chunk = (ilqr_chunk > 0 && T.maxls <= 6) ? ilqr_chunk : M;
  T.fs_start.assign(1, 0); T.fs_nstart.assign(1, 0);
  T.fs_items.clear(); T.fs_q1.clear(); T.fs_nodes.clear();
  for (int d = 0; d <= maxsd; ++d) {
    int maxlen = 0;
    for (int e = T.slvl_start[d]; e < T.slvl_start[d + 1]; ++e) { const int s = T.slvl_segs[e]; maxlen = std::max(maxlen, T.seg_start[s + 1] - T.seg_start[s]); }
    for (int k0 = 0; k0 < maxlen; k0 += chunk) {
      for (int e = T.slvl_start[d]; e < T.slvl_start[d + 1]; ++e) {
        const int s = T.slvl_segs[e], q0 = T.seg_start[s] + k0, q1 = std::min(T.seg_start[s + 1], q0 + chunk);
        if (q0 >= q1) continue;
        // item record: positions [q0, q1) of seg_nodes, its first two nodes and the first node's parent (the rollout's prologue
        // would otherwise walk q0 -> node -> parent -> state through four dependent loads)
        const int c0 = T.seg_nodes[q0], c1 = T.seg_nodes[q0 + 1 < q1 ? q0 + 1 : q1 - 1];
        for (int v : {q0, q1, c0, c1, c0 == 0 ? -1 : (int)parent[c0], 0, 0, 0}) T.fs_items.push_back(v);
        T.fs_q1.push_back(q1);
        for (int q = q0; q < q1; ++q) T.fs_nodes.push_back(T.seg_nodes[q]);
      }
      T.fs_start.push_back((int)T.fs_q1.size()); T.fs_nstart.push_back((int)T.fs_nodes.size());
    }
  }
  T.nfs = (int)T.fs_start.size() - 1;
  return -1;
}

// One device arena per call: [uploaded doubles (nd_in) | floats | ints | tree structs | constants] = ONE host->device copy of o_work bytes,
// then the doubles the kernels produce (workspace + results), then (generic mode) the materialised fields.  Offsets count elements of their
// region (doubles: below nd_in in the uploaded part, from nd_in on in the produced part), `field` bytes of the arena.
struct IlTreeOff {
  size_t us, nodew, xs, stats, trace;
  size_t relag, Fx, L, Lx, Lxx, relag2, Fx2, L2, Lx2, Lxx2;      // what the derivative pass writes, and (derivative speculator) a second set laid out alike
  size_t k, K, Vx, Vxx, xsn, usn, Ln;                            // [nslot] sets
  size_t prob, mean, cov;                                        // floats
  size_t parent, lnodes, cstart, clist, rel, rel2, lstart, sstart, snodes, slstart, slsegs, segrec, fsstart, fsitems, fsq1, fsnstart, fsnodes;      // ints
  size_t field;
};
struct IlArena {
  size_t nd = 0, nf = 0, ni = 0, nd_in = 0;
  size_t o_gx, o_gy, o_lane, o_evx, o_evu, o_quad, o_evo;        // doubles
  size_t o_scu, o_scx, o_scl, o_scj;                             // doubles of a scoring call: candidate controls (uploaded) | states, node costs, sums (produced)
  // doubles of a gains call: mu (uploaded) | k, K, dV, V_x, V_xx, nominal xs, L of all trees, J, bad_node (produced, back to back: one read-back)
  size_t o_gmu, o_gk, o_gK, o_gdv, o_gvx, o_gvxx, o_gxs, o_gl, o_gj, o_gbad;
  // doubles of a policy-rollout call: k, K, alpha, dx0 (uploaded) | nominal states per candidate block, states, controls, node costs, sums (produced)
  size_t o_pk, o_pK, o_pal, o_pdx, o_pxn, o_pxs, o_pus, o_pl, o_pj;
  size_t o_evn, o_bars, o_ctl, ctl_ints;                         // ints: queries' nodes, barrier + abort words, slot control blocks (ints per tree)
  size_t bytesIn, bytesF, bytesI, o_structs, o_consts, o_work, total;      // bytes
  std::vector<IlTreeOff> tree;
  size_t takeD(size_t n) { const size_t o = nd; nd += (n + 1) & ~(size_t)1; return o; }
  size_t takeF(size_t n) { const size_t o = nf; nf += (n + 3) & ~(size_t)3; return o; }
  size_t takeI(size_t n) { const size_t o = ni; ni += (n + 3) & ~(size_t)3; return o; }
};
// what il_layout needs to know of a call
struct IlShape {
  int W, H, n_lane_pts, nq;             // nq: queries of a cost evaluation, 0 for a solve
  int n_trees;
  const int *n_agents;                  // [n_trees] (1 in the generic mode)
  bool gen, use_exo, dev_flat;          // dev_flat: the agent arrays are read where a plan left them on the device, not uploaded
  int trace_cap;
  int n_cand = 0;                       // candidate control trees of a scoring call, 0 otherwise
  bool gains = false;                   // a gains call (k_ilqr_gains)
  int n_pol = 0, n_pol_blk = 0;         // candidates of a policy-rollout call and the workgroups they are dealt to (k_ilqr_policy), 0 otherwise
};

static void il_layout(const IlShape &s, const IlqrChoice &ch, const IlTables *tab, IlArena &A) {
  const int n_trees = s.n_trees;
  const bool spec = ch.spec != 0;
  const size_t nslot = (size_t)ch.nslot;
  A = IlArena();
  A.tree.resize(n_trees);
  const auto nodes = [tab](int t) { return tab[t].lvl_nodes.size(); };
  // the doubles region starts with everything the host uploads (grid, lane, queries, initial controls, per-node
  // weights); the workspace behind `nd_in` is produced by the kernels and never copied from the host
  A.o_gx = A.takeD(s.W); A.o_gy = A.takeD(s.H); A.o_lane = A.takeD((size_t)s.n_lane_pts * 2 + 2);
  A.o_evx = A.takeD((size_t)s.nq * 6); A.o_evu = A.takeD((size_t)s.nq * 2);
  A.o_evn = A.takeI(s.nq);
  A.o_bars = A.takeI(4 * (size_t)n_trees + 4);      // barrier words of the multi-workgroup launch + its abort word (zero at upload)
  A.ctl_ints = (sizeof(IlSlotCtl) + 15) / 16 * 4;
  A.o_ctl = A.takeI(ch.form == 2 ? A.ctl_ints * (size_t)n_trees : 0);      // (zero at upload; 16-byte aligned: the ints region is)
  for (int t = 0; t < n_trees; ++t) A.tree[t].us = A.takeD(2 * nodes(t));
  for (int t = 0; t < n_trees; ++t) A.tree[t].nodew = A.takeD(s.gen ? nodes(t) * IL_NW : 0);
  size_t Mtot = 0;
  for (int t = 0; t < n_trees; ++t) Mtot += nodes(t);
  const size_t n_sc = (size_t)s.n_cand * Mtot;      // (candidate, node) rows of a scoring call; 0 otherwise: nothing below moves
  A.o_scu = A.takeD(2 * n_sc);
  // the gains and policy requests' uploads; without them every region below is empty and nothing moves
  const size_t n_g = s.gains ? Mtot : 0, n_gt = s.gains ? (size_t)n_trees : 0, n_pm = s.n_pol > 0 ? Mtot : 0, n_po = (size_t)s.n_pol * Mtot;
  A.o_gmu = A.takeD(n_gt);
  A.o_pk = A.takeD(2 * n_pm); A.o_pK = A.takeD(12 * n_pm); A.o_pal = A.takeD((size_t)s.n_pol); A.o_pdx = A.takeD(6 * (size_t)s.n_pol);
  A.nd_in = A.nd;
  A.o_quad = A.takeD(s.gen ? 2 : (size_t)s.W * s.H); A.o_evo = A.takeD((size_t)s.nq * IL_EVAL_OUT);
  // results of all trees are contiguous (us already is: it lives in the upload region), so they come back in three copies
  for (int t = 0; t < n_trees; ++t) A.tree[t].xs = A.takeD(6 * nodes(t));
  for (int t = 0; t < n_trees; ++t) A.tree[t].stats = A.takeD(2 * IL_NSTAT);
  for (int t = 0; t < n_trees; ++t) {
    IlTreeOff &L = A.tree[t];
    const size_t M = nodes(t), a = (size_t)s.n_agents[t];
    L.trace = A.takeD((size_t)2 * s.trace_cap * IL_TRACE_W);
    L.relag = A.takeD(s.use_exo ? M * IL_RA : 0); L.Fx = A.takeD(36 * M); L.L = A.takeD(M); L.Lx = A.takeD(6 * M); L.Lxx = A.takeD(36 * M);
    L.relag2 = A.takeD(spec && s.use_exo ? M * IL_RA : 0); L.Fx2 = A.takeD(spec ? 36 * M : 0); L.L2 = A.takeD(spec ? M : 0); L.Lx2 = A.takeD(spec ? 6 * M : 0);
    L.Lxx2 = A.takeD(spec ? 36 * M : 0);
    L.k = A.takeD(nslot * 2 * M); L.K = A.takeD(nslot * 12 * M); L.Vx = A.takeD(nslot * 6 * M); L.Vxx = A.takeD(nslot * 36 * M);
    L.xsn = A.takeD(nslot * 60 * M); L.usn = A.takeD(nslot * 20 * M); L.Ln = A.takeD(nslot * 10 * M);
    L.prob = A.takeF(M); L.mean = A.takeF(s.dev_flat ? 0 : M * a * 2); L.cov = A.takeF(s.dev_flat ? 0 : M * a);
    L.parent = A.takeI(M); L.lnodes = A.takeI(M); L.cstart = A.takeI(M + 1); L.clist = A.takeI(M); L.rel = A.takeI(M); L.rel2 = A.takeI(spec ? M : 0);
  }
  for (int t = 0; t < n_trees; ++t) {
    IlTreeOff &L = A.tree[t];
    const IlTables &T = tab[t];
    L.lstart = A.takeI(T.lvl_start.size());
    L.sstart = A.takeI(T.seg_start.size()); L.snodes = A.takeI(nodes(t)); L.slstart = A.takeI(T.slvl_start.size()); L.slsegs = A.takeI(T.slvl_segs.size());
    L.segrec = A.takeI(T.seg_rec.size());
    L.fsstart = A.takeI(T.fs_start.size()); L.fsitems = A.takeI(T.fs_items.size()); L.fsq1 = A.takeI(T.fs_q1.size());
    L.fsnstart = A.takeI(T.fs_nstart.size()); L.fsnodes = A.takeI(nodes(t));
  }
  A.o_scx = A.takeD(6 * n_sc); A.o_scl = A.takeD(n_sc); A.o_scj = A.takeD((size_t)s.n_cand * n_trees);
  A.o_gk = A.takeD(2 * n_g); A.o_gK = A.takeD(12 * n_g); A.o_gdv = A.takeD(n_g); A.o_gvx = A.takeD(6 * n_g); A.o_gvxx = A.takeD(36 * n_g);
  A.o_gxs = A.takeD(6 * n_g); A.o_gl = A.takeD(n_g); A.o_gj = A.takeD(n_gt); A.o_gbad = A.takeD(n_gt);
  A.o_pxn = A.takeD(6 * (size_t)s.n_pol_blk * n_pm); A.o_pxs = A.takeD(6 * n_po); A.o_pus = A.takeD(2 * n_po); A.o_pl = A.takeD(n_po);
  A.o_pj = A.takeD((size_t)s.n_pol * (s.n_pol > 0 ? n_trees : 0));
  A.bytesIn = A.nd_in * sizeof(double); A.bytesF = A.nf * sizeof(float); A.bytesI = A.ni * sizeof(int);
  A.o_structs = A.bytesIn + A.bytesF + A.bytesI;
  A.o_consts = (A.o_structs + (size_t)n_trees * sizeof(IlqrTreeDev) + 15) & ~(size_t)15;
  A.o_work = (A.o_consts + 2 * sizeof(IlqrConst) + 15) & ~(size_t)15;
  A.total = (A.o_work + (A.nd - A.nd_in) * sizeof(double) + 15) & ~(size_t)15;
  for (int t = 0; t < n_trees; ++t) {
    A.tree[t].field = A.total;
    if (s.gen) A.total += nodes(t) * s.W * s.H * sizeof(double);
  }
}

// one tree's tables into the image of the ints region (hI: IlArena::ni ints)
static void il_stage_ints(const IlTreeOff &L, const int32_t *parent, const IlTables &T, int *hI) {
  const auto put = [hI](size_t o, const std::vector<int> &v) { if (!v.empty()) memcpy(hI + o, v.data(), v.size() * sizeof(int)); };
  memcpy(hI + L.parent, parent, T.lvl_nodes.size() * sizeof(int));
  put(L.lstart, T.lvl_start); put(L.lnodes, T.lvl_nodes); put(L.cstart, T.child_start); put(L.clist, T.child_list);
  put(L.sstart, T.seg_start); put(L.snodes, T.seg_nodes); put(L.slstart, T.slvl_start); put(L.slsegs, T.slvl_segs); put(L.segrec, T.seg_rec);
  put(L.fsstart, T.fs_start); put(L.fsitems, T.fs_items); put(L.fsq1, T.fs_q1); put(L.fsnstart, T.fs_nstart); put(L.fsnodes, T.fs_nodes);
}
