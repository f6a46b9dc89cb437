// What mind_aime_plan decides without a device: the internal scenario tree (AimeBook: create_nodes, decide_branch, get_branch_time and the
// first step of get_scenario_tree, planners/mind/scenario_tree.py, restated over plain arrays; the cost trees flattened as
// trajectory_tree.py's flatten_scenario_tree does), the sharding arithmetic (pl_block, pl_owner, pl_route), the chunk size of a round
// (pl_chunk), the job tables of the two packing kernels (JobTable) and the two buffer layouts (RootLayout, InLayout).  No HIP call, no
// context: aime_plan.hip's stages switch on these records; tests read them through mind_debug_aime_book.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mind_hip.h"

constexpr int PL_K = 6;        // modes per scene (AIME_K)
constexpr int PL_OBS = 50;     // history window (RB_T)

struct PlScene {            // an observation pushed through the predictor: the root or a re-based branch node
  int node;                 // internal tree node it belongs to (0 = root)
  float prob;
  int cur_t, end_t;
  float rot[4], orig[2], tgt[22];
};

struct PlNode {
  int round, scene, mode, parent, depth;
  int owner, lscene;        // sharded: the rank whose pl_world[round] holds the node's predicted rows, its scene index there
  float prob;
  int cur_t, end_t;
  bool branch, end, term, rebased;
  unsigned long long hit;   // bit t: some agent's sigma at predicted step t > 9 x its sigma at the compare step
  float tgt[22];
};

// contiguous block [lo, hi) of n items for rank r of w (the first ranks take the remainder: parallel.Shard.block)
inline void pl_block(int n, int r, int w, int &lo, int &hi) {
  const int base = n / w, rem = n % w;
  lo = r * base + (r < rem ? r : rem);
  hi = lo + base + (r < rem ? 1 : 0);
}
inline int pl_owner(int n, int w, int b) {
  for (int r = 0; r < w; ++r) { int lo, hi; pl_block(n, r, w, lo, hi); if (b >= lo && b < hi) return r; }
  return w - 1;
}

// do the exchanges of a sharded plan run?  (a transport is set and the group has several ranks, or one rank forced: mind_set_exchange)
inline bool pl_exchanges(bool have_transport, int world, bool force) { return have_transport && (world > 1 || force); }

// scenes per predictor call of a round of Bk scenes: the whole round unless its edge tensor would exceed the budget ("plan_chunk_mb")
inline int pl_chunk(int n_tokens, int bytes_per_pair, int plan_chunk_mb, int Bk) {
  const double edge_mb = (double)n_tokens * (((n_tokens + 15) / 16) * 16) * bytes_per_pair / (1024.0 * 1024.0);
  return std::max(1, (int)std::min<double>((double)(Bk > 0 ? Bk : 1), (double)plan_chunk_mb / edge_mb));
}

// The bounded wait for a word the device stores when a round's mirrored decisions are complete (k_aime_select_branch / k_aime_branch): acquire
// loads until the word holds `want`; the clock (seconds, any origin) is read every `spins_per_look` misses, and past `timeout_s` the wait gives
// up -- the caller then drains the stream and reads the same bytes (never hang on a word).  true: the word arrived.
typedef double (*pl_clock_fn)(void *user);
inline bool pl_wait_word(const volatile unsigned *word, unsigned want, double timeout_s, pl_clock_fn now, void *user, unsigned spins_per_look) {
  if (__atomic_load_n((const unsigned *)word, __ATOMIC_ACQUIRE) == want) return true;
  const double t0 = now(user);
  for (unsigned spins = 0;;) {
    if (__atomic_load_n((const unsigned *)word, __ATOMIC_ACQUIRE) == want) return true;
    if (++spins < spins_per_look) continue;
    spins = 0;
    if (now(user) - t0 > timeout_s) return false;
  }
}

// a "left to the host path" exit of the bookkeeping: which one and the numbers its message names (pl_err_format: the caller's fail() prints it)
enum { PL_OK = 0, PL_E_ROUNDS, PL_E_ROOT, PL_E_TRIMMED, PL_E_AGAIN, PL_E_ORDER, PL_E_NO_END };
struct PlErr { int code = PL_OK, a0 = 0, a1 = 0; explicit operator bool() const { return code != PL_OK; } };
inline const char *pl_err_format(int code) {
  switch (code) {
    case PL_E_ROUNDS: return "unsupported: more than %d AIME rounds";
    case PL_E_ROOT: return "unsupported: the root is a branching candidate";
    case PL_E_TRIMMED: return "unsupported: branch time of a trimmed node with CUR_T > 0";
    case PL_E_AGAIN: return "unsupported: a node of round %d is expanded again in round %d";
    case PL_E_ORDER: return "unsupported: branch set out of scene order";
    case PL_E_NO_END: return "unsupported: no end node found in the scenario tree";
  }
  return "";
}

// offsets (floats, each array on a 4-float boundary) of the two device layouts
struct PlTake { size_t o = 0; size_t operator()(size_t n) { const size_t r = o; o += (n + 3) & ~(size_t)3; return r; } };
struct RootLayout {       // the root upload; raw (device-built root): raw windows / pad flags / lane polylines go up, the slots before `types` are filled by kernels
  size_t actors, ctrs, vecs, lanes, lc, lv, tn, tr, cov, types, tl, ti, wpos, wang, wvel, fr, rpos, rang, rvel, rpad, lpts, lfl, total;
  RootLayout(size_t a, size_t l, size_t P, bool raw) {
    PlTake take;
    actors = take(a * 14 * 48); ctrs = take(a * 2); vecs = take(a * 2); lanes = take(l * 160);
    lc = take(l * 2); lv = take(l * 2); tn = take(160); tr = take(20); cov = take(a);
    types = take(a * PL_OBS * 7); tl = take(P * 2); ti = take(P * 12);
    wpos = take(a * PL_OBS * 2); wang = take(a * PL_OBS); wvel = take(a * PL_OBS * 2);
    fr = take(28); rpos = take(raw ? a * PL_OBS * 2 : 0); rang = take(raw ? a * PL_OBS : 0);
    rvel = take(raw ? a * PL_OBS * 2 : 0); rpad = take(raw ? a * PL_OBS : 0);
    lpts = take(raw ? l * 11 * 2 * 2 : 0); lfl = take(raw ? l * 6 : 0);      // doubles (2 floats each), ints
    total = take.o;
  }
};
struct InLayout {         // one re-based input set of S scenes: actors | actor_ctrs | actor_vecs | lane_ctrs | lane_vecs | tgt_nodes | tgt_rpe | frames | cov_last
  size_t actors, ctrs, vecs, lc, lv, tn, tr, fr, cov, total;
  InLayout(size_t S, size_t a, size_t l) {
    PlTake take;
    actors = take(S * a * 14 * 48); ctrs = take(S * a * 2); vecs = take(S * a * 2); lc = take(S * l * 2); lv = take(S * l * 2);
    tn = take(S * 160); tr = take(S * 20); fr = take(S * 28); cov = take(S * a); total = take.o;
  }
};

// Who sends which scenes of the next round to whom: rank j re-based the scenes [s0_r[j], s0_r[j] + cnt_r[j]), rank k's block of the S scenes
// consumes them.  snd / rcv [world][2]: the scene range this rank sends to / receives from every rank; tab [2][world]: the same in bytes (the
// all-to-all's table); any: scenes that travel on ANY rank (every rank computes the same number: a round with none is skipped by all of them)
struct PlRoute {
  std::vector<int64_t> tab;
  std::vector<int> snd, rcv;
  long long any = 0;
};
inline void pl_route(int S, int world, int rank, const std::vector<int> &cnt_r, const std::vector<int> &s0_r, size_t per_scene, bool self_too, PlRoute &q) {
  q.tab.assign(2 * (size_t)world, 0); q.snd.assign(2 * (size_t)world, 0); q.rcv.assign(2 * (size_t)world, 0);
  q.any = 0;
  for (int j = 0; j < world; ++j)
    for (int k = 0; k < world; ++k) {
      if (j == k && !self_too) continue;
      int klo, khi;
      pl_block(S, k, world, klo, khi);
      const int i0 = std::max(s0_r[j], klo), i1 = std::max(i0, std::min(s0_r[j] + cnt_r[j], khi));      // scenes rank j produced that rank k consumes
      q.any += i1 - i0;
      const int64_t bytes = (int64_t)(i1 - i0) * (int64_t)per_scene * (int64_t)sizeof(float);
      if (j == rank) { q.tab[k] = bytes; q.snd[2 * k] = i0; q.snd[2 * k + 1] = i1; }
      if (k == rank) { q.tab[(size_t)world + j] = bytes; q.rcv[2 * j] = i0; q.rcv[2 * j + 1] = i1; }
    }
}

// The table of one packing kernel (k_aime_gather / k_aime_flat): jobs (AimeGather / AimeFlat: four ints), per job the round whose world buffer
// holds its rows (pack() writes that buffer's address), per workgroup its job and agent.  Device image: jobs | addresses | job of block | agent of block,
// each on a 16-byte boundary
struct PlJob { int row0, n, dst, a; };
struct JobTable {
  std::vector<PlJob> jobs;
  std::vector<int> world, job_of_block, agent_of_block;
  static size_t al(size_t n) { return (n + 15) & ~(size_t)15; }
  void clear() { jobs.clear(); world.clear(); job_of_block.clear(); agent_of_block.clear(); }
  void add(const PlJob &j, int round) {
    for (int e = 0; e < j.a; ++e) { job_of_block.push_back((int)jobs.size()); agent_of_block.push_back(e); }
    jobs.push_back(j); world.push_back(round);
  }
  size_t off_world() const { return al(jobs.size() * sizeof(PlJob)); }
  size_t off_job() const { return off_world() + al(jobs.size() * sizeof(float *)); }
  size_t off_agent() const { return off_job() + al(job_of_block.size() * sizeof(int)); }
  size_t bytes() const { return off_agent() + al(job_of_block.size() * sizeof(int)); }
  void pack(char *dst, const float *const *world_of_round) const {
    if (jobs.empty()) return;
    memcpy(dst, jobs.data(), jobs.size() * sizeof(PlJob));
    const float **w = (const float **)(dst + off_world());
    for (size_t i = 0; i < jobs.size(); ++i) w[i] = world_of_round[world[i]];
    memcpy(dst + off_job(), job_of_block.data(), job_of_block.size() * sizeof(int));
    memcpy(dst + off_agent(), agent_of_block.data(), agent_of_block.size() * sizeof(int));
  }
};

struct PlGeom { int B, lo, hi, Bk, Bmax; };     // a round: its scenes, this rank's block [lo, hi) of them, the largest block (the decision buffers are laid out for it)

// what a round's decisions made of the tree: the branch set and who re-bases it
struct PlRound {
  std::vector<int> todo;             // branching nodes in leaf order = the next round's scenes
  std::vector<int> cnt_r, s0_r;      // per rank: the children of ITS scenes are the contiguous range [s0_r, s0_r + cnt_r) of the next round's scenes
  std::vector<int> win;              // k_aime_windows' three ints per child of this rank: [Sm parent scenes | Sm first rows | Sm steps kept]
  int S = 0, s0 = 0, Sm = 0;         // the branch set's size, this rank's range of it
};

struct AimeBook {
  int HZ = 0, max_depth = 0, a = 0, XW = 1, XR = 0;
  bool dist = false;                 // exchanges run (a forced one-rank group included)
  int n_rounds = 0;
  std::vector<PlNode> nodes;         // [0] = the root
  std::vector<int> leaves;
  std::vector<PlScene> batch;        // the scenes of the round that runs next
  PlRound rec;
  // results (finish)
  std::vector<mind_aime_node> table;
  int64_t n_rows = 0;
  JobTable gather, flat;
  std::vector<int32_t> tree_top, tree_off, flat_parent;
  std::vector<float> flat_prob;
  // scratch, kept between plans: a plan allocates nothing in steady state
  std::vector<int> cand, queue, last, stack;
  std::vector<std::vector<int>> kids;
  std::vector<float> pr;

  AimeBook() {}
  AimeBook(int pred_len, int max_depth_, int n_agents, int world, int rank, bool dist_) { reset(pred_len, max_depth_, n_agents, world, rank, dist_); }

  // internal tree (scenario_tree.py:60-67): root = node 0, a leaf with branch_flag; the previous plan's cost trees are gone
  void reset(int pred_len, int max_depth_, int n_agents, int world, int rank, bool dist_) {
    HZ = pred_len; max_depth = max_depth_; a = n_agents; XW = world; XR = rank; dist = dist_;
    n_rounds = 0;
    nodes.assign(1, PlNode());
    PlNode &r = nodes[0];
    memset(&r, 0, sizeof(r));
    r.round = -1; r.parent = -1; r.prob = 1.f; r.end_t = HZ; r.branch = true;
    leaves.assign(1, 0);
    batch.assign(1, PlScene());
    PlScene &s = batch[0];
    s.node = 0; s.prob = 1.f; s.cur_t = 0; s.end_t = HZ;
    tree_top.clear();
  }

  PlErr begin_round(int max_rounds, PlGeom &g) const {
    PlErr e;
    if (n_rounds >= max_rounds) { e.code = PL_E_ROUNDS; e.a0 = max_rounds; return e; }
    g.B = (int)batch.size();
    pl_block(g.B, XR, XW, g.lo, g.hi);
    g.Bk = g.hi - g.lo;
    g.Bmax = (g.B + XW - 1) / XW;
    return e;
  }

  static int flags_of(const PlNode &n) { return (n.branch ? MIND_AIME_BRANCH : 0) | (n.end ? MIND_AIME_END : 0) | (n.term ? MIND_AIME_TERMINATE : 0); }
  int root_flags() const { return flags_of(nodes[0]); }

  // One round's decisions, h_dec = [ranks][sel Bmax x 6 | sel_prob Bmax x 6 | hit Bmax x 6 x 2] (one rank's worth when no exchange runs):
  // create_nodes, decide_branch, the branch-time scan -> rec; batch becomes the branch set (empty rec.todo: the tree is complete)
  PlErr round(const float *h_dec, int Bmax) {
    PlErr err;
    const int B = (int)batch.size(), round = n_rounds;
    const size_t n_back = (size_t)Bmax * 6 * 4;
    // ---- create_nodes (scenario_tree.py:73-80): the kept modes scene by scene, visiting order within a scene
    for (int b = 0; b < B; ++b) {
      const int owner = dist ? pl_owner(B, XW, b) : 0;
      int olo, ohi;
      pl_block(B, owner, XW, olo, ohi);
      if (!dist) { olo = 0; }
      const float *h_sel = h_dec + (size_t)owner * n_back, *h_selp = h_sel + (size_t)Bmax * 6;
      const unsigned *h_hit = (const unsigned *)(h_selp + (size_t)Bmax * 6);
      const int bl = b - olo;
      for (int j = 0; j < PL_K; ++j) {
        const int k = (int)h_sel[(size_t)bl * 6 + j];
        if (k < 0) continue;
        PlNode n;
        memset(&n, 0, sizeof(n));
        n.round = round; n.scene = b; n.mode = k; n.parent = batch[b].node; n.depth = nodes[n.parent].depth + 1;
        n.owner = owner; n.lscene = bl;
        n.prob = h_selp[(size_t)bl * 6 + j]; n.cur_t = batch[b].cur_t; n.end_t = batch[b].end_t;
        n.hit = (unsigned long long)h_hit[2 * ((size_t)bl * 6 + j)] | ((unsigned long long)h_hit[2 * ((size_t)bl * 6 + j) + 1] << 32);
        memcpy(n.tgt, batch[b].tgt, sizeof(n.tgt));
        const int idx = (int)nodes.size();
        nodes.push_back(n);
        for (size_t q = 0; q < leaves.size(); ++q)
          if (leaves[q] == n.parent) { leaves.erase(leaves.begin() + q); break; }
        leaves.push_back(idx);
      }
    }
    n_rounds += 1;
    // ---- decide_branch (scenario_tree.py:82-100) over the leaves in insertion order
    std::vector<int> &todo = rec.todo;
    cand.clear(); todo.clear();
    for (int li : leaves) {
      PlNode &n = nodes[li];
      if (n.branch) { n.branch = false; n.term = true; }
      else if (!n.end) {
        if (n.depth >= max_depth) n.term = true;
        else cand.push_back(li);
      }
    }
    for (int li : cand) {
      PlNode &n = nodes[li];
      if (li == 0) { err.code = PL_E_ROOT; return err; }
      // get_branch_time (:592-611): first even t in (CUR_T, END_T) whose sigma ratio exceeds 9.  A node that was re-based before and
      // has CUR_T > 0 would index past its trimmed history in the reference: left to the host path.
      if (n.rebased && n.cur_t > 0) { err.code = PL_E_TRIMMED; return err; }
      int t_b = n.end_t;
      for (int t = n.cur_t + 1 + (n.cur_t + 1) % 2; t < n.end_t; t += 2)
        if ((n.hit >> t) & 1ull) { t_b = t; break; }
      if (t_b < n.end_t) n.end_t = t_b;
      if (t_b < HZ) todo.push_back(li);
      else n.end = true;
    }
    const int S = rec.S = (int)todo.size();
    rec.cnt_r.assign(XW, 0); rec.s0_r.assign(XW + 1, 0); rec.win.clear();
    rec.s0 = rec.Sm = 0;
    if (todo.empty()) return err;
    // ---- update_obser (:467-567) of the branching nodes happens on the device.  Sharded: a rank re-bases the children of ITS scenes (the
    //      parent windows and the predicted rows are there); the branch set is in leaf order = parent-scene order, so a rank's children are
    //      one contiguous range [s0, s0 + Sm) of the next round's scenes
    for (int li : todo)
      if (nodes[li].round != round) { err.code = PL_E_AGAIN; err.a0 = nodes[li].round; err.a1 = round + 1; return err; }
    for (int s = 0; s < S; ++s) {
      // (cannot fire: the nodes of a round are created scene by scene and all of `todo` are this round's -- kept as the one-function form's guard)
      if (s > 0 && nodes[todo[s]].scene < nodes[todo[s - 1]].scene) { err.code = PL_E_ORDER; return err; }
      rec.cnt_r[nodes[todo[s]].owner] += 1;
    }
    for (int r = 0; r < XW; ++r) rec.s0_r[r + 1] = rec.s0_r[r] + rec.cnt_r[r];
    const int s0 = rec.s0 = rec.s0_r[XR], Sm = rec.Sm = rec.cnt_r[XR];
    rec.win.resize(3 * (size_t)Sm);
    for (int s = 0; s < Sm; ++s) {
      const PlNode &n = nodes[todo[s0 + s]];
      rec.win[s] = n.scene;                                  // parent window: the scene of this round the node was predicted from (global index)
      rec.win[Sm + s] = n.lscene * a * PL_K + n.mode;        // first row (agent 0) of the node's mode in this rank's world rows
      rec.win[2 * Sm + s] = n.end_t - n.cur_t;               // steps kept
    }
    // next round's batch = the branch set in leaf order (scenario_tree.py:102-108)
    batch.assign(S, PlScene());
    for (int s = 0; s < S; ++s) {
      PlNode &n = nodes[todo[s]];
      n.branch = true; n.rebased = true;
      PlScene &sc = batch[s];
      sc.node = todo[s]; sc.prob = n.prob; sc.cur_t = n.end_t; sc.end_t = HZ;
    }
    return err;
  }

  // get_scenario_tree, first step (:208-216): every node on a finished branch is labelled; the node table; the jobs that pack their rows; the
  // cost trees of the finished branches, flattened as TrajectoryTreeOptimizer would (trajectory_tree.py:19-124 / get_scenario_tree :208-272):
  // sibling-normalised probabilities, LIFO depth-first creation order, every even step = one trajectory node
  PlErr finish() {
    PlErr err;
    bool any_end = false;
    for (int li : leaves) any_end |= nodes[li].end;
    if (!any_end) { err.code = PL_E_NO_END; return err; }
    for (int li : leaves) {
      if (!nodes[li].end) continue;
      for (int q = li; q > 0; q = nodes[q].parent) nodes[q].end = true;
    }
    const int N = (int)nodes.size() - 1;
    table.assign(N, mind_aime_node());
    gather.clear(); flat.clear();
    n_rows = 0;
    for (int i = 0; i < N; ++i) {
      const PlNode &n = nodes[i + 1];
      mind_aime_node &p = table[i];
      p.round = n.round; p.scene = n.scene; p.mode = n.mode; p.parent = n.parent - 1; p.prob = n.prob; p.cur_t = n.cur_t; p.end_t = n.end_t;
      p.flags = flags_of(n);
      memcpy(p.tgt_pts, n.tgt, sizeof(p.tgt_pts));
      p.dur = 0; p.row_off = -1;
      if (n.end) {
        const int dur = n.end_t - n.cur_t;
        p.dur = dur; p.row_off = n_rows;
        if (dur > 0 && (!dist || n.owner == XR))             // (sharded: the rank that holds the node's predicted rows packs them)
          gather.add({n.lscene * a * PL_K + n.mode, dur, (int)n_rows, a}, n.round);
        n_rows += (int64_t)a * dur * 3;
      }
    }
    if (kids.size() < nodes.size()) kids.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) kids[i].clear();
    for (int i = 1; i < (int)nodes.size(); ++i) kids[nodes[i].parent].push_back(i);
    tree_top.clear(); tree_off.assign(1, 0); flat_parent.clear(); flat_prob.clear();
    for (int top : kids[0]) {
      if (!nodes[top].end) continue;
      // probabilities: breadth-first renormalisation over the siblings that lie on finished branches
      // (float32 throughout: SCEN_PROB is a float32 scalar and the Python literals 0.0 / 1.0 it meets are weak scalars under numpy >= 2,
      // which is what the host path -- pinned against the reference's sibling probabilities in tests/golden/aime.npz -- computes with)
      pr.assign(nodes.size(), 0.f);
      pr[top] = 1.f;
      queue.assign(1, top);
      for (size_t qh = 0; qh < queue.size(); ++qh) {
        const int cur = queue[qh];
        float total = 0.f;
        for (int ch : kids[cur]) if (nodes[ch].end) total = total + nodes[ch].prob;
        for (int ch : kids[cur]) if (nodes[ch].end) { pr[ch] = nodes[ch].prob / total * pr[cur]; queue.push_back(ch); }
      }
      // flatten: stack pop() = the last child first; a node's trajectory nodes are chained, the first hangs off its parent's last
      const int base = tree_off.back();
      int count = 0;
      last.assign(nodes.size(), -1); stack.assign(1, top);
      while (!stack.empty()) {
        const int q = stack.back();
        stack.pop_back();
        const PlNode &n = nodes[q];
        const int dur = n.end_t - n.cur_t, nn = (dur + 1) / 2;
        const int up = q == top ? -1 : last[n.parent];
        if (nn > 0) {
          for (int m = 0; m < nn; ++m) {
            flat_parent.push_back(m == 0 ? up : count + m - 1);
            flat_prob.push_back(pr[q]);
          }
          if (!dist || n.owner == XR) flat.add({n.lscene * a * PL_K + n.mode, nn, base + count, a}, n.round);
          count += nn;
          last[q] = count - 1;
        } else {
          last[q] = up;
        }
        for (int ch : kids[q]) if (nodes[ch].end) stack.push_back(ch);
      }
      tree_top.push_back(top - 1);
      tree_off.push_back(base + count);
    }
    return err;
  }
};
