"""mind_aime_plan's bookkeeping (mind_amd/csrc/aime_book.h) on the host -- no GPU needed.

mind_debug_aime_book replays AimeBook / pl_route / pl_chunk, the functions the plan itself calls, over a stream of per-round decision words
(sel | sel_prob | hit, as k_aime_select / k_aime_branch write them).  Hand-written streams are checked against tables written out here, seeded
random streams against the project's own Python host rules (planners/basic/tree.py, ScenarioTreeGenerator.decide_branch /
_scenario_trees_from_tree, trajectory_tree.flatten_scenario_tree), the sharding arithmetic against parallel.Shard.block and against itself.

Two cases cannot be built from decision words and are therefore not here: a CUR_T of odd parity (a CUR_T is 0 or a branch time, and branch
times are even) and the exit "branch set out of scene order" (the nodes of a round are created scene by scene and a branch set that holds a node
of an earlier round leaves through "expanded again" first).  The exit "the root is a branching candidate" needs a round after an empty branch
set, where the plan has stopped; the replay goes on while rounds are given."""
from types import SimpleNamespace

import numpy as np
import pytest

from mind_amd._lib import aime_book
from mind_amd.parallel import Shard
from mind_amd.planners.basic.tree import Node, Tree
from mind_amd.planners.mind.scenario_tree import ScenarioData, ScenarioTreeGenerator
from mind_amd.planners.mind.trajectory_tree import flatten_scenario_tree

BRANCH, END, TERM = 1, 2, 4
A = 3                   # agents per scene


def block(n, r, w):
    return Shard.block(SimpleNamespace(rank=r, world=w), n)


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def pack(scenes, world=1, dist=False):
    """the decision words of a round: per scene a list of up to six kept modes (mode, prob, hit bits) in visiting order"""
    B, ranks, Bmax = len(scenes), world if dist else 1, -(-len(scenes) // world)
    out = np.zeros((ranks, 24 * Bmax), np.float32)
    for r in range(ranks):
        lo, hi = block(B, r, world) if dist else (0, B)
        sel, selp, hit = np.full((Bmax, 6), -1, np.float32), np.zeros((Bmax, 6), np.float32), np.zeros((Bmax, 6, 2), np.uint32)
        for b in range(lo, hi):
            for j, (k, p, h) in enumerate(scenes[b]):
                sel[b - lo, j], selp[b - lo, j], hit[b - lo, j] = k, p, (h & 0xffffffff, h >> 32)
        out[r] = np.concatenate([sel.ravel(), selp.ravel(), hit.ravel().view(np.float32)])
    return out


def node(d, i):
    n = d["nodes"][i]
    return (n["round"], n["scene"], n["mode"], n["parent"], n["cur_t"], n["end_t"], n["flags"], n["dur"], n["row_off"])


def chain(n, up=-1, at=0):
    return [up] + list(range(at, at + n - 1))


ONE = [(0, .5, 0)]         # a scene that keeps one mode, which ends


def br(t, k=0):
    """a kept mode k that branches at step t"""
    return [(k, .5, 1 << t)]


# ---- hand-written streams ----------------------------------------------------------------------------------------------------------------
def test_one_round_nothing_branches():
    d = aime_book(50, 3, A, [pack([[(2, .6, 0), (0, .3, 0)]])])
    assert d["error"] is None and d["root_flags"] == BRANCH and len(d["rounds"]) == 1
    r = d["rounds"][0]
    assert (r["B"], r["lo"], r["hi"], r["Bmax"], r["S"], r["Sm"]) == (1, 0, 1, 1, 0, 0) and r["todo"] == [] and r["win"] == []
    assert [node(d, i) for i in range(2)] == [(0, 0, 2, -1, 0, 50, END, 50, 0), (0, 0, 0, -1, 0, 50, END, 50, A * 50 * 3)]
    assert [n["prob"] for n in d["nodes"]] == [f32bits(.6), f32bits(.3)]
    assert d["n_rows"] == 2 * A * 50 * 3
    assert d["gather"]["jobs"] == [(2, 50, 0, A, 0), (0, 50, A * 50 * 3, A, 0)]
    assert d["gather"]["job_of_block"] == [0] * A + [1] * A and d["gather"]["agent_of_block"] == list(range(A)) * 2
    assert d["tree_top"] == [0, 1] and d["tree_off"] == [0, 25, 50]
    assert d["flat_parent"] == chain(25) * 2 and d["flat_prob"] == [f32bits(1.0)] * 50
    assert d["flat"]["jobs"] == [(2, 25, 0, A, 0), (0, 25, 25, A, 0)]
    # device image of a job table: jobs | addresses | job of block | agent of block, each on a 16-byte boundary
    assert d["flat"]["bytes"] == 2 * 16 + 2 * 8 + 2 * 32


def test_one_mode_branches_at_an_even_step_the_other_ends():
    d = aime_book(50, 3, A, [pack([[(1, .5, 1 << 4), (3, .25, 0)]]), pack([[(0, .125, 0)]])])
    assert d["error"] is None and len(d["rounds"]) == 2
    r0, r1 = d["rounds"]
    assert r0["todo"] == [1] and r0["cnt_r"] == [1] and r0["s0_r"] == [0, 1] and r0["win"] == [0, 1, 4]      # parent scene, first row, steps kept
    assert (r1["B"], r1["S"]) == (1, 0)
    assert [node(d, i) for i in range(3)] == [(0, 0, 1, -1, 0, 4, BRANCH | END, 4, 0), (0, 0, 3, -1, 0, 50, END, 50, A * 4 * 3),
                                               (1, 0, 0, 0, 4, 50, END, 46, A * 54 * 3)]
    assert d["tree_top"] == [0, 1] and d["tree_off"] == [0, 25, 50]
    assert d["flat_parent"] == chain(25) + chain(25)
    # sibling-normalised: the only finished child of node 0 takes its whole probability
    assert d["flat_prob"] == [f32bits(1.0)] * 50
    assert d["flat"]["jobs"] == [(1, 2, 0, A, 0), (0, 23, 2, A, 1), (3, 25, 25, A, 0)]


def test_siblings_are_flattened_last_child_first_with_float32_probabilities():
    p1, p2 = np.float32(.3), np.float32(.2)
    d = aime_book(50, 3, A, [pack([[(1, .5, 1 << 4)]]), pack([[(0, p1, 0), (5, p2, 0)]])])
    tot = np.float32(0) + p1 + p2
    assert d["tree_off"] == [0, 48] and d["flat_parent"] == chain(2) + chain(23, 1, 2) + chain(23, 1, 25)
    assert d["flat_prob"] == [f32bits(1)] * 2 + [f32bits(p2 / tot * np.float32(1))] * 23 + [f32bits(p1 / tot * np.float32(1))] * 23
    assert d["flat"]["jobs"] == [(1, 2, 0, A, 0), (5, 23, 2, A, 1), (0, 23, 25, A, 1)]


def test_a_leaf_at_max_depth_terminates():
    d = aime_book(50, 2, A, [pack([[(1, .5, 1 << 4), (3, .25, 0)]]), pack([[(0, .125, 1 << 10)]])])
    assert d["error"] is None and d["rounds"][1]["todo"] == []
    assert [node(d, i) for i in range(3)] == [(0, 0, 1, -1, 0, 4, BRANCH, 0, -1), (0, 0, 3, -1, 0, 50, END, 50, 0), (1, 0, 0, 0, 4, 50, TERM, 0, -1)]
    assert d["tree_top"] == [1] and d["tree_off"] == [0, 25]


@pytest.mark.parametrize("hit", [1 << 3, 1 << 4, 1 << 2, 1 << 5, (1 << 3) | (1 << 4) | (1 << 5) | (1 << 50)])
def test_no_branch_time_from_odd_bits_or_bits_up_to_cur_t(hit):
    """the second round's node has CUR_T 4: bits 2, 3, 4, the bit at CUR_T + 1 and a bit at END_T are no branch time"""
    d = aime_book(50, 3, A, [pack([[(1, .5, 1 << 4)]]), pack([[(0, .125, hit)]])])
    assert d["rounds"][1]["todo"] == [] and node(d, 1) == (1, 0, 0, 0, 4, 50, END, 46, A * 4 * 3)


def test_the_bit_at_cur_t_plus_one_and_the_first_even_step_behind_it():
    for cur_t in (0, 4):
        first = [] if cur_t == 0 else [pack([[(1, .5, 1 << 4)]])]
        d = aime_book(50, 3, A, first + [pack([[(0, .125, 1 << (cur_t + 1))]])])
        assert d["rounds"][-1]["todo"] == [] and node(d, len(first))[4:7] == (cur_t, 50, END)
        d = aime_book(50, 4, A, first + [pack([[(0, .125, 3 << (cur_t + 1))]]), pack([ONE])])
        assert d["rounds"][len(first)]["todo"] == [len(first) + 1] and node(d, len(first))[4:6] == (cur_t, cur_t + 2)


def test_a_bit_in_the_second_word():
    d = aime_book(50, 3, A, [pack([[(1, .5, 1 << 40), (2, .25, 1 << 49)]]), pack([[(0, .125, 1 << 49)]])])
    r0 = d["rounds"][0]
    assert r0["todo"] == [1] and r0["win"] == [0, 1, 40]            # bit 49 is odd
    assert node(d, 0)[4:6] == (0, 40) and node(d, 1)[4:7] == (0, 50, END) and node(d, 2)[4:7] == (40, 50, END)
    d = aime_book(60, 3, A, [pack([[(1, .5, 1 << 58), (2, .25, 1 << 32)]])])
    assert d["rounds"][0]["todo"] == [1, 2] and d["rounds"][0]["win"] == [0, 0, 1, 2, 58, 32]


# ---- the "unsupported" exits: left to the Python path, which matches on the prefix --------------------------------------------------------
@pytest.mark.parametrize("rounds, kw, message", [
    ([pack([[]]), pack([[]])], {}, "unsupported: the root is a branching candidate"),
    # C (CUR_T 4) branches and keeps no mode; two rounds on, with the other branch still growing, it is a candidate again
    ([pack([br(4) + br(4, 1)]), pack([br(10), br(10)]), pack([[], br(20)]), pack([br(30)]), pack([br(40)])], {"max_depth": 9},
     "unsupported: branch time of a trimmed node with CUR_T > 0"),
    # the same with a node of the first round (CUR_T 0): its branch time is found again
    ([pack([br(4) + br(4, 1)]), pack([[], br(10)]), pack([br(20)])], {"max_depth": 9}, "unsupported: a node of round 0 is expanded again in round 3"),
    ([pack([br(4)]), pack([br(10)]), pack([ONE])], {"max_rounds": 2}, "unsupported: more than 2 AIME rounds"),
    ([pack([[]])], {}, "unsupported: no end node found in the scenario tree"),
    ([pack([br(4)]), pack([br(10)])], {"max_depth": 2}, "unsupported: no end node found in the scenario tree"),
])
def test_unsupported_exits(rounds, kw, message):
    d = aime_book(50, kw.pop("max_depth", 3), A, rounds, **kw)
    assert d["code"] != 0 and d["error"] == message and "nodes" not in d


def test_rejected_arguments():
    assert aime_book(50, 3, A, [np.zeros(23, np.float32)]) is None             # a round of the wrong length
    assert aime_book(61, 3, A, [pack([ONE])]) is None and aime_book(50, 3, A, [pack([ONE])], world=2, rank=2) is None


# ---- agreement with the Python host rules -------------------------------------------------------------------------------------------------
class Unsupported(Exception):
    pass


class Witness:
    """the round-by-round host path (ScenarioTreeGenerator._branch_aime_host) over decision words instead of a network: the tree container and
    decide_branch / get_branch_set / _scenario_trees_from_tree are the planner's own; the branch-time search scans the same bits and the
    observation update keeps the times only"""
    decide_branch = ScenarioTreeGenerator.decide_branch
    get_branch_set = ScenarioTreeGenerator.get_branch_set
    get_end_set = ScenarioTreeGenerator.get_end_set
    create_nodes = ScenarioTreeGenerator.create_nodes
    _scenario_trees_from_tree = ScenarioTreeGenerator._scenario_trees_from_tree

    def __init__(self, pred_len, max_depth):
        self.pred_len, self.obs_len, self.shard, self.branch_depth, self.round = pred_len, 0, None, 0, 0
        self.config = SimpleNamespace(max_depth=max_depth)
        self.tree = Tree()
        root = {"SCEN_ID": "root", "SCEN_PROB": np.float32(1), "CUR_T": 0, "END_T": pred_len}
        self.tree.add_node(Node("root", None, ScenarioData(None, root, branch_flag=True)))

    def get_branch_times(self, datas):
        out = []
        for d in datas:
            if d.get("REBASED") and d["CUR_T"] > 0:
                raise Unsupported("trimmed")
            for t in range(d["CUR_T"] + 1 + (d["CUR_T"] + 1) % 2, d["END_T"], 2):
                if d["HIT"] >> t & 1:
                    d["END_T"] = t
                    break
            out.append(d["END_T"])
        return out

    def update_obser_batch(self, curs, own=None):
        out = []
        for c in curs:
            if c["ROUND"] != self.round:
                raise Unsupported("again")
            c["REBASED"] = True
            out.append(({"SCEN_ID": c["SCEN_ID"], "SCEN_PROB": c["SCEN_PROB"], "CUR_T": c["END_T"], "END_T": self.pred_len}, c))
        return out

    def expand(self, batch, scenes):
        """create_nodes' input for one round: the kept modes of every scene of the branch set"""
        z = np.zeros((1, self.pred_len, 2), np.float32)
        return [{"SCEN_ID": f"{self.round}_{b}_{k}", "PARENT_ID": obs["SCEN_ID"], "SCEN_PROB": np.float32(p), "CUR_T": obs["CUR_T"], "END_T": obs["END_T"],
                 "HIT": h, "ROUND": self.round, "TRAJS_POS_HIST": z, "TRAJS_COV_HIST": z[:, :, :1], "TGT_PTS": None}
                for b, (obs, kept) in enumerate(zip(batch, scenes)) for k, p, h in kept]


def random_stream(seed):
    """-> (pred_len, max_depth, max_rounds, [scenes of round 0, ...], witness or the name of the exit it takes)"""
    rng = np.random.default_rng(seed)
    pred_len, max_depth, max_rounds = int(rng.choice([50, 60, 37])), int(rng.choice([1] + [2, 3, 4] * 8)), int(rng.choice([32] * 12 + [3]))
    w, rounds = Witness(pred_len, max_depth), []
    try:
        batch = [n.data.obs_data for n in w.get_branch_set()]
        while batch:
            if w.round >= max_rounds:
                rounds.append([[] for _ in batch])        # (the replay stops where its rounds end: hand it the round the plan would refuse)
                raise Unsupported("rounds")
            scenes = []
            for _ in batch:
                modes = rng.permutation(6)[:rng.integers(1, 4)]
                scenes.append([(int(k), np.float32(rng.uniform(.01, 1)),
                                0 if rng.random() < .45 else int(np.bitwise_or.reduce(np.uint64(1) << rng.integers(0, 64, rng.integers(1, 4), np.uint64)))) for k in modes])
            rounds.append(scenes)
            w.create_nodes(w.expand(batch, scenes))
            w.decide_branch()
            w.round += 1
            batch = [n.data.obs_data for n in w.get_branch_set()]
        if not w.get_end_set():
            raise Unsupported("no end")
    except Unsupported as e:
        return pred_len, max_depth, max_rounds, rounds, str(e)
    return pred_len, max_depth, max_rounds, rounds, w


EXITS = {"rounds": "unsupported: more than", "trimmed": "unsupported: branch time of a trimmed node", "again": "unsupported: a node of round",
         "no end": "unsupported: no end node"}
N_STREAMS = 200


def test_random_streams_agree_with_the_python_host_rules():
    unsupported = 0
    for seed in range(N_STREAMS):
        pred_len, max_depth, max_rounds, rounds, w = random_stream(seed)
        d = aime_book(pred_len, max_depth, A, [pack(s) for s in rounds], max_rounds=max_rounds)
        if isinstance(w, str):
            unsupported += 1
            assert d["error"] is not None and d["error"].startswith(EXITS[w]), (seed, w, d["error"])
            continue
        assert d["error"] is None, (seed, d["error"])
        trees = w._scenario_trees_from_tree()
        keys = [k for k in w.tree.nodes if k != "root"]
        assert [f"{n['round']}_{n['scene']}_{n['mode']}" for n in d["nodes"]] == keys, seed
        for n, k in zip(d["nodes"], keys):
            t = w.tree.nodes[k]
            s = t.data
            par = -1 if t.parent_key == "root" else keys.index(t.parent_key)
            flags = (BRANCH if s.branch_flag else 0) | (END if s.end_flag else 0) | (TERM if s.terminate_flag else 0)
            assert (n["parent"], n["cur_t"], n["end_t"], n["flags"], n["prob"]) == (par, s.data["CUR_T"], s.data["END_T"], flags, f32bits(s.data["SCEN_PROB"])), (seed, k)
            assert n["dur"] == (s.data["END_T"] - s.data["CUR_T"] if s.end_flag else 0)
        rs = w.tree.get_root().data
        assert d["root_flags"] == (BRANCH if rs.branch_flag else 0) | (END if rs.end_flag else 0) | (TERM if rs.terminate_flag else 0)
        flats = [flatten_scenario_tree(t) for t in trees]
        assert [keys[i] for i in d["tree_top"]] == [t.get_root_key() for t in trees], seed
        assert d["tree_off"] == [0] + list(np.cumsum([len(f["parent"]) for f in flats])), seed
        assert d["flat_parent"] == [int(v) for f in flats for v in f["parent"]], seed
        assert d["flat_prob"] == [int(v) for f in flats for v in f["prob"].view(np.uint32)], seed
    # the generator was written so that the witness alone leaves fewer than one stream in ten to the host path
    assert unsupported < N_STREAMS // 10, unsupported


# ---- sharding ---------------------------------------------------------------------------------------------------------------------------
WORLDS = (1, 2, 3, 5)


def test_blocks_and_owners_are_shard_blocks():
    for world in WORLDS:
        for S in range(14):
            # three scenes whose kept modes all branch: S scenes in the next round
            scenes = [[(k, .1, 1 << 10) for k in range(6)], [(k, .1, 1 << 10) for k in range(6)], [(0, .1, 1 << 10)]]
            kept = [[m for m in sc if (S > 0 and (b * 6 + m[0]) < S)] for b, sc in enumerate(scenes)]
            for rank in range(world):
                d = aime_book(50, 3, A, [pack([br(4) + br(4, 1) + br(4, 2)], world, True), pack(kept, world, True)], world=world, rank=rank, force=True)
                r0, r1 = d["rounds"]
                assert (r0["lo"], r0["hi"]) == block(1, rank, world) and (r1["B"], r1["lo"], r1["hi"]) == (3, *block(3, rank, world))
                assert r1["S"] == S and sum(r1["cnt_r"]) == S
                lo, hi = block(S, rank, world)
                got = sorted(s for j in range(world) for s in range(r1["rcv"][2 * j], r1["rcv"][2 * j + 1]))
                assert got == list(range(lo, hi)), (world, rank, S)                   # pl_block: what this rank consumes
                # pl_owner: the children of a rank's scenes are one contiguous range of the branch set
                assert r1["cnt_r"] == [sum(len(kept[b]) for b in range(*block(3, r, world))) for r in range(world)]
                assert r1["s0_r"] == [0] + list(np.cumsum(r1["cnt_r"])) and (r1["s0"], r1["Sm"]) == (r1["s0_r"][rank], r1["cnt_r"][rank])


def routes(world, force, rounds_of, per_scene=7):
    return [aime_book(50, 4, A, rounds_of(world), world=world, rank=r, force=force, per_scene=per_scene) for r in range(world)]


def full_rounds(world, dist=True):
    six = lambda t: [(k, .1, 1 << t) for k in range(6)]
    return [pack([six(4)], world, dist), pack([six(10)] * 6, world, dist), pack([six(20)[:3]] * 36, world, dist)]


def test_routes_are_mutually_consistent():
    for world in WORLDS:
        for force in (False, True):
            if world == 1 and not force:
                continue
            ds = routes(world, force, full_rounds)
            for ri in range(3):
                rs = [d["rounds"][ri] for d in ds]
                S = rs[0]["S"]
                assert S == (6, 36, 108)[ri] and len({r["any"] for r in rs}) == 1
                seen = []
                for j in range(world):
                    for k in range(world):
                        # what j sends to k is what k receives from j, scenes and bytes
                        assert rs[j]["snd"][2 * k:2 * k + 2] == rs[k]["rcv"][2 * j:2 * j + 2]
                        n = rs[j]["snd"][2 * k + 1] - rs[j]["snd"][2 * k]
                        assert rs[j]["tab"][k] == rs[k]["tab"][world + j] == n * 7 * 4 and n >= 0
                        if j == k and not force:
                            assert n == 0              # a rank's own scenes stay where they are ...
                            lo, hi = max(rs[j]["s0"], block(S, j, world)[0]), min(rs[j]["s0"] + rs[j]["Sm"], block(S, j, world)[1])
                            seen += list(range(lo, hi))
                        else:
                            seen += list(range(rs[j]["snd"][2 * k], rs[j]["snd"][2 * k + 1]))
                assert sorted(seen) == list(range(S))       # ... and with them the ranges tile [0, S) exactly once
                assert rs[0]["any"] == sum(r["tab"][k] for r in rs for k in range(world)) // 28


def test_a_forced_one_rank_group_sends_its_scenes_to_itself():
    (d,) = routes(1, True, full_rounds)
    for r, S in zip(d["rounds"], (6, 36, 108)):
        assert r["snd"] == r["rcv"] == [0, S] and r["tab"] == [S * 28, S * 28] and r["any"] == S


def test_a_round_whose_ranges_coincide_moves_nothing():
    # two ranks, two scenes with three children each: rank r re-bases [3r, 3r + 3) = its block of the six
    three = [(k, .1, 1 << 10) for k in range(3)]
    for d in routes(2, False, lambda w: [pack([br(4) + br(4, 1)], w, True), pack([three, three], w, True)]):
        r = d["rounds"][1]
        assert r["S"] == 6 and r["cnt_r"] == [3, 3] and r["any"] == 0 and r["tab"] == [0] * 4
    # ... four and two children: rank 0's fourth scene travels to rank 1
    four = three + [(3, .1, 1 << 10)]
    d0, d1 = routes(2, False, lambda w: [pack([br(4) + br(4, 1)], w, True), pack([four, three[:2]], w, True)])
    assert d0["rounds"][1]["any"] == 1 and d0["rounds"][1]["snd"] == [0, 0, 3, 4] and d1["rounds"][1]["rcv"] == [3, 4, 0, 0]


def test_the_job_tables_of_all_ranks_cover_every_row_and_flat_entry_once():
    """the invariant the zero-filled all-reduce relies on"""
    def rounds_of(world):
        six = lambda t: [(k, .1, (1 << t) if k % 2 else 0) for k in range(6)]
        return [pack([six(4)], world, True), pack([six(10)[:5]] * 3, world, True), pack([six(20)[:4]] * 6, world, True)]
    (one,) = [aime_book(50, 4, A, rounds_of(1)[:0] + [np.asarray(r)[:1] for r in rounds_of(1)])]
    for world in WORLDS:
        ds = routes(world, True, rounds_of)
        rows, flat = np.zeros(one["n_rows"], int), np.zeros(one["tree_off"][-1], int)
        for d in ds:
            assert [node(d, i) for i in range(len(d["nodes"]))] == [node(one, i) for i in range(len(one["nodes"]))]      # the tree is replicated
            assert (d["tree_off"], d["flat_parent"], d["flat_prob"]) == (one["tree_off"], one["flat_parent"], one["flat_prob"])
            for row0, dur, dst, a, _ in d["gather"]["jobs"]:
                rows[dst:dst + a * dur * 3] += 1
            for row0, n, dst, a, _ in d["flat"]["jobs"]:
                flat[dst:dst + n] += 1
            for t in (d["gather"], d["flat"]):
                assert t["job_of_block"] == [j for j in range(len(t["jobs"])) for _ in range(A)] and t["agent_of_block"] == list(range(A)) * len(t["jobs"])
        assert (rows == 1).all() and (flat == 1).all() and len(rows) > 0 and len(flat) > 0
        # a job's first row lies in the world buffer of the rank that predicted the node: its scene there, not the global one
        d = ds[-1]
        mine = [n for n in d["nodes"] if n["owner"] == world - 1 and n["flags"] & END and n["dur"] > 0]
        assert [j[0] for j in d["gather"]["jobs"]] == [n["lscene"] * A * 6 + n["mode"] for n in mine]
        assert [j[4] for j in d["gather"]["jobs"]] == [n["round"] for n in mine]


# ---- chunking -----------------------------------------------------------------------------------------------------------------------------
def chunk_of(Bk, n_tokens, mb, bytes_per_pair=512):
    kw = dict(n_tokens=n_tokens, plan_chunk_mb=mb, bytes_per_pair=bytes_per_pair)
    if Bk == 0:   # the second rank of two in a round of one scene
        r = aime_book(50, 3, A, [pack([ONE], 2, True)], world=2, rank=1, **kw)["rounds"][0]
    elif Bk == 1:
        r = aime_book(50, 3, A, [pack([ONE])], **kw)["rounds"][0]
    else:       # the third round of a full tree: 36 scenes
        six = lambda t: [(k, .1, 1 << t) for k in range(6)]
        r = aime_book(50, 3, A, [pack([six(4)]), pack([six(10)] * 6), pack([ONE] * 36)], **kw)["rounds"][2]
    assert r["hi"] - r["lo"] == Bk
    return r["chunk"]


@pytest.mark.parametrize("Bk", [0, 1, 36])
def test_chunk_sizes(Bk):
    # 64 tokens, 512 B per pair: one scene's edge tensor is exactly 2 MB
    assert chunk_of(Bk, 64, 1) == 1                               # a budget below one scene: still one scene per call
    assert chunk_of(Bk, 64, 2) == 1                               # exactly one scene
    assert chunk_of(Bk, 64, 5) == min(2, max(Bk, 1))
    assert chunk_of(Bk, 64, 71) == min(35, max(Bk, 1)) and chunk_of(Bk, 64, 72) == max(Bk, 1)
    assert chunk_of(Bk, 64, 96 * 1024) == max(Bk, 1)              # above the round
    assert chunk_of(Bk, 64, 4, 256) == min(4, max(Bk, 1))         # bf16 edges: half the bytes
    # tokens are padded to 16 on one side: 20 x 32 x 512 B = 320 kB per scene
    assert chunk_of(Bk, 20, 1) == min(3, max(Bk, 1))
    for n_tokens in (1, 17, 20, 64, 300):
        for mb in (1, 3, 1000):
            assert 1 <= chunk_of(Bk, n_tokens, mb) <= max(Bk, 1)
