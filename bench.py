#!/usr/bin/env python
"""bench.py --gpus N --steps K --warmup W [--workload demo_1|demo1|cfg4tree|...] [--shard | --replicas] [--full] [--dump-outputs DIR]

A step = one planning cycle of the headless closed loop (mind_amd.closed_loop, mirroring simulator.py:58-103 /
agent.py:277-331): 5 simulator steps of 0.02 s (observation fan-out, 10 Hz planner trigger, ego plant) containing one
MINDPlanner.plan() = AIME scenario tree (every tree node through the HIP predictor) + tree-iLQR contingency solves
(warm start + full) for every scenario tree + selection.  value = simulator steps / wall time, whole job.

Default workload = BASELINE.json configs[1]: the closed loop on the reference's recorded scene demo_1 (compact fixture
tests/golden/scenes/demo_1.npz).  The trained checkpoint is not in the reference tree; the recorded scenes run with the
BRANCHING formula weights (mind_amd/weights.py, variant "branching": the reference itself then expands 6 scenes in two AIME
rounds and solves 5 scenario trees per plan on demo_1 -- the load a trained checkpoint produces); with --full the plain formula
weights (one expansion, one or two trees per plan) are reported beside it as `plain_formula_weights`.

A plain run sets up, warms up (W cycles), times the K cycles and prints the line.  --full adds everything else the line can carry:
the extra workloads, sizes and precisions, the rocprofv3 traffic passes of the roofline and the CPU baseline.  --dump-outputs DIR
writes what the last timed cycle computed (dump_outputs) for an output-for-output comparison of two builds.

Multi-GPU (one process per GPU; plain `python bench.py --gpus N` spawns the N ranks itself through
torch.distributed.run, under a launcher it reads RANK / LOCAL_RANK / WORLD_SIZE):
  * default workload: every rank runs its own closed loop (independent scenes: weak scaling, no data-path collective),
    and with --full the line also carries `tree_replicas` (every rank plans the full cfg4 tree of a scene of its own: weak scaling of the node
    throughput) and `tree_sharded`: the full cfg4 scenario tree planned ONCE by all ranks together (AIME rounds
    block-sharded, contingency solves round-robin, RCCL all-gather / broadcast per round: strong scaling);
  * --workload cfg4tree / stress128tree (or --shard): that sharded plan is the headline (`scaling: strong`);
    --replicas forces independent replicas.
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
if "--pipelined" in sys.argv or "--per-process" in sys.argv:
    # one thread drives P contexts of three streams each: more than the ROCm runtime's default four hardware queues per process, and
    # streams that share a queue run in order (measured: 3 134 -> 3 959 sim steps/s at P = 4 with eight queues).  Read at runtime start.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import numpy as np
import torch

METRIC = "sim steps/sec (whole node) + scenario-tree nodes expanded/sec, AV2 demo scenes"
WORKLOADS = {
    # BASELINE configs[1]: the reference's recorded AV2 demo scenes (compact fixtures derived from data/<seq_id>/)
    "demo_1": dict(scene="demo_1"), "demo_2": dict(scene="demo_2"), "demo_3": dict(scene="demo_3"), "demo_4": dict(scene="demo_4"),
    # BASELINE config 3: demo_{1,2,3,4} concurrently on one GPU (use with --concurrent P: scene i plans demo_(i mod 4 + 1))
    "demo_all": dict(scene="demo_1"),
    # demo_1-like synthetic scene: ~40 tracked agents, ~55 lane polylines (N ~ 96) with scripted mode branching on top of
    # the real predictor forward (4 expansions + 3-4 scenario trees per plan: the load a trained checkpoint would produce)
    "demo1": dict(n_agents=40, n_lanes=5, n_segs=11, seed=3),
    # cfg4: 64 agents x 256 lane polylines
    "cfg4": dict(n_agents=64, n_lanes=8, n_segs=32, seed=4),
    # cfg4 with the full scripted 6-ary depth-4 AIME tree (259 expansions / plan; BASELINE config 4)
    "cfg4tree": dict(n_agents=64, n_lanes=8, n_segs=32, seed=4),
    # the agent count of BASELINE config 5 (128 agents x 256 lane polylines, N = 385) on the largest tree the
    # reference's probability floor lets grow (6-ary, 259 expansions)
    "stress128tree": dict(n_agents=128, n_lanes=8, n_segs=32, seed=5),
    # the same scene under the scripted 6-ary depth-5 tree with the probability floor lifted (mind_amd.synth.ScriptedDeepTree): rounds of
    # 1 / 6 / 36 / 216 / 1 296 scenes = 1 555 expansions per plan -- what K = 6 modes and max_depth = 5 leave of BASELINE configs[4]'s tree
    "stressdeep": dict(n_agents=128, n_lanes=8, n_segs=32, seed=5),
    # ... and one level deeper (ScriptedDeeperTree): six rounds, 1 / 6 / 36 / 216 / 1 296 / 7 776 scenes = 9 331 expansions per plan, BASELINE
    # configs[4]'s depth at the branching K = 6 allows; the last round only runs in chunks (its edge tensor alone is 307 GB in plain bf16)
    "stressdeeper": dict(n_agents=128, n_lanes=8, n_segs=32, seed=5),
}
FULL_TREE = ("cfg4tree", "stress128tree", "stressdeep", "stressdeeper")
DEEP = {"stressdeep": "deep", "stressdeeper": "deeper"}
BRANCHING_WEIGHTS, PLAIN_WEIGHTS = "formula_branching:20240121", "formula:20240121"

# ---- algorithmic work of the pair kernel ----------------------------------------------------------
F_MIN_N2 = 754944.0        # minimal-algorithm FLOPs per expansion, N^2 coefficient (K and V projections kept)
PAIR_FULL = 69632.0        # folded algorithm, per pair and layer: 2 x (2*128*128) GEMMs + 2*8*128 scores + 2*8*128 sum p.mem
PAIR_ATT = 36864.0         # a pair whose edge is not updated: first GEMM + attention
PAIR_UPD = 32768.0         # the edge-update GEMM alone
PEAK_F32_MFMA, PEAK_BF16_MFMA, PEAK_HBM = 157.3e12, 2500e12, 8.0e12      # MI355X_MICROARCH.md
# The arithmetic of the CREDITED slots of the line (value, ms_per_step, dtype, roofline): an fp32-class one -- the reference computes the
# predictor in fp32, and a narrower arithmetic than the reference's own is not a measurement of this metric.  "f32" = plain fp32
# operands on v_mfma_f32_16x16x4_f32; "bf16x6" = operands split three ways into bf16 hi + mid + lo (3 x 8 = 24 significand bits, exact), the
# six partial products >= 2^-24 on v_mfma_f32_16x16x32_bf16, fp32 accumulate.  bf16x3 (two-way split, 16 bits) is reported beside it.
HEADLINE_PREC = os.environ.get("MIND_BENCH_PREC", "bf16x6")
PREC_DTYPE = {"f32": "f32 (fp32 operands on the fp32 MFMA)",
              "bf16x6": "f32-class (bf16 hi+mid+lo split operands = 24 significand bits, six products, fp32 accumulate)",
              "bf16x3": "bf16x3 (bf16 hi+lo split operands, fp32 accumulate)", "bf16": "bf16"}
PREC_PASSES = {"f32": 1, "bf16x6": 6, "bf16x3": 3, "bf16": 1}
PREC_KERNEL = {"f32": "k_pair (fp32 MFMA)", "bf16x6": "k_pair_t6", "bf16x3": "k_pair_t<*,3>", "bf16": "k_pair_t<*,1>"}
PREC_NOTE = {"f32": "v_mfma_f32_16x16x4_f32 (fp32 MFMA = the fp32 vector rate)",
             "bf16x6": "operands split into bf16 hi + mid + lo (exact: 24 significand bits), the 6 products >= 2^-24 per term on "
                       "v_mfma_f32_16x16x32_bf16, fp32 accumulate: peak = dense bf16 peak / 6 passes",
             "bf16x3": "operands split into bf16 hi + lo, 3 products per term on v_mfma_f32_16x16x32_bf16, fp32 accumulate: "
                       "peak = dense bf16 peak / 3 passes",
             "bf16": "plain bf16 operands, fp32 accumulate"}


def fold_flops(N, nf):
    """FLOPs of the folded algorithm for one scene, all six launches: layers 0-3 update every edge, layer 4 only the
    a + 1 flagged columns, layer 5 runs only those columns (network.py:249: the last layer has no edge update)."""
    return 4 * N * N * PAIR_FULL + N * N * PAIR_ATT + N * nf * PAIR_UPD + N * nf * PAIR_ATT


def edge_bytes(N, nf):
    """Algorithmic HBM bytes of the six launches (fp32 edge, 512 B per pair): layer 0 writes, layers 1-3 read + write,
    layer 4 reads all and writes the flagged columns, layer 5 reads the flagged columns."""
    return 512.0 * (N * N + 3 * 2 * N * N + N * N + N * nf + N * nf)


def scene_workload(workload, i):
    """workload of the i-th concurrent scene / replica: its own seed for the synthetic worlds, round-robin over the four
    recorded scenes for demo_all."""
    if workload == "demo_all":
        return dict(scene="demo_%d" % (i % 4 + 1))
    wkw = dict(WORKLOADS[workload])
    if "seed" in wkw:
        wkw["seed"] = wkw["seed"] + i
    return wkw


def _concurrent_label(workload, P):
    if workload == "demo_all":
        return f"the recorded scenes demo_1..4 ({P} closed loops, scene i = demo_(i mod 4 + 1))", "recorded AV2 scenes, formula-initialised weights"
    if "scene" in WORKLOADS[workload]:
        return f"{P} closed loops on the recorded scene {workload}", "recorded AV2 scene, formula-initialised weights"
    return f"{P} {workload}-like synthetic scenes", "synthetic"


def make_planner(wkw, scripted=True):
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.synth import ScriptedBranching, SynthWorld
    cfg = os.path.join(ROOT, "mind_amd", "planners", "mind", "configs", "synthetic.json")
    w = SynthWorld(**wkw)
    pl = MINDPlanner(cfg)
    if scripted:
        pl.scen_tree_gen.network = ScriptedBranching(pl.network)
    for s in range(50):
        pl.update_observation(w.local_semantic_map(round(0.1 * s, 6)))
    lcl = w.local_semantic_map(4.9)
    pl.update_target_lane(np.asarray(w.target_lane[::2], dtype=np.float64))
    pl.update_state_ctrl(lcl.ego_agent.state, np.array([0.0, 0.0]))
    return pl, lcl, w


def make_closed_loop(wkw, scripted=True, full_tree=False, speculative=True, ckpt=None, own_context=False, native=False):
    """planner + closed-loop simulator advanced to the enable time (t = 4.0 s: 40 observation updates).
    ckpt: override of the planner config's ckpt_path (e.g. "formula_branching:20240121", mind_amd/weights.py).
    native: ClosedLoopSim's argument -- False = the Python steps (tests that hook into the planner's pieces), None = the native loop
    (one C call per planning cycle, mind_amd/native_loop.py) where it applies: the throughput runs below."""
    from mind_amd.closed_loop import ClosedLoopSim
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.synth import ScriptedBranching, ScriptedDeepTree, ScriptedDeeperTree, ScriptedFullTree, SynthWorld
    cfg = os.path.join(ROOT, "mind_amd", "planners", "mind", "configs", "synthetic.json")
    if "scene" in wkw:
        from mind_amd.scene_io import ReplayWorld, scene_fixture_path
        w = ReplayWorld.from_scene_file(scene_fixture_path(wkw["scene"]))
        cfg = dict(json.load(open(cfg)), planning_config="planners.mind.configs.planning." + wkw["scene"])
    else:
        w = SynthWorld(**wkw)
    if ckpt is not None:
        cfg = dict(cfg if isinstance(cfg, dict) else json.load(open(cfg)), ckpt_path=ckpt)
    if own_context:       # a HIP context + stream of its own for this planner (several planners driven from one thread: mind_amd/pipelined.py)
        cfg = dict(cfg if isinstance(cfg, dict) else json.load(open(cfg)), own_context=True)
    pl = MINDPlanner(cfg)
    # recorded scenes run the predictor's own modes, as the reference does with the same weights (its AIME tree then
    # collapses to a few nodes); the scripted modes are straight-line motions in the agent frame and would leave a
    # curved recorded target lane, so they are kept for the synthetic worlds only
    if scripted and "scene" not in wkw:
        pl.scen_tree_gen.network = (ScriptedDeeperTree if full_tree == "deeper" else ScriptedDeepTree if full_tree == "deep" else ScriptedFullTree if full_tree
                                    else ScriptedBranching)(pl.network)
        if full_tree in ("deep", "deeper"):
            # five rounds of expansions: the nodes of the fifth (depth 5) must still be examined to END their branches -- ScenTreeCfg.max_depth
            # (configs/planning/demo_1.py:5: 5) is a planning-config value; with it every branch would stop at the cap unfinished
            import copy
            pl.scen_tree_gen.config = copy.copy(pl.scen_tree_gen.config)
            pl.scen_tree_gen.config.max_depth = 7 if full_tree == "deeper" else 6
    # speculative warm start = a second HIP context per planner: a latency lever for a GPU that one closed loop leaves idle;
    # with many scenes sharing the device the extra contexts cost more than they hide (measured: 8 processes 3150 -> 2010)
    pl.traj_tree_opt.speculative = speculative and pl.traj_tree_opt.speculative      # MIND_SPECULATIVE_WARM_START=0 switches it off
    # episodes: the reference's 60 cycles for a recording; 24 for the synthetic worlds (all eight seeds the weak-scaling
    # and concurrent modes use stay on their lane that long; the default 3 + 20 cycles fit in one episode)
    sim = ClosedLoopSim(w, pl, episode_plans=60 if "scene" in wkw else 24, native=native)
    sim.run_until(sim.enable_time)
    return pl, sim, w


class Dist:
    """torch.distributed for the bench: barrier + max-over-ranks timing, sums; a no-op for one process."""

    def __init__(self, backend, local):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.backend = backend
        self.d = None
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if backend == "nccl":       # RCCL over xGMI: one rank per GPU
                dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            else:                       # gloo: the same code path on a box with fewer GPUs than ranks (tests)
                dist.init_process_group(backend)
            self.d = dist
        self.dev = "cuda" if backend == "nccl" else "cpu"

    def barrier(self):
        torch.cuda.synchronize()
        if self.d is not None:
            self.d.barrier()
        torch.cuda.synchronize()

    def reduce(self, v, op="sum"):
        if self.d is None:
            return float(v)
        t = torch.tensor([float(v)], device=self.dev, dtype=torch.float64)
        self.d.all_reduce(t, op=self.d.ReduceOp.MAX if op == "max" else self.d.ReduceOp.SUM)
        return float(t.item())

    def close(self):
        if self.d is not None:
            self.d.barrier()
            self.d.destroy_process_group()


def measure(dist, workload, steps, warmup, shard, replica=0, ckpt=None, pair_prec=None, tuning=None):
    """K timed planning cycles of one closed loop (barrier + synchronize on both sides, max over ranks), with the pair
    kernel's launch durations taken from HIP events on the context stream inside the timed region."""
    wkw = scene_workload(workload, replica)
    if ckpt is None and "scene" in wkw:
        ckpt = BRANCHING_WEIGHTS
    pl, sim, w = make_closed_loop(wkw, full_tree=DEEP.get(workload, workload in FULL_TREE), ckpt=ckpt,
                                  native=NATIVE_LOOP if not (shard and dist.world > 1) else False)
    sh = None
    if shard and dist.world > 1:
        sh = pl.enable_sharding()
    rt = pl.network.rt
    prec_before = rt.pair_precision()
    if pair_prec is not None:
        rt.set_pair_precision(pair_prec)        # every MFMA contraction of the predictor (pair kernel, ActorNet) follows this setting
    for k, v in (tuning or {}).items():
        rt.set_tuning(k, v[0])
    if workload in FULL_TREE:
        # thousands of agents per decoder call: the MFMA variant of its actor part pays here (209 vs 277 us at 13.8 k agents);
        # every rank of a sharded run takes the same kernel
        rt.set_tuning("dec_mfma_min", 0)
    sim.run_plans(max(warmup, 1))
    rt.set_profiling(True)
    acc = dict(ms=0.0, launches=0, n2=0.0, fold=0.0, bytes=0.0, calls=0)
    orig_predict = rt.predict

    def prof_predict(*a, **k):
        o = orig_predict(*a, **k)
        n, ms, _ = rt.fusion_stats()
        a_off, l_off = a[1], a[3]
        for i in range(len(a_off) - 1):
            na = a_off[i + 1] - a_off[i]
            N = na + (l_off[i + 1] - l_off[i]) + 1
            acc["n2"] += N * N
            acc["fold"] += fold_flops(N, na + 1)
            acc["bytes"] += edge_bytes(N, na + 1)
        acc["ms"] += ms
        acc["launches"] += n
        acc["calls"] += 1
        return o

    rt.predict = prof_predict
    # recorded scenes run the whole AIME loop inside ONE native call (mind_aime_plan): its pair-kernel launches are timed by the same
    # HIP events, summed over the plan's rounds
    orig_plan = rt.aime_plan

    def prof_plan(*a, **k):
        r = orig_plan(*a, **k)
        if r is not None:
            info = r[2]
            na, N = info["a"], info["a"] + info["l"] + 1
            for B in info["round_scenes"]:
                acc["n2"] += B * N * N
                acc["fold"] += B * fold_flops(N, na + 1)
                acc["bytes"] += B * edge_bytes(N, na + 1)
            acc["ms"] += info["pair_ms"]
            acc["launches"] += info["pair_launches"]
            acc["calls"] += len(info["round_scenes"])
        return r

    rt.aime_plan = prof_plan
    # the tree-iLQR launch of every plan, timed by HIP events on the context stream (mind_last_ilqr_stats)
    il = {"ms": 0.0, "launches": 0, "trees": 0, "wgs": 1, "prof": {}}
    orig_solve = pl.traj_tree_opt.solve_batch

    def prof_solve(*a, **k):
        r = orig_solve(*a, **k)
        ms, nt, g = rt.ilqr_stats()
        if ms > 0:
            il["ms"] += ms; il["launches"] += 1; il["trees"] += nt; il["wgs"] = g
            for kk, v in rt.ilqr_profile().items():        # phase cycles of the launch's critical cost tree
                il["prof"][kk] = il["prof"].get(kk, 0.0) + v
            il["prof"]["node_steps"] = il["prof"].get("node_steps", 0.0) + rt.ilqr_profile()["passes"] * rt.ilqr_profile()["depth"]
        return r

    pl.traj_tree_opt.solve_batch = prof_solve
    ctr0 = dict(pl.traj_tree_opt.counters)
    tsum0 = dict(pl.timing_sum)
    coll0 = (sh.n_collectives, sh.bytes_gathered) if sh is not None else (0, 0)
    # the native loop (mind_amd/native_loop.py: the whole cycle behind one C call) never comes back to the hooks above: the library sums the
    # same HIP-event durations itself (mind_loop_totals); differences over the timed region are taken below
    nl = getattr(sim, "_native_now", lambda: None)()
    tot0 = nl.totals() if nl is not None else None
    dist.barrier()
    t0 = time.perf_counter()
    n0 = pl.scen_tree_gen.n_expanded
    sim_steps = sim.run_plans(steps)            # K planning cycles = ~5K simulator steps
    expansions = pl.scen_tree_gen.n_expanded - n0
    dist.barrier()
    dt = time.perf_counter() - t0
    rt.predict = orig_predict
    rt.aime_plan = orig_plan
    pl.traj_tree_opt.solve_batch = orig_solve
    rt.set_profiling(False)
    n_agents_now = len(pl.agent_obs)
    if nl is not None and sim._native is nl:
        t1 = nl.totals()
        df = lambda k: t1[k] - tot0[k]
        acc["ms"] += df("pair_ms"); acc["launches"] += df("pair_launches"); acc["calls"] += df("rounds"); acc["n2"] += df("scene_n2")
        acc["fold"] += (4 * PAIR_FULL + PAIR_ATT) * df("scene_n2") + (PAIR_UPD + PAIR_ATT) * df("scene_n_a1")        # = sum of fold_flops(N, a + 1) over the expanded scenes
        acc["bytes"] += 512.0 * (8 * df("scene_n2") + 2 * df("scene_n_a1"))                                            # = sum of edge_bytes(N, a + 1)
        il["ms"] += df("ilqr_ms"); il["launches"] += df("ilqr_launches"); il["trees"] += df("ilqr_trees"); il["wgs"] = t1["ilqr_workgroups_per_tree"] or il["wgs"]
        keys = ("nodes", "depth", "passes", "derivatives", "backward", "state_chain", "cost_pass", "selection", "trees")
        for kk, v1, v0 in zip(keys, t1["ilqr_prof"], tot0["ilqr_prof"]):
            il["prof"][kk] = il["prof"].get(kk, 0.0) + (v1 - v0)
        il["prof"]["node_steps"] = il["prof"].get("node_steps", 0.0) + df("ilqr_node_steps")
        n_agents_now = nl.out.n_agents
    if pair_prec is not None:
        rt.set_pair_precision(prec_before)
    for k, v in (tuning or {}).items():
        rt.set_tuning(k, v[1])
    dt = dist.reduce(dt, "max")
    ctr = {k: v - ctr0.get(k, 0) for k, v in pl.traj_tree_opt.counters.items()}
    npl = max(pl.timing_sum["plans"] - tsum0["plans"], 1)
    brk = {"aime": (pl.timing_sum["aime_s"] - tsum0["aime_s"]) / npl * 1e3, "ilqr": (pl.timing_sum["ilqr_s"] - tsum0["ilqr_s"]) / npl * 1e3,
           "note": "host wall time per plan, mean over the timed plans: AIME rounds (predictor + glue) | tree-iLQR (solve_batch)"}
    return dict(pl=pl, sim=sim, w=w, dt=dt, breakdown_ms=brk, ilqr_kernel=il, sim_steps=sim_steps, expansions=expansions, expansions_all=dist.reduce(expansions),
                pair=acc, ilqr=ctr, a=n_agents_now, native_loop=nl is not None and sim._native is nl, l=int(pl.scen_tree_gen.n_lanes or pl.scen_tree_gen.lane_feat_in.shape[0]), steps=steps, weights=ckpt or PLAIN_WEIGHTS,
                collectives=(sh.n_collectives - coll0[0], sh.bytes_gathered - coll0[1]) if sh is not None else None,
                real_scene="scene" in wkw, sharded=sh is not None)


def roofline(m, prec):
    """Both bounds of the pair kernel from the launch durations measured inside the timed region.  `achieved` prices the
    FOLDED algorithm the kernel executes (fold_flops above: never more than the work done, so frac <= 1); the SURVEY 8(d)
    F_min figure (K/V projections un-folded, 754 944 N^2 per expansion) is quoted beside it."""
    p = m["pair"]
    s = p["ms"] * 1e-3
    if s <= 0 or p["launches"] == 0:
        return None
    passes = PREC_PASSES[prec]
    peak = PEAK_F32_MFMA if prec == "f32" else PEAK_BF16_MFMA / passes
    f_mfma = p["fold"] / s / peak
    f_hbm = p["bytes"] / s / PEAK_HBM
    bound = "hbm" if f_hbm > f_mfma else "mfma"
    return {
        "kernel": PREC_KERNEL[prec] + " (RelaFusionLayer pair kernel, 6 launches per predictor call)", "bound": bound,
        "achieved": (p["bytes"] / s / 1e9) if bound == "hbm" else (p["fold"] / s / 1e12),
        "peak": PEAK_HBM / 1e9 if bound == "hbm" else peak / 1e12, "unit": "GB/s" if bound == "hbm" else "TFLOP/s",
        "frac": max(f_hbm, f_mfma), "traffic": None,
        "mfma": {"achieved_tflops": p["fold"] / s / 1e12, "peak_tflops": peak / 1e12, "frac": f_mfma,
                 "arith": prec, "note": PREC_NOTE[prec]},
        "hbm": {"achieved_gbs": p["bytes"] / s / 1e9, "peak_gbs": PEAK_HBM / 1e9, "frac": f_hbm},
        "f_min_tflops": F_MIN_N2 * p["n2"] / s / 1e12,
        "launches_profiled": p["launches"], "avg_launch_ms": p["ms"] / p["launches"],
        "algorithmic_flops_per_launch": p["fold"] / p["launches"], "algorithmic_bytes_per_launch": p["bytes"] / p["launches"],
        "note": "algorithmic FLOPs per scene = 4 N^2 69632 + N^2 36864 + N (a+1) (32768 + 36864) over the six launches (folded algorithm: "
                "rank-decomposed proj_memory, K projection folded into the query, V projection folded out of the sum); algorithmic bytes = "
                "512 B per pair read/written once per layer; launch durations from HIP events on the context stream inside the timed "
                "region; f_min_tflops prices SURVEY 8(d)'s un-folded F_min; traffic: PMC passes are separate runs (profiles/), not "
                "measured in this run"}


def measure_traffic(workload, alg_bytes_per_launch, steps=6, warmup=2, prec=None):
    """HBM traffic of the pair kernel from the hardware counters: two sibling runs of this script under `rocprofv3 --pmc
    FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes with --kernel-trace only, as MI355X_MICROARCH.md prescribes: the two do not fit
    one pass).  FETCH_SIZE / WRITE_SIZE count kilobytes; FETCH_SIZE reports half the bytes of wide coalesced reads on gfx950 and is
    doubled.  Returns (bytes per launch, details) or (None, reason)."""
    import csv
    import glob
    import shutil
    import tempfile
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None, "rocprofv3 not on PATH"
    per = {}
    for cnt in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="mind_pmc_")
        try:
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run([prof, "--pmc", cnt, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                                "--workload", workload, "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extras",
                                "--no-traffic"] + (["--prec", prec] if prec else []), cwd="/tmp", env=env, capture_output=True, text=True, timeout=420)
            if r.returncode != 0:
                return None, f"rocprofv3 --pmc {cnt} exited with {r.returncode}: {r.stderr[-200:]}"
            tot, disp = 0.0, set()
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if "k_pair" in row.get("Kernel_Name", "") and row.get("Counter_Name") == cnt:
                        tot += float(row["Counter_Value"])
                        disp.add(row.get("Dispatch_Id"))
            if not disp:
                return None, f"no {cnt} rows for the pair kernel"
            per[cnt] = (tot / len(disp), len(disp))
        except Exception as e:      # noqa: BLE001
            return None, f"{type(e).__name__}: {e}"[:300]
        finally:
            shutil.rmtree(d, ignore_errors=True)
    fetch = 2.0 * per["FETCH_SIZE"][0] * 1024.0
    write = per["WRITE_SIZE"][0] * 1024.0
    return fetch + write, {"fetch_bytes_per_launch": fetch, "write_bytes_per_launch": write, "launches_counted": per["FETCH_SIZE"][1],
                           "over_algorithmic": (fetch + write) / alg_bytes_per_launch if alg_bytes_per_launch else None,
                           "how": "two sibling runs of bench.py under rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (+ --kernel-trace only); "
                                  "counters in KB, FETCH_SIZE x 2 on gfx950 (MI355X_MICROARCH.md, HBM); mean over every k_pair launch of the runs; "
                                  "at this scene size (N = 96, 4.7 MB of edges) the traffic includes Infinity-Cache hits"}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(pl, lcl, n_scene_tokens, expansions, scen_trees, trees_per_plan=None):
    """The oracle (CPU restatement, kind 'port') on this host: one predictor forward of the same scene size at
    1 / 8 / 16 / 32 / 64 threads (best kept, 1-thread figure quoted) + the contingency solves of this plan's
    scenario trees (plain C, 1 thread), timed on a bounded sample."""
    from mind_amd.synth import predictor_batch
    from mind_amd.weights import formula_state_dict
    from oracle import ilqr as oi
    from oracle import predictor as op
    sd = formula_state_dict(as_torch=True)
    a, l = n_scene_tokens
    pb = predictor_batch(a, l, 1, seed=9)
    tb = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else [torch.from_numpy(x) for x in v]) for k, v in pb.items()}
    ncpu = os.cpu_count() or 1
    n_before = torch.get_num_threads()
    per_threads = {}
    # all hardware threads only on small hosts: torch-CPU on a tensor this size collapses under 128+ threads (measured on the
    # 256-thread GPU box: 55 s per forward at 256 threads vs 36 ms at 16)
    for nt in sorted({1, 8, 16, 32, 64, ncpu if ncpu <= 64 else 64}):
        if nt > ncpu:
            continue
        torch.set_num_threads(nt)
        op.forward(sd, tb)
        t0, reps = time.perf_counter(), 0
        while time.perf_counter() - t0 < 2.0 and reps < 10:
            op.forward(sd, tb)
            reps += 1
        per_threads[nt] = (time.perf_counter() - t0) / reps
    torch.set_num_threads(n_before)
    best_nt = min(per_threads, key=per_threads.get)
    t_pred = per_threads[best_nt]
    cfg = oi.default_cfg()
    t0 = time.perf_counter()
    n_tree = 0
    for st in scen_trees[:3]:
        nodes = [(k, n.parent_key, n.data) for k, n in st.nodes.items()]
        oi.contingency(cfg, nodes, pl.state, pl.ctrl, pl.gt_tgt_lane, lcl.target_velocity)
        n_tree += 1
    t_ilqr = (time.perf_counter() - t0) / max(n_tree, 1)
    # a plan of the timed run holds `trees_per_plan` scenario trees on average (the sampled plan is one cycle of it)
    n_solves = trees_per_plan if trees_per_plan else len(scen_trees)
    plan_s = expansions * t_pred + n_solves * t_ilqr
    plan_1 = expansions * per_threads[1] + n_solves * t_ilqr
    return {"value": 5.0 / plan_s, "unit": "sim steps/s", "cores": best_nt, "kind": "port", "cpu": cpu_model(), "hardware_threads": ncpu,
            "value_1_thread": 5.0 / plan_1,
            "predictor_ms_by_threads": {str(k): v * 1e3 for k, v in per_threads.items()},
            "sample": f"1 oracle predictor forward (a={a}, l={l}, torch-CPU fp32; best {t_pred*1e3:.0f} ms at {best_nt} threads of {sorted(per_threads)}, "
                      f"{per_threads[1]*1e3:.0f} ms at 1) + {n_tree} oracle C tree-iLQR contingency solves ({t_ilqr*1e3:.0f} ms each, 1 thread); "
                      f"plan = {expansions} expansions + {n_solves:.3g} solves (the timed run's mean)",
            "plan_ms": plan_s * 1e3}


def ilqr_block(m):
    """The tree-iLQR kernel of the workload: launch duration (HIP events on the context stream), its share of the step, how much of
    the device it uses and -- from the kernel's own cycle counters for the launch's critical cost tree -- the cycles per node of its
    two serial loops and the split over its phases."""
    k, steps = m["ilqr_kernel"], max(m["steps"], 1)
    if not k["launches"]:
        return None
    p = k["prof"]
    ns = max(p.get("node_steps", 0.0), 1.0)
    tot = sum(p.get(q, 0.0) for q in ("derivatives", "backward", "state_chain", "cost_pass", "selection")) or 1.0
    ctr = m["ilqr"]
    ms_launch = k["ms"] / k["launches"]
    # algorithmic bytes of the sweep: 2 x 115 doubles per node and iteration between forward and backward pass + 12 B per
    # agent for each of the <= 11 cost evaluations of an iteration of the full fit
    nbytes = ctr.get("node_iterations", 0) * 2 * 115 * 8 + ctr.get("node_iterations_exo", 0) * 11 * 12
    return {"kernel_ms_per_launch": ms_launch, "share_of_step": k["ms"] / (m["dt"] * 1e3),
            "cost_trees_per_launch": k["trees"] / k["launches"], "workgroups_per_tree": k["wgs"],
            "cus_busy": k["trees"] / k["launches"] * k["wgs"], "cus": 256,
            "critical_tree": {"nodes": p.get("nodes", 0) / k["launches"], "serial_depth": p.get("depth", 0) / k["launches"],
                              "passes_per_launch": p.get("passes", 0) / k["launches"]},
            "cycles_per_node_step": {"riccati": p.get("backward", 0.0) / ns, "state_chain": p.get("state_chain", 0.0) / ns},
            "phase_share": {q: p.get(q, 0.0) / tot for q in ("derivatives", "backward", "state_chain", "cost_pass", "selection")},
            "sweep_gb_per_s": nbytes / max(k["ms"] * 1e-3, 1e-12) / 1e9,
            "note": "latency-bound (serial depth x iterations of dependent float64 chains; a float64 VALU instruction issues in ~6 cycles on "
                    "gfx950), hence cycles per node step instead of a bandwidth fraction; sweep_gb_per_s prices SURVEY 8(d)'s algorithmic bytes "
                    "of the sweep against the kernel's launch time"}


def summarize(m, prec):
    """compact block for an extra workload"""
    r = roofline(m, prec)
    ctr = m["ilqr"]
    out = {"sim_steps_per_s": m["sim_steps"] / m["dt"], "ms_per_plan": m["dt"] / m["steps"] * 1e3,
           "nodes_expanded_per_s": m["expansions_all"] / m["dt"], "expansions_per_plan": m["expansions_all"] / m["steps"],
           "agents": m["a"], "lane_polylines": m["l"], "scenario_trees_per_plan": m["pl"].timing.get("n_scen_trees"),
           "ilqr_solves_per_s": ctr["solves"] / m["dt"], "ilqr_iterations_per_s": ctr["iterations"] / m["dt"],
           "k_ilqr_ms_per_launch": (m["ilqr_kernel"]["ms"] / m["ilqr_kernel"]["launches"]) if m["ilqr_kernel"]["launches"] else None,
           "k_ilqr_workgroups_per_tree": m["ilqr_kernel"]["wgs"],
           "breakdown_ms": m["breakdown_ms"], "k_ilqr": ilqr_block(m),
           # plans (warm-up included) whose whole AIME loop ran inside mind_aime_plan; 0 = the round-by-round path (sharded / wrapped networks)
           "aime_native_plans": getattr(m["pl"].scen_tree_gen, "n_native_plans", 0)}
    if r is not None:
        out["k_pair"] = {"bound": r["bound"], "frac": r["frac"], "mfma_frac": r["mfma"]["frac"], "hbm_frac": r["hbm"]["frac"],
                         "tflops": r["mfma"]["achieved_tflops"], "gbs": r["hbm"]["achieved_gbs"], "avg_launch_ms": r["avg_launch_ms"],
                         "f_min_tflops": r["f_min_tflops"]}
    if m["collectives"] is not None:
        out["collectives_per_plan"] = m["collectives"][0] / m["steps"]
        out["gathered_mb_per_plan"] = m["collectives"][1] / m["steps"] / 1e6
    return out


def recorded_scenes(prec, plans=20, warmup=3):
    """The other three recorded scenes + the whole demo_1 run (BASELINE configs[0]/[1]: 500 simulator steps, 60 cycles)."""
    dist = Dist.__new__(Dist)
    dist.rank, dist.world, dist.d, dist.dev, dist.backend = 0, 1, None, "cpu", None
    out = {}
    for name in ("demo_2", "demo_3", "demo_4"):
        m = measure(dist, name, plans, warmup, False)
        out[name] = {k: v for k, v in summarize(m, prec).items() if k in ("sim_steps_per_s", "ms_per_plan", "agents", "lane_polylines", "expansions_per_plan")}
    from mind_amd.closed_loop import ClosedLoopSim
    from mind_amd.planners.mind.planner import MINDPlanner
    pl, sim, w = make_closed_loop(dict(WORKLOADS["demo_1"]), ckpt=BRANCHING_WEIGHTS)
    sim = ClosedLoopSim(w, MINDPlanner(pl.planner_cfg))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(500):
        sim.step()
    torch.cuda.synchronize()
    out["demo_1_whole_run"] = {"simulator_steps": 500, "plans": sim.n_plans, "seconds": time.perf_counter() - t0, "weights": BRANCHING_WEIGHTS,
                               "note": "BASELINE configs[0]/[1]: the reference's whole demo_1 run (10 s, 60 planning cycles; ~10 min with rendering on its own hardware)"}
    return out


# ---- concurrent scenes on one GPU (BASELINE config 3) ---------------------------------------------------------------------
NATIVE_LOOP = None if os.environ.get("MIND_NATIVE_LOOP", "1") != "0" else False      # ClosedLoopSim(native=...) of the single-loop throughput runs
# Several scenes on one GPU (profiles/r06q_config3_native*.txt, r06aj_*): up to four scenes as a process each run the NATIVE loop with its
# speculative warm start (MIND_NATIVE_SPECULATE: warm-start fits of the previous plan's tree shapes on a second context beside the AIME rounds) --
# 9.1-9.4 k sim steps/s against 7.3-7.6 k for the Python steps with the same speculation and 5.3 k for native loops without it; sixteen scenes
# are bound by the device, not by the interpreter, and keep the Python event loops (two processes of eight: 9.0-9.5 k; native threads 7.6-8.0 k).
# MIND_CONCURRENT_NATIVE=1 / 0 forces native loops / Python steps everywhere.
CONCURRENT_NATIVE = None if os.environ.get("MIND_CONCURRENT_NATIVE", "0") == "1" else False


def _proc_scene(i, workload, steps, warmup, ready, go, q, speculative, ckpt=None):
    """One scene in its own process (own HIP context): signals ready, waits for the common start, reports back."""
    import torch as th
    native = CONCURRENT_NATIVE
    if speculative and "MIND_CONCURRENT_NATIVE" not in os.environ:      # (a handful of processes: the native loop + its speculative warm start)
        os.environ.setdefault("MIND_NATIVE_SPECULATE", "1")
        native = None
    pl, sim, w = make_closed_loop(scene_workload(workload, i), full_tree=workload in FULL_TREE, speculative=speculative, ckpt=ckpt, native=native)
    sim.run_plans(max(warmup, 1))
    th.cuda.synchronize()
    ready.wait()
    go.wait()
    t0 = time.time()
    n = sim.run_plans(steps)
    th.cuda.synchronize()
    q.put((i, n, t0, time.time(), pl.scen_tree_gen.n_expanded))


def _proc_group(g, scene_ids, workload, steps, warmup, ready, go, q, ckpt=None):
    """A group of scenes in one process: ONE host thread, the event loop of mind_amd.pipelined over the group's closed loops (a HIP context
    and stream per scene).  Signals ready, waits for the common start, reports back."""
    import torch as th
    from mind_amd.pipelined import PipelinedClosedLoops
    if CONCURRENT_NATIVE is None:
        return _proc_group_native_threads(g, scene_ids, workload, steps, warmup, ready, go, q, ckpt)
    th.cuda.set_stream(th.cuda.Stream())
    loops = [make_closed_loop(scene_workload(workload, i), scripted="scene" not in scene_workload(workload, i), speculative=False, ckpt=ckpt,
                              own_context=True) for i in scene_ids]
    pc = PipelinedClosedLoops([l[1] for l in loops])
    pc.run_plans(max(warmup, 1))
    th.cuda.synchronize()
    ready.wait()
    go.wait()
    t0 = time.time()
    n = pc.run_plans(steps)
    th.cuda.synchronize()
    q.put((g, n, t0, time.time(), sum(l[0].scen_tree_gen.n_expanded for l in loops)))


def _proc_group_native_threads(g, scene_ids, workload, steps, warmup, ready, go, q, ckpt=None):
    """A group of scenes in one process, one host thread per scene, every thread inside ONE native call for its whole run (mind_loop_advance: the
    interpreter lock is released, a HIP context + stream per thread): the host work of a cycle is a few tens of microseconds of C per scene."""
    import threading
    import torch as th
    n = len(scene_ids)
    sims, done, errs = [None] * n, [0] * n, []
    t_ready, t_go = threading.Barrier(n + 1), threading.Barrier(n + 1)

    def worker(k):
        try:
            with th.cuda.stream(th.cuda.Stream()):
                pl, sim, w = make_closed_loop(scene_workload(workload, scene_ids[k]), scripted="scene" not in scene_workload(workload, scene_ids[k]),
                                              speculative=False, ckpt=ckpt, native=CONCURRENT_NATIVE)
                sim.run_plans(max(warmup, 1))
                th.cuda.current_stream().synchronize()
                sims[k] = (pl, sim)
                t_ready.wait()
                t_go.wait()
                done[k] = sim.run_plans(steps)
                th.cuda.current_stream().synchronize()
        except Exception as e:      # noqa: BLE001
            errs.append(e)
            for b in (t_ready, t_go):
                b.abort()

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(n)]
    for t in ths:
        t.start()
    t_ready.wait()
    ready.wait()
    go.wait()
    t0 = time.time()
    t_go.wait()
    for t in ths:
        t.join()
    if errs:
        raise errs[0]
    q.put((g, sum(done), t0, time.time(), sum(s[0].scen_tree_gen.n_expanded for s in sims)))


def run_concurrent_groups(args):
    """BASELINE config 3 at the size that fills the GPU: P scenes as P / Q host processes of Q scenes each -- the interpreter work of the scenes
    (about 0.9 ms per plan, the bound of the one-thread event loop) runs on P / Q cores, the device sees P / Q contexts instead of P (sixteen
    processes time-slice it: profiles/r05l_*)."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    P, Q = args.concurrent, args.per_process
    groups = [list(range(a, min(a + Q, P))) for a in range(0, P, Q)]
    G = len(groups)
    ready, go, q = ctx.Barrier(G + 1), ctx.Barrier(G + 1), ctx.Queue()
    procs = [ctx.Process(target=_proc_group, args=(g, ids, args.workload, args.steps, args.warmup, ready, go, q, args.ckpt)) for g, ids in enumerate(groups)]
    for p_ in procs:
        p_.start()
    ready.wait(timeout=900)
    go.wait(timeout=60)
    res = [q.get(timeout=900) for _ in range(G)]
    for p_ in procs:
        p_.join(timeout=60)
    dt = max(r[3] for r in res) - min(r[2] for r in res)       # same host clock: first start to last finish
    steps = sum(r[1] for r in res)
    print(json.dumps({
        "metric": METRIC, "value": steps / dt, "unit": "sim steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16x3 pair kernel / f32 predictor / f64 iLQR", "data": _concurrent_label(args.workload, P)[1],
        "config": {"workload": f"{_concurrent_label(args.workload, P)[0]} planned concurrently on one GPU: {G} host processes, each ONE thread over "
                               f"{Q} scenes (a HIP context + stream per scene, event loop over three-piece plans), {args.steps} planning cycles each",
                   "concurrent_scenes": P, "host_processes": G, "scenes_per_process": Q, "sim_steps_timed": steps},
        "ms_per_plan_aggregate": dt / (args.steps * P) * 1e3}))


def run_concurrent_processes(args):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    P = args.concurrent
    ready, go, q = ctx.Barrier(P + 1), ctx.Barrier(P + 1), ctx.Queue()
    procs = [ctx.Process(target=_proc_scene, args=(i, args.workload, args.steps, args.warmup, ready, go, q, P <= 4, args.ckpt)) for i in range(P)]
    for p_ in procs:
        p_.start()
    ready.wait(timeout=600)
    go.wait(timeout=60)
    res = [q.get(timeout=600) for _ in range(P)]
    for p_ in procs:
        p_.join(timeout=60)
    dt = max(r[3] for r in res) - min(r[2] for r in res)       # same host clock: first start to last finish
    steps = sum(r[1] for r in res)
    print(json.dumps({
        "metric": METRIC, "value": steps / dt, "unit": "sim steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 predictor / f64 iLQR", "data": _concurrent_label(args.workload, P)[1],
        "config": {"workload": f"{_concurrent_label(args.workload, P)[0]} planned concurrently on one GPU (one host process + HIP "
                               f"context per scene), {args.steps} planning cycles each", "concurrent_scenes": P,
                   "sim_steps_timed": steps},
        "ms_per_plan_aggregate": dt / (args.steps * P) * 1e3}))


def run_concurrent(args):
    """P closed loops (different scenes) in P host threads, each with its own HIP context on its own stream: the
    GPU work of one scene overlaps the host bookkeeping and the GPU work of the others."""
    import threading
    P = args.concurrent
    if os.environ.get("MIND_SWITCH_INTERVAL"):
        sys.setswitchinterval(float(os.environ["MIND_SWITCH_INTERVAL"]))
    loops, errs = [None] * P, []
    ready, go = threading.Barrier(P + 1), threading.Barrier(P + 1)
    done_steps = [0] * P

    def worker(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                # (the native loop -- one C call for the thread's whole run, the interpreter lock released -- where it applies: recorded scenes)
                pl, sim, w = make_closed_loop(scene_workload(args.workload, i), full_tree=args.workload in FULL_TREE, speculative=P <= 4, ckpt=args.ckpt,
                                              native=CONCURRENT_NATIVE)
                sim.run_plans(max(args.warmup, 1))
                torch.cuda.current_stream().synchronize()
                loops[i] = (pl, sim)
                ready.wait()
                go.wait()
                done_steps[i] = sim.run_plans(args.steps)
                torch.cuda.current_stream().synchronize()
        except Exception as e:           # surface the failure instead of dead-locking the barriers
            errs.append(e)
            for b in (ready, go):
                b.abort()

    ths = [threading.Thread(target=worker, args=(i,)) for i in range(P)]
    for t in ths:
        t.start()
    ready.wait()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go.wait()
    for t in ths:
        t.join()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if errs:
        raise errs[0]
    steps = sum(done_steps)
    print(json.dumps({
        "metric": METRIC, "value": steps / dt, "unit": "sim steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 predictor / f64 iLQR", "data": _concurrent_label(args.workload, P)[1],
        "config": {"workload": f"{_concurrent_label(args.workload, P)[0]} planned concurrently on one GPU (one host thread + HIP "
                               f"context + stream per scene), {args.steps} planning cycles each", "concurrent_scenes": P,
                   "sim_steps_timed": steps},
        "ms_per_plan_aggregate": dt / (args.steps * P) * 1e3}))


def run_pipelined(args):
    """P closed loops in ONE process and ONE host thread, every planner on its own HIP context / stream, scene i's contingency solves on
    the device beside scene i + 1's AIME rounds (mind_amd.pipelined)."""
    from mind_amd.pipelined import PipelinedClosedLoops
    P = args.concurrent
    loops = [make_closed_loop(scene_workload(args.workload, i), scripted="scene" not in scene_workload(args.workload, i), speculative=False, ckpt=args.ckpt,
                              own_context=True) for i in range(P)]
    pc = PipelinedClosedLoops([l[1] for l in loops])
    pc.run_plans(max(args.warmup, 1))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = pc.run_plans(args.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({
        "metric": METRIC, "value": steps / dt, "unit": "sim steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16x3 pair kernel / f32 predictor / f64 iLQR", "data": _concurrent_label(args.workload, P)[1],
        "config": {"workload": f"{_concurrent_label(args.workload, P)[0]} planned from ONE host thread, one HIP context + stream per scene, "
                               f"scene i's tree-iLQR on the device beside scene i + 1's AIME rounds, {args.steps} planning cycles each",
                   "concurrent_scenes": P, "sim_steps_timed": steps},
        "ms_per_plan_aggregate": dt / (args.steps * P) * 1e3}))


def run_fused(args):
    """BASELINE config 3 as written: P closed loops in ONE process, the AIME rounds of all scenes merged into one predictor
    batch per round (mind_amd.fused); to be compared with --concurrent P --processes (one process per scene)."""
    from mind_amd.fused import FusedClosedLoops
    P = args.concurrent
    loops = [make_closed_loop(scene_workload(args.workload, i), scripted=False, speculative=False, ckpt=args.ckpt) for i in range(P)]
    fl = FusedClosedLoops([l[1] for l in loops])
    fl.run_plans(max(args.warmup, 1))
    torch.cuda.synchronize()
    n0 = sum(l[0].scen_tree_gen.n_expanded for l in loops)
    c0, sc0 = fl.fused.n_calls, fl.fused.n_scenes
    t0 = time.perf_counter()
    steps = fl.run_plans(args.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    plans = sum(l[1].n_plans for l in loops)
    print(json.dumps({
        "metric": METRIC, "value": steps / dt, "unit": "sim steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16x3 pair kernel / f32 predictor / f64 iLQR", "data": _concurrent_label(args.workload, P)[1],
        "nodes_expanded_per_s": (sum(l[0].scen_tree_gen.n_expanded for l in loops) - n0) / dt,
        "config": {"workload": f"{_concurrent_label(args.workload, P)[0]} planned by ONE process, the AIME rounds of all scenes fused into one "
                               f"predictor batch per round, {args.steps} planning cycles each", "concurrent_scenes": P, "sim_steps_timed": steps,
                   "weights": args.ckpt or "formula:20240121"},
        "predictor_calls": fl.fused.n_calls - c0, "scenes_per_predictor_call": (fl.fused.n_scenes - sc0) / max(fl.fused.n_calls - c0, 1),
        "ms_per_plan_aggregate": dt / (args.steps * P) * 1e3}))


def config3_block(P=4, steps=20, warmup=3):
    """BASELINE configs[2] (demo_1..4 concurrently on one GPU) for the default line: two sibling runs of this script, `--concurrent P
    --processes` (a host process + HIP context per scene) and `--concurrent P --pipelined` (ONE process, one host thread, a context per scene),
    each reporting the aggregate rate of its P closed loops."""
    out = {"scenes": P, "workload": "the recorded scenes demo_1..4, one closed loop each, planned concurrently on one GPU"}
    for mode, key in (("--processes", "processes"), ("--pipelined", "one_thread_event_loop")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", "demo_all", "--concurrent", str(P), mode, "--steps", str(steps),
                                "--warmup", str(warmup), "--no-cpu-baseline", "--no-extras", "--no-traffic"], capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                out[key] = {"error": (r.stderr or "no output")[-200:]}
                continue
            d = json.loads(line[-1])
            out[key] = {"sim_steps_per_s": d["value"], "ms_per_round_of_plans": d["ms_per_step"]}
        except Exception as e:      # noqa: BLE001
            out[key] = {"error": f"{type(e).__name__}: {e}"[:200]}
    best = max((v["sim_steps_per_s"] for v in out.values() if isinstance(v, dict) and "sim_steps_per_s" in v), default=None)
    out["sim_steps_per_s"] = best
    # the size that fills the device: sixteen scenes as two host processes of eight (profiles/r05z_config3_groups.txt: two processes are the
    # optimum from eight scenes on -- the interpreter work on two cores, two contexts on the device without time-slicing)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", "demo_all", "--concurrent", "16", "--processes", "--per-process", "8",
                            "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extras", "--no-traffic"], capture_output=True, text=True,
                           timeout=400)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode == 0 and line:
            d = json.loads(line[-1])
            out["sixteen_scenes_two_processes"] = {"sim_steps_per_s": d["value"], "ms_per_round_of_plans": d["ms_per_step"]}
        else:
            out["sixteen_scenes_two_processes"] = {"error": (r.stderr or "no output")[-200:]}
    except Exception as e:      # noqa: BLE001
        out["sixteen_scenes_two_processes"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return out


# ---- the contract line ------------------------------------------------------------------------------------------------------
EXTRAS_FILE = "bench_extras.json"
LINE_LIMIT = 4096


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def dump_outputs(m, d):
    """--dump-outputs DIR: what the last timed planning cycle handed its caller (MINDPlanner.plan's control and
    [[scenario tree], [trajectory tree]], the closed loop's ego state), one float64 .npy per array, a few KB in all.  The inputs
    (recorded scene or seeded synthetic world, formula weights) are the same from run to run, so two builds compare file by file."""
    os.makedirs(d, exist_ok=True)
    pl, sim = m["pl"], m["sim"]
    scen, traj = sim.last_result
    tt, st = traj[0], scen[0]
    keys = list(st.nodes)
    arrs = {"ego_state": sim.state, "ctrl": sim.ctrl, "traj_xs": tt._arrays[0], "traj_us": tt._arrays[1],
            "tree_costs": pl.timing["tree_costs"], "best_tree": [pl.timing["best_traj_idx"]],
            # scenario tree of the chosen plan, nodes in insertion order: parent index (-1 = root), then the probability, predicted positions,
            # covariances and target points of every node, flattened and concatenated, with each node's element count
            "scen_parent": [keys.index(st.nodes[k].parent_key) if st.nodes[k].parent_key in st.nodes else -1 for k in keys]}
    for i, name in enumerate(("scen_prob", "scen_pos", "scen_cov", "scen_tgt")):
        parts = [_f64(st.nodes[k].data[i]).ravel() for k in keys]
        arrs[name] = np.concatenate(parts) if parts else np.zeros(0)
        arrs[name + "_sizes"] = [p.size for p in parts]
    for name, v in arrs.items():
        np.save(os.path.join(d, name + ".npy"), _f64(v))


def _sig(v, n=5):
    """floats to n significant digits (the line is a record, not an archive); containers recursively"""
    if isinstance(v, float):
        return float(f"{v:.{n}g}")
    if isinstance(v, dict):
        return {k: _sig(x, n) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, n) for x in v]
    return v


def contract_line(out, args):
    """ONE compact JSON line (< 4 KB) with the driver's contract keys, `roofline`, `cpu_baseline` and the few scalars of the other
    measurements a reader needs; every block of the run in full goes to bench_extras.json beside this script (named in the line)."""
    path = os.environ.get("MIND_BENCH_EXTRAS", os.path.join(ROOT, EXTRAS_FILE))
    try:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        extras = os.path.relpath(path, ROOT) if path.startswith(ROOT) else path
    except OSError as e:
        extras = f"not written ({type(e).__name__})"

    def pick(d, *keys):
        return {k: d[k] for k in keys if isinstance(d, dict) and k in d}

    line = pick(out, "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "measured_after_warmup")
    line["config"] = pick(out["config"], "workload", "agents", "lane_polylines", "expansions_per_plan", "scenario_trees_per_plan", "weights", "parallelism", "sim_steps_timed")
    line["nodes_expanded_per_s"] = out.get("nodes_expanded_per_s")
    r = out.get("roofline")
    if r:
        line["roofline"] = dict(pick(r, "kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_ms",
                                     "launches_profiled"), hbm_frac=r["hbm"]["frac"], mfma_frac=r["mfma"]["frac"], arith=r["mfma"]["arith"])
    else:
        line["roofline"] = None
    c = out.get("cpu_baseline")
    if c:
        line["cpu_baseline"] = pick(c, "value", "unit", "cores", "kind", "cpu", "hardware_threads", "value_1_thread", "sample")
    k = out.get("k_ilqr")
    if k:
        line["k_ilqr"] = pick(k, "kernel_ms_per_launch", "share_of_step", "cost_trees_per_launch", "cus_busy")
    line["breakdown_ms"] = pick(out.get("breakdown_ms") or {}, "aime", "ilqr")
    if "bf16x3" in out:
        line["bf16x3"] = pick(out["bf16x3"], "value", "ms_per_step", "hbm_frac")
    for key in ("tree_f32", "tree", "tree_sharded", "tree_replicas", "stress", "stress_bf16", "stress_deep", "stress_deeper"):
        t = out.get(key)
        if not isinstance(t, dict):
            continue
        if "error" in t:
            line[key] = {"error": t["error"][:120]}
            continue
        b = pick(t, "ms_per_plan", "nodes_expanded_per_s", "k_ilqr_ms_per_launch", "gathered_mb_per_plan", "collectives_per_plan", "speedup_vs_1")
        if "k_pair" in t:
            b["k_pair"] = pick(t["k_pair"], "hbm_frac", "mfma_frac", "avg_launch_ms")
        line[key] = b
    for key in ("collectives_per_plan", "gathered_mb_per_plan"):
        if key in out:
            line[key] = out[key]
    c3 = out.get("config3")
    if isinstance(c3, dict):
        line["config3"] = {"scenes": c3.get("scenes"), "sim_steps_per_s": c3.get("sim_steps_per_s"),
                           "processes": (c3.get("processes") or {}).get("sim_steps_per_s"),
                           "one_thread_event_loop": (c3.get("one_thread_event_loop") or {}).get("sim_steps_per_s"),
                           "x16_two_processes": (c3.get("sixteen_scenes_two_processes") or {}).get("sim_steps_per_s")}
    line["extras_file"] = extras
    text = json.dumps(_sig(line), separators=(",", ":"))
    if len(text) > LINE_LIMIT:          # never let an extra cost the contract line: drop the optional blocks, largest first
        for key in ("stress_deep", "stress_bf16", "stress", "stress_deeper", "config3", "tree_replicas", "breakdown_ms", "k_ilqr", "tree", "tree_sharded"):
            line.pop(key, None)
            text = json.dumps(_sig(line), separators=(",", ":"))
            if len(text) <= LINE_LIMIT:
                break
    return text


# ---- launch ---------------------------------------------------------------------------------------------------------------
def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks through torch.distributed.run (one process per
    GPU, rendezvous on 127.0.0.1) and pass their output through."""
    n_dev = torch.cuda.device_count()
    if args.backend == "nccl" and n_dev < args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} needs {args.gpus} devices, {n_dev} visible (RCCL runs one rank per GPU; "
                         f"--backend gloo shares a device between ranks, for tests only)")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="demo_1", choices=list(WORKLOADS))
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for --gpus N > 1 (nccl = RCCL; gloo only for tests on a single-GPU box)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-traffic", action="store_true", help="skip the two rocprofv3 --pmc sibling runs that fill roofline.traffic")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra workloads (synthetic branching, cfg4 tree, other recorded scenes)")
    ap.add_argument("--tree-steps", type=int, default=20, help="planning cycles of the extra cfg4-tree measurement")
    ap.add_argument("--concurrent", type=int, default=0,
                    help="BASELINE config 3: plan this many independent scenes concurrently on the GPU (one host thread, "
                         "HIP context and stream per scene); prints the aggregate rate")
    ap.add_argument("--processes", action="store_true",
                    help="with --concurrent: one host PROCESS per scene instead of one thread (host bookkeeping in parallel too)")
    ap.add_argument("--per-process", type=int, default=1,
                    help="with --concurrent P --processes: Q scenes per host process (P / Q processes, each one thread over its Q scenes as --pipelined)")
    ap.add_argument("--pipelined", action="store_true",
                    help="with --concurrent P: one process, one host thread, a context per scene, scene i's tree-iLQR beside scene i + 1's AIME rounds")
    ap.add_argument("--fused", action="store_true",
                    help="with --concurrent: ONE process, the scenes' AIME rounds fused into one predictor batch (BASELINE config 3 as written)")
    ap.add_argument("--ckpt", default=None, help='planner ckpt_path override, e.g. "formula_branching:20240121" (mind_amd/weights.py) or a .tar')
    ap.add_argument("--shard", action="store_true",
                    help="strong scaling: all ranks plan the SAME scene, AIME rounds and contingency solves sharded over ranks "
                         "(the default for the full-tree workloads)")
    ap.add_argument("--replicas", action="store_true", help="N > 1: independent closed loops per rank even for a full-tree workload")
    ap.add_argument("--prec", default=HEADLINE_PREC, choices=list(PREC_DTYPE),
                    help="arithmetic of the predictor's MFMA contractions for the headline measurement (default: the fp32-class one; bf16x3 is reported beside it)")
    ap.add_argument("--headline-first", action="store_true", help="with --full: measure the headline before the extra workloads (the default runs them first: a fresh box warms up on them)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: the extra workloads and precisions, the rocprofv3 traffic passes and the CPU baseline "
                         "(a plain run sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed planning cycle handed its caller as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args, sys.argv[1:])
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if world_env != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world_env} ranks")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.backend == "gloo":
        local = local % torch.cuda.device_count()
        os.environ["LOCAL_RANK"] = str(local)
    torch.cuda.set_device(local)
    if os.environ.get("MIND_BENCH_OWN_STREAM", "1") == "1":
        # the planner's context stream = a non-blocking stream of torch's pool instead of the legacy default stream (whose
        # synchronisations also cover other blocking streams): measured +1 % on demo_1 and cfg4tree (profiles/r02am_*)
        torch.cuda.set_stream(torch.cuda.Stream())
    dist = Dist(args.backend, local)
    rank, world = dist.rank, dist.world
    if args.concurrent > 1:
        if args.fused:
            return run_fused(args)
        if args.pipelined:
            return run_pipelined(args)
        if args.processes and args.per_process > 1:
            return run_concurrent_groups(args)
        return run_concurrent_processes(args) if args.processes else run_concurrent(args)
    shard = world > 1 and not args.replicas and (args.shard or args.workload in FULL_TREE)
    extras = args.full and not args.no_extras and args.workload == "demo_1"
    # With --full, the demo-size measurements of the line (plain weights, synthetic branching, the other recorded scenes, config 3, exact fp32: seconds of
    # closed loops) run BEFORE the headline: a fresh box needs a few seconds of work to reach its steady state -- the first
    # invocation of the day measured the same AIME rounds at 2.07 ms of host wall instead of 1.78 (profiles/r05v_*: 1 233-1 374 sim steps/s
    # first, 1 470-1 500 from the second process on) -- and the closed loop's rate is what a loop that has been running delivers.  The full-tree
    # workloads run AFTER it (behind their 200 GB arenas the same process runs the small loop 10 % slower).  --headline-first: the old order.
    # Every measurement builds its own planner and closed loop.
    pre = {}

    def run_small_extras():
        if extras and rank == 0 and world == 1:
            pm = measure(dist, "demo_1", args.steps, args.warmup, False, ckpt=PLAIN_WEIGHTS)
            pre["plain_formula_weights"] = dict(summarize(pm, pm["pl"].network.rt.pair_precision()), workload="recorded demo_1 with the plain formula weights (all modes merge: one expansion per plan)")
            pre["synthetic_branching"] = dict((lambda sb_: summarize(sb_, sb_["pl"].network.rt.pair_precision()))(measure(dist, "demo1", args.steps, args.warmup, False)),
                                              workload="demo_1-like synthetic scene, scripted mode branching on the real predictor forward")
            pre["recorded_scenes"] = recorded_scenes(pm["pl"].network.rt.pair_precision())
            pre["config3"] = config3_block()

    def run_extras(small):
        if small:
            return run_small_extras()
        if extras and rank == 0 and world == 1:
            # the headline workload under the two-way split (bf16 hi + lo operands: 16 significand bits, narrower than the reference's fp32 --
            # reported beside the credited fp32-class figures, never in their place)
            if args.prec != "bf16x3":
                fm = measure(dist, "demo_1", args.steps, args.warmup, False, pair_prec="bf16x3")
                fr = roofline(fm, "bf16x3")
                pre["bf16x3"] = {"value": fm["sim_steps"] / fm["dt"], "unit": "sim steps/s", "ms_per_step": fm["dt"] / fm["steps"] * 1e3,
                                 "pair_kernel_avg_launch_ms": fr["avg_launch_ms"] if fr else None,
                                 "hbm_frac": fr["hbm"]["frac"] if fr else None, "mfma_frac": fr["mfma"]["frac"] if fr else None,
                                 "k_ilqr_ms_per_launch": (fm["ilqr_kernel"]["ms"] / fm["ilqr_kernel"]["launches"]) if fm["ilqr_kernel"]["launches"] else None,
                                 "note": "same workload with the pair kernel / ActorNet operands split two ways (bf16 hi + lo, 3 products per term): "
                                         "meets the 2e-4 m parity bar but is narrower than the reference's fp32, hence an extra"}
        if extras:
            # the full cfg4 scenario tree (259 expansions per plan): on one GPU, or planned once by all ranks together.  A failure
            # here must not cost the headline line (every rank reaches the same except branch or none does: the plan is replicated)
            key = "tree_sharded" if world > 1 else "tree"
            try:
                # (one GPU: `tree` is the opt-in two-way split, the series of rounds 2-5; `tree_f32` below is the same tree in the headline's fp32-class
                # arithmetic, the library's default.  Several GPUs: the sharded tree runs in the headline's arithmetic)
                tprec = "bf16x3" if world == 1 else args.prec
                t = measure(dist, "cfg4tree", args.tree_steps, 2, world > 1, pair_prec=tprec)      # two warm-up plans: the arenas and table caches reach their final sizes
                pre[key] = dict(summarize(t, tprec), arith=tprec, workload="cfg4tree: 64 agents x 256 lane polylines, full scripted 6-ary "
                                "depth-4 AIME tree on the real predictor forward", n_gpus=world,
                                scaling="strong" if world > 1 else None, plans_timed=args.tree_steps)
            except Exception as e:       # noqa: BLE001
                pre[key] = {"error": f"{type(e).__name__}: {e}"[:400]}
            if world == 1 and args.prec != "bf16x3":
                # ... and in the headline's fp32-class arithmetic (the figure that carries credit for BASELINE configs[3] on one GPU)
                try:
                    t = measure(dist, "cfg4tree", max(args.tree_steps // 2, 2), 2, False, pair_prec=args.prec)
                    pre["tree_f32"] = dict(summarize(t, args.prec), arith=args.prec, workload="cfg4tree in the headline's fp32-class arithmetic (" + PREC_DTYPE[args.prec] + ")",
                                           plans_timed=max(args.tree_steps // 2, 2))
                except Exception as e:       # noqa: BLE001
                    pre["tree_f32"] = {"error": f"{type(e).__name__}: {e}"[:400]}
            if world > 1:
                # the same full tree planned by every rank for a scene of its own (independent trees, no data-path collective): the node
                # throughput of the whole job when the scenes, not one scene's branches, are what is spread over the GPUs
                try:
                    t = measure(dist, "cfg4tree", args.tree_steps, 2, False, replica=rank, pair_prec=args.prec)
                    pre["tree_replicas"] = dict(summarize(t, args.prec), arith=args.prec, workload="cfg4tree on every rank, one independent scene per rank (full scripted 6-ary "
                                                "depth-4 AIME tree on the real predictor forward); nodes_expanded_per_s is the whole job's", n_gpus=world,
                                                scaling="weak", plans_timed=args.tree_steps)
                    if "ms_per_plan" in pre.get("tree_sharded", {}):
                        # the same tree on one GPU (a replica's plan) over the plan all ranks share: north_star's strong-scaling figure
                        pre["tree_sharded"]["speedup_vs_1"] = pre["tree_replicas"]["ms_per_plan"] / pre["tree_sharded"]["ms_per_plan"]
                except Exception as e:       # noqa: BLE001
                    pre["tree_replicas"] = {"error": f"{type(e).__name__}: {e}"[:400]}
        if extras and rank == 0 and world == 1:
            try:
                sm = measure(dist, "stress128tree", 6, 2, False, pair_prec="bf16x3")
                pre["stress"] = dict(summarize(sm, "bf16x3"), arith="bf16x3", workload="stress128tree: 128 agents x 256 lane polylines (N = 385), full scripted 6-ary depth-4 AIME "
                                     "tree (259 expansions per plan: the largest tree the reference's probability floor lets grow), two-way split (bf16x3)",
                                     plans_timed=6)
                bm = measure(dist, "stress128tree", 6, 2, False, pair_prec="bf16")
                pre["stress_bf16"] = dict(summarize(bm, "bf16"), workload="the same in plain bf16 (BASELINE config 5's 'bf16 MFMA attention'; misses the 1e-3 m bar)",
                                          plans_timed=6)
            except Exception as e:       # noqa: BLE001
                pre["stress"] = {"error": f"{type(e).__name__}: {e}"[:400]}
            try:
                # the deepest tree K = 6 modes allow (ScriptedDeepTree: floor lifted, five rounds, the last one 1 296 scenes = 51 GB of bf16
                # edges, through the predictor in chunks under the default 96 GB budget only if it had to)
                dm = measure(dist, "stressdeep", 2, 1, False, pair_prec="bf16")
                pre["stress_deep"] = dict(summarize(dm, "bf16"), workload="stressdeep: 128 agents x 256 lane polylines (N = 385), scripted 6-ary depth-5 AIME tree with "
                                          "the path-probability floor lifted (rounds of 1 / 6 / 36 / 216 / 1 296 scenes = 1 555 expansions, 7 776 leaves per "
                                          "plan), plain bf16 (edge tensor in bf16)", plans_timed=2)
            except Exception as e:       # noqa: BLE001
                pre["stress_deep"] = {"error": f"{type(e).__name__}: {e}"[:400]}
            try:
                # one level deeper (ScriptedDeeperTree): six rounds, the last one 7 776 scenes = 307 GB of bf16 edges, in chunks under a
                # 64 GB budget (about 200 GB of the 288 GB in use); one plan timed behind one warm-up plan (arena growth)
                xm = measure(dist, "stressdeeper", 1, 1, False, pair_prec="bf16", tuning={"plan_chunk_mb": (64 * 1024, 96 * 1024)})
                pre["stress_deeper"] = dict(summarize(xm, "bf16"), workload="stressdeeper: the same scene under the scripted 6-ary depth-6 tree (BASELINE configs[4]'s "
                                            "depth at the branching K = 6 modes allow): rounds of 1 / 6 / 36 / 216 / 1 296 / 7 776 scenes = 9 331 expansions, 46 656 "
                                            "leaves per plan, the last round in chunks under a 64 GB edge budget, plain bf16", plans_timed=1)
            except Exception as e:       # noqa: BLE001
                pre["stress_deeper"] = {"error": f"{type(e).__name__}: {e}"[:400]}

    def run_extras_guarded(small):
        try:
            run_extras(small)
        except Exception as e:       # noqa: BLE001      (an extra must never cost the headline line)
            pre["extras_error"] = f"{type(e).__name__}: {e}"[:400]

    if not args.headline_first:
        run_extras_guarded(True)
    m = measure(dist, args.workload, args.steps, args.warmup, shard, replica=0 if shard else rank, ckpt=args.ckpt, pair_prec=args.prec)
    pl, sim = m["pl"], m["sim"]
    prec = args.prec
    value = m["sim_steps"] * (1 if shard else world) / m["dt"]
    a, l = m["a"], m["l"]
    exp_plan = m["expansions_all"] / args.steps / (1 if shard else world)
    ctr = m["ilqr"]
    real = m["real_scene"]
    out = {
        "metric": METRIC, "value": value, "unit": "sim steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": m["dt"] / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if shard else "weak", "vs_baseline": None,
        "dtype": PREC_DTYPE[prec] + " pair kernel + ActorNet, f32 elsewhere in the predictor, f64 iLQR",
        # the headline loop runs behind a few seconds of the small extra workloads (a fresh box reaches its steady state on them: the first
        # invocation on a cold box measured 1 233-1 374 where every later one measured 1 470-1 500, profiles/r05v_*); --headline-first measures it cold
        "measured_after_warmup": bool(extras and not args.headline_first),
        "data": ("recorded AV2 scene (map + tracks of the reference's %s, tests/golden/scenes), formula-initialised weights" % args.workload) if real else "synthetic",
        "nodes_expanded_per_s": m["expansions_all"] / m["dt"],
        "config": {"workload": (f"BASELINE configs[1]: closed loop on the recorded scene {args.workload}" if real else f"{args.workload}-like synthetic scene") +
                               f", {a} agents x {l} lane polylines (N={a+l+1}); step = one planning cycle (5 simulator steps of 0.02 s): AIME tree "
                               f"({exp_plan:.1f} expansions, " + ("the predictor's own modes" if real else "scripted mode branching on the real predictor forward") +
                               f") + tree-iLQR warm+full solves of {pl.timing['n_scen_trees']} scenario trees",
                   "agents": a, "lane_polylines": l, "expansions_per_plan": exp_plan, "sim_steps_timed": m["sim_steps"],
                   "scenario_trees_per_plan": pl.timing["n_scen_trees"], "weights": m["weights"],
                   "parallelism": (f"one plan sharded over {world} GPUs (AIME rounds block-sharded, solves round-robin)" if shard
                                   else f"{world} independent closed loop(s), one per GPU, no data-path collective")},
        "roofline": roofline(m, prec),
        # the tree-iLQR kernel is latency-bound (serial depth x iterations): reported as rates, not against a roofline
        "ilqr": {"solves_per_s": ctr["solves"] / m["dt"], "iterations_per_s": ctr["iterations"] / m["dt"],
                 "trees_per_plan": ctr["solves"] / max(args.steps, 1) / 2, "iterations_per_solve": ctr["iterations"] / max(ctr["solves"], 1),
                 "warm_start_fits_speculated": ctr["warm_speculated"], "warm_start_fits_reused": ctr["warm_hits"],
                 "kernel_ms_per_launch": (m["ilqr_kernel"]["ms"] / m["ilqr_kernel"]["launches"]) if m["ilqr_kernel"]["launches"] else None,
                 "kernel_launches_timed": m["ilqr_kernel"]["launches"], "workgroups_per_tree": m["ilqr_kernel"]["wgs"],
                 "note": "per rank; kernel_ms_per_launch = k_ilqr (warm-start fit + full fit of all scenario trees of a plan) from HIP events on the context stream; every scenario tree is solved twice per plan (warm start, then full cost); the warm-start fits of "
                         "the previous cycle's tree shapes run beside the predictor and are reused where the shape recurs"},
        "breakdown_ms": m["breakdown_ms"],
        "k_ilqr": ilqr_block(m),
    }
    if m["collectives"] is not None:
        out["collectives_per_plan"] = m["collectives"][0] / args.steps
        out["gathered_mb_per_plan"] = m["collectives"][1] / args.steps / 1e6
    if args.dump_outputs and rank == 0:
        dump_outputs(m, args.dump_outputs)
    if args.headline_first:
        run_extras_guarded(True)
    run_extras_guarded(False)
    out.update(pre)
    if rank == 0 and world == 1 and args.full:
        if not args.no_traffic and out.get("roofline"):
            tb, det = measure_traffic(args.workload, out["roofline"]["algorithmic_bytes_per_launch"], prec=args.prec)
            out["roofline"]["traffic"] = tb
            out["roofline"]["traffic_detail"] = det
        if not args.no_cpu_baseline:
            if getattr(sim, "_native", None) is not None:
                sim._native.hand_back()          # (the oracle's sample is a plan's scenario trees and observation windows: back to Python objects,
                sim.run_plans(1)                 #  one cycle of the Python steps builds them)
            lcl = sim._observation()
            out["cpu_baseline"] = cpu_baseline(pl, lcl, (a, l), max(int(round(exp_plan)), 1), pl.scen_tree_gen.get_scenario_tree(),
                                               trees_per_plan=m["ilqr"].get("solves", 0) / 2.0 / max(m["steps"], 1))
    if rank == 0:
        print(contract_line(out, args))
    dist.close()


if __name__ == "__main__":
    main()
