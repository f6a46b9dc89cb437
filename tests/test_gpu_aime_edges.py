"""GPU: the AIME glue kernels (k_aime_world, k_aime_select, k_aime_branch, k_aime_select_branch, k_aime_rebase) on the edge families of
tests/aime_edge_cases.py against the float64 restatement tests/aime_restate.py.

Continuous outputs: e_ref = error of the float32 HOST path against the float64 truth, e_hip = the kernel's; the bar is
e_hip <= 4 e_ref + floor (the factor of tests/test_gpu_predictor_regimes.py for two independent float32 evaluations of one quantity;
floor = one float32 ulp at the largest magnitude of the compared quantity -- the world coordinate for world-frame lengths, ego-frame metres
for re-based ones -- and one ulp of pi for angles and unit vectors; one bar per scene in the re-basing families).  The bar never reads the
kernel's output.  Every case prints `family output e_ref e_hip bar` (profiles/aime_edges.txt holds one run).  Bit-level facts (one-hot and
pad rows, ORIG, the target window and its info rows, max-sigma + last covariance, the ego's zero signature) and every decision (kept
modes, their probabilities, the branch-time words, the window index) are asserted exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aime_edge_cases as EC  # noqa: E402
import aime_restate as R  # noqa: E402
from test_aime_restate_host import DECIDE, REBASE, WORLD, decide_truth, host_rebase, host_world, true_rebase, true_world, ulp32  # noqa: E402

from mind_amd._lib import MindError  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ULP_PI = float(np.spacing(F32(np.pi)))
CLS = np.array([0.1, 0.14, 0.3, 0.11, 0.15, 0.2], F32)          # the modes 30 m off the lane (2, 5) lead: the lane test decides who is first


class Table:
    def __init__(self, family):
        self.family, self.rows, self.bad = family, {}, []

    def add(self, output, hip, host, truth, floor):
        hip, host, truth = np.asarray(hip, np.float64), np.asarray(host, np.float64), np.asarray(truth, np.float64)
        assert np.array_equal(np.isnan(hip), np.isnan(truth)), (self.family, output, "NaN pattern")
        ok = np.isfinite(truth)
        assert np.array_equal(hip[~ok & ~np.isnan(truth)], truth[~ok & ~np.isnan(truth)])
        e_ref = float(np.abs(host - truth)[ok].max()) if ok.any() else 0.0
        e_hip = float(np.abs(hip - truth)[ok].max()) if ok.any() else 0.0
        r = self.rows.setdefault(output, [0.0, 0.0, floor])
        r[0], r[1], r[2] = max(r[0], e_ref), max(r[1], e_hip), max(r[2], floor)

    def check(self):
        for output, (e_ref, e_hip, floor) in self.rows.items():
            bar = 4 * e_ref + floor
            print(f"{self.family} {output} {e_ref:.3e} {e_hip:.3e} {bar:.3e}")
            if not e_hip <= bar:
                self.bad.append((output, e_ref, e_hip, bar))
        assert not self.bad, (self.family, self.bad)


def _run_world(hp, c, n_scenes=None, decide=False):
    B = n_scenes or len(c["a_off"]) - 1
    A = int(c["a_off"][B])
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x[:A])).to(hp.device)
    kw = dict(cls=g(np.tile(CLS, (B, 1))), scen_prob=np.ones(B, F32), dist_thres=c["dist_thres"]) if decide else {}
    w = hp.aime_world(g(c["reg"]), g(c["vel"]), g(c["ctrs"]), g(c["vecs"]), c["a_off"][:B + 1], c["rots"][:B], c["origs"][:B], c["cov_last"][:A],
                      c["last"][:B], target_lane=c["lane"], **kw)
    return {k: v.cpu().numpy() for k, v in w.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("name,c", WORLD, ids=[n for n, _ in WORLD])
def test_world_kernel_on_the_edge_families(hip_predictor, name, c):
    w = _run_world(hip_predictor, c)
    world, topo, end = w["world"], w["topo"], w["ego_end"]
    tab = Table(name)
    for b in range(len(c["a_off"]) - 1):
        sl = slice(c["a_off"][b], c["a_off"][b + 1])
        h, t = host_world(c, b), true_world(c, b)
        pfloor = ulp32(max(np.abs(t["pos"]).max(), 1.0))
        tab.add("pos", world[sl, ..., 0:2], h["pos"], t["pos"], pfloor)
        tab.add("vel", world[sl, ..., 2:4], h["vel"], t["vel"], ulp32(max(np.abs(t["vel"]).max(), 1.0)))
        tab.add("heading", world[sl, ..., 4], h["ang"], t["ang"], ULP_PI)
        assert np.array_equal(world[sl, ..., 5], t["cov"]), (name, b)              # max(sigma_x, sigma_y) + cov_last, bit for bit
        assert not topo[c["a_off"][b]].any()                                        # the ego's own signature is 0
        if t["topo"].size:
            tab.add("topo", topo[sl][1:], h["topo"], t["topo"], ULP_PI)
        if t["end"] is not None:
            tab.add("ego_end_xy", end[b, :, :2], h["end"][:, :2], t["end"][:, :2], pfloor)
            assert np.array_equal(end[b, :, 2], t["cov"][0, :, c["last"][b]])
            if c["lane"] is not None:
                tab.add("ego_end_dist", end[b, :, 3], h["end"][:, 3], t["end"][:, 3], pfloor)
            else:
                assert np.isinf(end[b, :, 3]).all()
    tab.check()


LANE_TESTED = [(n, c) for n, c in WORLD if c["dist_thres"] is not None]


@pytest.mark.parametrize("name,c", LANE_TESTED, ids=[n for n, _ in LANE_TESTED])
def test_lane_pruning_decisions_equal_the_reference_loop(hip_predictor, name, c):
    """keep-or-prune by the distance of the ego's end point to the target lane, repeated lane points included: a zero-length FIRST
    segment makes the reference's distance NaN and keeps every mode; a zero-length interior segment is skipped.  The decisions are clear of
    the threshold in float64 (tests/test_aime_restate_host.py); the merge runs on the kernel's own signatures, clear of pi/6."""
    B = 2                                                                           # (the third scene has last < 0: no lane test possible)
    w = _run_world(hip_predictor, c, n_scenes=B, decide=True)
    for b in range(B):
        t = true_world(c, b)
        a0, a1 = c["a_off"][b], c["a_off"][b + 1]
        assert np.array_equal(np.isnan(w["ego_end"][b, :, 3]), np.isnan(t["end"][:, 3])), (name, b)
        sel, selp, margin = R.select(CLS, F32(1.0), w["topo"][a0 + 1:a1], t["end"].astype(F32), c["dist_thres"])
        assert margin >= 1e-3, (name, b, margin)
        print(f"{name} scene {b}: lane distances {np.round(t['end'][:, 3], 3)} kept {sel[sel >= 0]}")
        assert np.array_equal(w["sel"][0, b].astype(np.int64), sel) and np.array_equal(w["sel"][1, b], selp), (name, b, w["sel"][0, b], sel)
        # the leading mode ends 30 m off the lane: pruned by every finite distance, kept by the NaN of a zero-length first segment
        assert sel[0] == (2 if name == "lane_repeat_first" else 4), (name, b, sel)


# ------------------------------------------------------------------------------------------------------------------------------
FORMS = [(fused, by_value) for fused in (True, False) for by_value in (False, True)]


@pytest.mark.parametrize("name,c", DECIDE, ids=[n for n, _ in DECIDE])
def test_decisions_equal_the_restatement_in_all_four_launch_forms(hip_predictor, name, c):
    sel, selp, hit, _ = decide_truth(c)
    dev = hip_predictor.device
    up = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("cls", "topo", "ego_end", "world")}
    for fused, by_value in FORMS:
        g_sel, g_selp, g_hit = hip_predictor.aime_decide(c["a_off"], c["cmp"], up["cls"], c["scen_prob"], up["topo"], up["ego_end"], up["world"],
                                                         dist_thres=c["dist_thres"], prob_floor=c["prob_floor"], fused=fused, by_value=by_value)
        form = f"{name} fused={fused} by_value={by_value}"
        assert np.array_equal(g_sel, sel), (form, g_sel, sel)
        assert np.array_equal(g_selp, selp), form
        assert np.array_equal(g_hit, hit), (form, [(b, j, hex(int(g_hit[b, j, 0])), hex(int(hit[b, j, 0])), hex(int(g_hit[b, j, 1])), hex(int(hit[b, j, 1])))
                                                   for b, j in zip(*np.nonzero((g_hit != hit).any(-1)))])


@pytest.mark.parametrize("name,c", EC.decide_refused(0), ids=["nine_scenes", "ragged"])
def test_tables_by_value_are_refused_beyond_what_they_hold(hip_predictor, name, c):
    sel, selp, hit, _ = decide_truth(c)
    args = (c["a_off"], c["cmp"], c["cls"], c["scen_prob"], c["topo"], c["ego_end"], c["world"])
    for fused in (True, False):
        got = hip_predictor.aime_decide(*args, dist_thres=c["dist_thres"], fused=fused, by_value=False)
        assert np.array_equal(got[0], sel) and np.array_equal(got[1], selp) and np.array_equal(got[2], hit), (name, fused)
        with pytest.raises(MindError, match="by value"):
            hip_predictor.aime_decide(*args, dist_thres=c["dist_thres"], fused=fused, by_value=True)


# ------------------------------------------------------------------------------------------------------------------------------
def _run_rebase(hp, c):
    o = hp.aime_rebase(c["pos"], c["ang"], c["vel"], c["types"], c["lane_ctrs"], c["lane_vecs"], c["tlane"], c["tinfo"], pad=c["pad"],
                       time_ahead=c["time_ahead"], min_vel=c["min_vel"])
    return {k: v.cpu().numpy() for k, v in o.items() if isinstance(v, torch.Tensor)}


_REBASE_RUNS = {}


def _rebase_run(hp, name):
    if name not in _REBASE_RUNS:
        _REBASE_RUNS[name] = _run_rebase(hp, dict(REBASE)[name])
    return _REBASE_RUNS[name]


@pytest.mark.parametrize("name,c", REBASE, ids=[n for n, _ in REBASE])
def test_rebase_kernel_on_the_edge_families(hip_predictor, name, c):
    got = _rebase_run(hip_predictor, name)
    h = host_rebase(c)
    S, a = c["pos"].shape[:2]
    l = len(c["lane_ctrs"])
    actors = got["actors"].reshape(S, a, 14, 48)
    ego = lambda x: ulp32(max(np.abs(x).max(), 1.0))                                # every compared length lives in the ego's frame: the floor too
    for s_ in range(S):
        tab = Table(f"rebase_{name}[{s_}]")                                         # one bar per scene: a scene is not held to its family's worst
        t = true_rebase(c, s_, h)
        fr = got["frames"][s_]
        # bit-level facts: ORIG, the target window (same index as the restatement's decision) and its info rows, one-hot and pad rows
        assert np.array_equal(fr[4:6], c["pos"][s_, 0, -1])
        assert np.array_equal(fr[6:], c["tlane"][t["idx"] - 5:t["idx"] + 6].reshape(-1)), (name, s_, t["idx"], t["info"], fr[6:8])
        assert np.array_equal(got["tgt_nodes"][s_][:, 4:], c["tinfo"][t["idx"] - 4:t["idx"] + 6]), (name, s_)
        assert np.array_equal(actors[s_][:, 6:], t["actors"][:, 6:].astype(F32)), (name, s_)
        tab.add("rot", fr[:4], h["frames"][s_, :4], t["frames"][:4], ULP_PI)
        tab.add("actor_ctrs", got["actor_ctrs"].reshape(S, a, 2)[s_], h["actor_ctrs"][s_], t["actor_ctrs"], ego(t["actor_ctrs"]))
        tab.add("actor_vecs", got["actor_vecs"].reshape(S, a, 2)[s_], h["actor_vecs"][s_], t["actor_vecs"], ULP_PI)
        tab.add("actors_disp", actors[s_][:, 0:2], h["actors"][s_][:, 0:2], t["actors"][:, 0:2], ego(t["actors"][:, 0:2]))
        tab.add("actors_cos_sin", actors[s_][:, 2:4], h["actors"][s_][:, 2:4], t["actors"][:, 2:4], ULP_PI)
        tab.add("actors_vel", actors[s_][:, 4:6], h["actors"][s_][:, 4:6], t["actors"][:, 4:6], ego(t["actors"][:, 4:6]))
        if l:
            tab.add("lane_ctrs", got["lane_ctrs"].reshape(S, l, 2)[s_], h["lane_ctrs"][s_], t["lane_ctrs"], ego(t["lane_ctrs"]))
            tab.add("lane_vecs", got["lane_vecs"].reshape(S, l, 2)[s_], h["lane_vecs"][s_], t["lane_vecs"], ULP_PI)
        tab.add("tgt_nodes", got["tgt_nodes"][s_][:, :4], h["tgt_nodes"][s_][:, :4], t["tgt_nodes"][:, :4], ego(t["tgt_nodes"][:, :4]))
        tab.add("tgt_rpe", got["tgt_rpe"][s_], h["tgt_rpe"][s_], t["tgt_rpe"], ULP_PI)
        tab.check()


def test_target_window_ties_ends_and_the_two_lane_paths(hip_predictor):
    """the 256-thread argmin takes the FIRST minimum (a tie inside one thread's stride, a tie between neighbouring threads); the window
    index clamps at both ends of the lane; a lane of 1 024 points (staged in LDS) and the same lane with one more point (walked in global
    memory) give the same index and the same outputs"""
    by = dict(REBASE)
    runs = {P: _rebase_run(hip_predictor, f"lane_pos_P{P}") for P in (12, 1024, 1025, 2000)}
    for P in (1024, 1025, 2000):
        lane = by[f"lane_pos_P{P}"]["tlane"]
        first = [int(np.flatnonzero((lane == runs[P]["frames"][s_, 6:8]).all(1))[0]) for s_ in range(8)]
        assert [f + 5 for f in first] == [5, 6, 20, 20, 43, 375, P - 6, P - 6], (P, first)
    lane = by["lane_pos_P12"]["tlane"]
    assert [int(np.flatnonzero((lane == runs[12]["frames"][s_, 6:8]).all(1))[0]) + 5 for s_ in range(5)] == [5, 6, 6, 6, 6]
    for k in ("frames", "tgt_nodes", "tgt_rpe", "actor_ctrs", "actor_vecs"):
        assert np.array_equal(runs[1024][k][:6], runs[1025][k][:6]), k
    assert np.array_equal(runs[1024]["actors"][:6], runs[1025]["actors"][:6])
    info24, info25 = by["lane_pos_P1024"]["tinfo"], by["lane_pos_P1025"]["tinfo"]
    assert np.array_equal(info24, info25[:1024])                                    # (the same per-point info: the node rows may be compared)


# ------------------------------------------------------------------------------------------------------------------------------
def _moved(lcl, obs, theta, shift):
    """the same world after a rigid motion: rotated by theta about the origin, then shifted (float64, before anything is rounded)"""
    import copy
    from types import SimpleNamespace
    Rm = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    mv = lambda p: np.matmul(np.asarray(p, np.float64)[..., :2], Rm.T) + np.asarray(shift, np.float64)
    turn = lambda h: float(np.arctan2(np.sin(h + theta), np.cos(h + theta)))        # headings stay in (-pi, pi]: some land on either side of the cut
    obs2 = {}
    for tid, tr in obs.items():
        st = [type(s_)(s_.observed, s_.timestep, tuple(float(v) for v in mv(s_.position)), turn(s_.heading),
                       tuple(float(v) for v in np.matmul(np.asarray(s_.velocity, np.float64), Rm.T))) for s_ in tr.object_states]
        obs2[tid] = type(tr)(tr.track_id, st, tr.object_type, tr.category)
    m = copy.copy(lcl.map_data)
    m._centerlines = {k: np.concatenate([mv(v), v[:, 2:]], 1) for k, v in lcl.map_data._centerlines.items()}

    def agent(a):
        xy = mv(a.state[:2])
        return SimpleNamespace(state=np.array([xy[0], xy[1], a.state[2], turn(a.state[3])]), type=a.type, id=a.id, timestep=a.timestep)
    lcl2 = SimpleNamespace(ego_agent=agent(lcl.ego_agent), exo_agents=[agent(a) for a in lcl.exo_agents], map_data=m,
                           target_lane=mv(lcl.target_lane).astype(F32), target_lane_info=lcl.target_lane_info, target_velocity=lcl.target_velocity)
    return lcl2, obs2, Rm


def _root_layout(a, l, P):
    """offsets (floats) of the root scene on the device: RootLayout of mind_amd/csrc/aime_book.h, every array on a 4-float boundary"""
    o, off = {}, 0
    for name, n in (("actors", a * 14 * 48), ("ctrs", a * 2), ("vecs", a * 2), ("lanes", l * 160), ("lc", l * 2), ("lv", l * 2), ("tn", 160), ("tr", 20),
                    ("cov", a), ("types", a * 50 * 7), ("tl", P * 2), ("ti", P * 12), ("wpos", a * 100), ("wang", a * 50), ("wvel", a * 100), ("fr", 28)):
        o[name] = slice(off, off + n)
        off += (n + 3) & ~3
    return o


def test_device_built_root_far_from_the_origin_and_at_the_heading_cut(hip_predictor):
    """The root scene as the native plan builds it on the device (k_aime_rebase on the raw windows, k_aime_root_lanes, k_aime_root_hist), read
    back from the plan's root buffer, on a small synthetic world rigidly rotated by pi - 0.01 and shifted by (4 000, -3 000) m: every heading
    within 0.05 of the -pi cut, every coordinate 5 km out.  Truth: the float64 restatement of the featuriser on the same float32 windows and
    float64 lane pieces; e_ref: the float32 host featuriser (process_data / prepare_root_data) on the moved world; the same bar, with the
    floor at the magnitude of the compared quantity (ego-frame outputs: ego-frame metres; world-frame histories: world metres)."""
    from mind_amd.planners.mind import utils as U
    from mind_amd.planners.mind.configs.planning._base import ScenTreeCfg
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.planners.mind.scenario_tree import ScenarioTreeGenerator as STG
    from mind_amd.synth import SynthWorld
    from test_aime_restate_host import EPS
    w = SynthWorld(n_agents=6, n_lanes=3, n_segs=8, seed=1)
    lcl, obs, _ = _moved(w.local_semantic_map(4.9), w.tracks(4.9, drop={2: 30}), np.pi - 0.01, (4000.0, -3000.0))
    gen = STG(torch.device("cpu"), None, 50, 50, ScenTreeCfg())
    gen.reset()
    gen.set_target_lane(*MINDPlanner.resample_target_lane(MINDPlanner.__new__(MINDPlanner), lcl))
    cfg, tlane, tinfo = gen.config, gen.target_lane, gen.target_lane_info
    # float32 host featuriser
    root = gen.prepare_root_data(gen.process_data(lcl, obs))
    # the same raw inputs the planner hands to the native plan (scenario_tree.py: _native_args)
    pos, ang, vel, types, flags, tids, cats = U.get_agent_trajectories(obs)
    st = U._static_lane_pieces(lcl.map_data, 15.0, 10)
    travel0 = F32(max(lcl.ego_agent.state[2], 0.5) * cfg.tar_time_ahead)
    raw = dict(pos=pos, ang=ang, vel=vel, pad=flags, types=types, lane_pts=st["pts"], lane_flags=st["flags"], travel0=travel0)
    a, l, P = pos.shape[0], int(st["num_lanes"]), len(tlane)
    assert np.abs(np.abs(ang[:, -1]) - np.pi).max() < 0.05 and np.abs(pos).min(axis=(0, 1)).min() > 2900.0
    hip_predictor.aime_plan(None, None, None, None, tlane, tinfo, cfg.tar_time_ahead, cfg.tar_dist_thres, cfg.max_depth, pred_len=50, raw=raw)
    buf = hip_predictor.debug_read("pl_root")
    o = _root_layout(a, l, P)
    got = {k: buf[s_].copy() for k, s_ in o.items()}
    assert np.array_equal(got["tl"], tlane.reshape(-1)) and np.array_equal(got["types"], types.astype(F32).reshape(-1))   # the layout is the one read
    # float64 truth; the window index is a float32 decision, clear of its neighbours
    orig, theta = pos[0, -1], ang[0, -1]
    idx, info = R.window_index(tlane, orig, travel0)
    assert info["gap"] >= 100 * ulp32(4000.0) and info["slack"] >= 100 * info["steps"] * EPS * float(travel0), info
    t = R.rebase(pos, ang, vel, types, flags, np.zeros((0, 2)), np.zeros((0, 2)), tlane, tinfo, idx)
    lc, lv, lanes = R.root_lanes(st["pts"], st["flags"], orig, theta)
    wpos, wang, wvel = R.root_hist(t, orig, theta)
    # bit-level facts
    fr = got["fr"]
    assert np.array_equal(fr[4:6], orig) and np.array_equal(fr[6:], tlane[idx - 5:idx + 6].reshape(-1)), (idx, fr[6:8])
    actors, h_act = got["actors"].reshape(a, 14, 48), root["ACTORS"]
    assert np.array_equal(actors[:, 6:], t["actors"][:, 6:].astype(F32))
    g_lanes, g_tn = got["lanes"].reshape(l, 10, 16), got["tn"].reshape(10, 16)
    assert np.array_equal(g_lanes[..., 4:], lanes[..., 4:].astype(F32)) and np.array_equal(g_tn[:, 4:], tinfo[idx - 4:idx + 6])
    assert np.array_equal(got["cov"], np.full(a, 1e-5, F32))
    tab = Table("moved_root")
    ego = lambda x: ulp32(max(np.abs(x).max(), 1.0))
    tab.add("rot", fr[:4], root["ROT"].reshape(-1), t["frames"][:4], ULP_PI)
    tab.add("actor_ctrs", got["ctrs"].reshape(a, 2), root["TRAJS_CTRS"], t["actor_ctrs"], ego(t["actor_ctrs"]))
    tab.add("actor_vecs", got["vecs"].reshape(a, 2), root["TRAJS_VECS"], t["actor_vecs"], ULP_PI)
    tab.add("actors_disp", actors[:, 0:2], h_act[:, 0:2], t["actors"][:, 0:2], ego(t["actors"][:, 0:2]))
    tab.add("actors_cos_sin", actors[:, 2:4], h_act[:, 2:4], t["actors"][:, 2:4], ULP_PI)
    tab.add("actors_vel", actors[:, 4:6], h_act[:, 4:6], t["actors"][:, 4:6], ego(t["actors"][:, 4:6]))
    tab.add("lane_ctrs", got["lc"].reshape(l, 2), gen.lane_graph["lane_ctrs"], lc, ego(lc))
    tab.add("lane_vecs", got["lv"].reshape(l, 2), gen.lane_graph["lane_vecs"], lv, ULP_PI)
    tab.add("lanes", g_lanes[..., :4], root["LANES"][..., :4], lanes[..., :4], ego(lanes[..., :4]))
    tab.add("tgt_nodes", g_tn[:, :4], root["TGT_NODES"][:, :4], t["tgt_nodes"][:, :4], ego(t["tgt_nodes"][:, :4]))
    tab.add("tgt_rpe", got["tr"], root["TGT_RPE"], t["tgt_rpe"], ULP_PI)
    tab.add("hist_pos", got["wpos"].reshape(a, 50, 2), root["TRAJS_POS_HIST"], wpos, ego(wpos))
    tab.add("hist_heading", got["wang"].reshape(a, 50), root["TRAJS_ANG_HIST"], wang, ULP_PI)
    tab.add("hist_vel", got["wvel"].reshape(a, 50, 2), root["TRAJS_VEL_HIST"], wvel, ego(wvel))
    tab.check()
