"""MINDPlanner.update_observation / plan behind one native call each (mind_planner_*, mind_amd/native_plan.py; planner config / attribute
`native_plan`) against the planner's Python path, both driven by the Python steps of ClosedLoopSim(native=False): the same kernels on the
same windows, so every cycle must be bit-identical -- ego state and control, chosen tree, candidate costs, every array of the returned
scenario / trajectory trees, the running counters (the snapshot of tests/test_gpu_native_loop.py).  Reads the repository and
tests/golden/ only."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _snap():
    from test_gpu_native_loop import _same, _snapshot
    return _snapshot, _same


def _make(scene, native_plan, episode_plans=None, world=None, run=True):
    sys.path.insert(0, ROOT)
    from bench import BRANCHING_WEIGHTS, WORKLOADS
    from mind_amd.closed_loop import ClosedLoopSim
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.scene_io import ReplayWorld, scene_fixture_path
    cfg = os.path.join(ROOT, "mind_amd", "planners", "mind", "configs", "synthetic.json")
    wkw = dict(WORKLOADS[scene])
    w = ReplayWorld.from_scene_file(scene_fixture_path(wkw["scene"]))
    if world is not None:
        w = world(w)
    cfg = dict(json.load(open(cfg)), planning_config="planners.mind.configs.planning." + wkw["scene"], ckpt_path=BRANCHING_WEIGHTS)
    if native_plan:
        cfg["native_plan"] = True
    pl = MINDPlanner(cfg)
    pl.traj_tree_opt.speculative = False
    sim = ClosedLoopSim(w, pl, episode_plans=episode_plans, native=False)
    if world is not None:
        w.sim = sim
    if run:
        sim.run_until(sim.enable_time)
    return pl, sim


def _same_windows(pa, pb):
    assert list(pa.agent_obs) == list(pb.agent_obs)
    for k in pa.agent_obs:
        ta, tb = pa.agent_obs[k], pb.agent_obs[k]
        assert len(ta.object_states) == len(tb.object_states) and np.array_equal(ta._arr, tb._arr), k
        assert [tuple(s)[:2] for s in ta.object_states] == [tuple(s)[:2] for s in tb.object_states], k


@pytest.mark.parametrize("scene", ["demo_1", "demo_2", "demo_3", "demo_4"])
def test_native_plan_equals_the_python_path(scene):
    """14 planning cycles with episodes of 6 (two restarts: agent_obs.clear() reaches the library's windows), no cycle handed back"""
    _snapshot, _same = _snap()
    pa, sa = _make(scene, True, episode_plans=6)
    pb, sb = _make(scene, False, episode_plans=6)
    assert pa.native_plan and pa._native is not None, pa.native_plan_stats
    assert not pb.native_plan and pb._native is None and sa._native is None and sb._native is None
    assert len(pa.agent_obs) == 0 and len(pb.agent_obs) > 0          # the windows live in the library
    multi = 0
    for cycle in range(14):
        na = sa.run_plans(1)
        a = _snapshot(pa, sa)              # (the two planners share the thread's context: a plan's tables are read before the other one plans)
        nb = sb.run_plans(1)
        b = _snapshot(pb, sb)
        assert na == nb, (cycle, na, nb)
        _same(a, b, cycle)
        multi += len(a["costs"]) > 1
    assert pa.native_plan_stats["fallback"] == 0 and pa.native_plan_stats["native"] == 14, pa.native_plan_stats
    assert pb.native_plan_stats == {"native": 0, "fallback": 0, "reason": None}
    assert sa.n_episodes == sb.n_episodes == 2 and multi >= 4
    assert pa.scen_tree_gen.n_native_plans == pb.scen_tree_gen.n_native_plans
    # the plan's trees are built when they are read; once the planner has planned again they are gone
    from mind_amd._lib import MindError
    lcl = sa._observation()
    pa.update_state_ctrl(lcl.ego_agent.state, sa.ctrl)
    ok, ctrl, res = pa.plan(lcl)
    assert ok and len(res) == 2 and pa.native_plan_stats["native"] == 15
    pa.plan(lcl)
    with pytest.raises(MindError, match="planned again"):
        res[0]
    # ... and the windows come back as the Python path keeps them
    pa._native_hand_back("the test asks for the windows")
    assert pa._native is None and pa.native_plan_stats["reason"] == "the test asks for the windows"
    _same_windows(pa, pb)


class ReactiveWorld:
    """A world that cannot be tabulated ahead of time, around a recorded one: every exo agent within RADIUS of the ego's CURRENT plant state
    is slowed (the closer, the more), every reported state carries observation noise (seeded per agent and time step, so that it does not
    depend on how often a state is asked for), one track is first reported 0.3 s after the enable time and one disappears 0.6 s after it."""
    RADIUS, NOISE, SEED = 30.0, 0.02, 11

    def __init__(self, base):
        self.base, self.sim = base, None
        t0 = base.enable_time
        steady = [i for i in range(1, base.n_agents) if all(base.is_valid(i, t0 + 0.1 * k) for k in range(-10, 16))]
        assert len(steady) >= 2
        self.late, self.leaves = steady[0], steady[-1]

    def __getattr__(self, name):
        return getattr(self.base, name)

    def is_valid(self, i, t):
        if i == self.late and t < self.base.enable_time + 0.3 - 1e-9:
            return False
        if i == self.leaves and t > self.base.enable_time + 0.6 - 1e-9:
            return False
        return self.base.is_valid(i, t)

    def agent_state(self, i, t):
        s = np.array(self.base.agent_state(i, t))
        if i == 0:
            return s
        sim = self.sim
        ego = sim.state if (sim is not None and sim.enabled) else self.base.agent_state(0, t)
        d = float(np.hypot(float(s[0]) - float(ego[0]), float(s[1]) - float(ego[1])))
        if d < self.RADIUS:
            s[2] = s[2] * (0.5 + 0.5 * d / self.RADIUS)
        rng = np.random.default_rng([self.SEED, i, int(round(t * 1000))])
        s[:3] += (rng.normal(size=3) * self.NOISE).astype(s.dtype)
        return s


@pytest.mark.parametrize("scene", ["demo_1", "demo_3"])
def test_a_world_that_cannot_be_tabulated(scene, monkeypatch):
    """ReactiveWorld (exo states depend on the ego's plant state, noise, a late and a leaving track): mind_loop cannot run it -- there is no
    table of it -- native_plan engages and every cycle equals the Python path.  The driver's prefetch of the next observation presumes a
    replay (it would read the ego state five steps early), so it is off for both planners.
    Observed on an MI355X (RADIUS 30 m, NOISE 0.02, SEED 11): 0 fallback cycles of 14 on demo_1, 0 of 14 on demo_3."""
    monkeypatch.setenv("MIND_PREFETCH_OBS", "0")
    _snapshot, _same = _snap()
    pa, sa = _make(scene, True, episode_plans=8, world=ReactiveWorld)
    pb, sb = _make(scene, False, episode_plans=8, world=ReactiveWorld)
    assert pa._native is not None, pa.native_plan_stats
    wa = sa.world
    seen_late, slowed = [], 0
    for cycle in range(14):
        sa.run_plans(1)
        a = _snapshot(pa, sa)
        sb.run_plans(1)
        _same(a, _snapshot(pb, sb), cycle)
        seen_late.append(wa.is_valid(wa.late, sa.sim_time))
        slowed += any(np.hypot(*(np.asarray(wa.base.agent_state(i, sa.sim_time))[:2] - sa.state[:2])) < wa.RADIUS for i in range(1, wa.n_agents))
    st = pa.native_plan_stats
    print(f"{scene}: {st['native']} native cycles, {st['fallback']} fallback cycles ({st['reason']})")
    assert st["native"] + st["fallback"] == 14 and st["fallback"] <= 2, st
    assert slowed > 0 and not all(seen_late) and any(seen_late)       # the world really reacted, the late track really was late


def test_tables_that_change_between_two_cycles():
    """update_target_lane with another lane and a changed target velocity between two cycles (the world object is what ClosedLoopSim puts
    into lcl_smp): both planners follow, still bit-identical, and the change itself causes no fallback"""
    _snapshot, _same = _snap()
    pa, sa = _make("demo_2", True)
    pb, sb = _make("demo_2", False)
    for cycle in range(9):
        if cycle == 3:
            for pl, sim in ((pa, sa), (pb, sb)):
                gt = np.array(pl.gt_tgt_lane, np.float64)
                pl.update_target_lane(gt[:-2] + np.array([0.4, -0.3]))
                sim.world.target_velocity = float(sim.world.target_velocity) * 0.8 + 0.5
        if cycle == 6:           # the lane the scenario tree and the evaluation read: a NEW lane object, shifted sideways
            for pl, sim in ((pa, sa), (pb, sb)):
                w = sim.world
                w.target_lane = np.array(w.target_lane) + np.asarray([0.3, 0.2], np.asarray(w.target_lane).dtype)
        gt_before, tl_before = pa._native._gt_bytes, pa._native._tl
        sa.run_plans(1)
        a = _snapshot(pa, sa)
        sb.run_plans(1)
        _same(a, _snapshot(pb, sb), cycle)
        # a table goes to the library when it changed, only then
        assert (pa._native._gt_bytes != gt_before) == (cycle in (0, 3)) and (pa._native._tl is not tl_before) == (cycle in (0, 6)), cycle
    assert pa.native_plan_stats["fallback"] == 0 and pa.native_plan_stats["native"] == 9 and pa._native is not None


def test_hand_back_when_the_planner_changes_under_it():
    """five native cycles, then the host featuriser is selected (device_root = False): the windows move into planner.agent_obs and the
    Python path continues from them"""
    _snapshot, _same = _snap()
    pa, sa = _make("demo_2", True)
    pb, sb = _make("demo_2", False)
    for cycle in range(10):
        if cycle == 5:
            pa.scen_tree_gen.device_root = False
            pb.scen_tree_gen.device_root = False
        sa.run_plans(1)
        a = _snapshot(pa, sa)
        sb.run_plans(1)
        assert (pa._native is not None) == (cycle < 5)
        _same(a, _snapshot(pb, sb), cycle)
        if cycle == 5:
            _same_windows(pa, pb)
    assert "device-built root" in pa.native_plan_stats["reason"] and pa.native_plan_stats["native"] == 5
    _same_windows(pa, pb)


def test_a_driver_that_plans_in_halves_takes_the_windows_over():
    _snapshot, _same = _snap()
    pa, sa = _make("demo_3", True)
    pb, sb = _make("demo_3", False)
    sa.run_plans(2); sb.run_plans(2)
    assert pa._native is not None
    snaps = []
    for pl, sim in ((pa, sa), (pb, sb)):
        for _ in range(12):
            lcl = sim.step_begin()
            sim.step_end(pl.plan_end(pl.plan_begin(lcl)) if lcl is not None else None)
        snaps.append(_snapshot(pl, sim))
    assert pa._native is None and "plan_begin" in pa.native_plan_stats["reason"]
    _same(snaps[0], snaps[1], "halves")
    _same_windows(pa, pb)


def test_same_device_work_as_the_native_loop():
    """a mind_loop cycle and a mind_planner cycle of the same scene and step: the same tree-iLQR launch (cost trees, workgroups per tree),
    the same rounds, expansions and pair-kernel launches"""
    sys.path.insert(0, ROOT)
    from test_gpu_native_loop import _make as _make_loop
    pa, sa = _make("demo_4", True)
    pl_, sl = _make_loop("demo_4", None)
    assert pa._native is not None and sl._native is not None
    rt = pa.network.rt
    assert pl_.network.rt is rt
    rt.set_profiling(True)
    try:
        prev = (0, 0)
        for cycle in range(6):
            sa.run_plans(1)
            ia = rt.ilqr_stats()[1:]
            oa = pa._native.out
            ta = pa._native.totals()
            a = (tuple(ia), oa.n_rounds, oa.n_expanded, oa.n_trees, oa.n_traj_nodes, ta["pair_launches"], ta["ilqr_launches"])
            sl.run_plans(1)
            ib = rt.ilqr_stats()[1:]
            ob = sl._native.out
            tb = sl._native.totals()
            b = (tuple(ib), ob.n_rounds, ob.n_expanded, ob.n_trees, ob.n_traj_nodes, tb["pair_launches"], tb["ilqr_launches"])
            assert a == b, (cycle, a, b)
            assert a[5] > prev[0] and a[6] == prev[1] + 1
            prev = (a[5], a[6])
    finally:
        rt.set_profiling(False)


def test_native_plan_errors_are_codes_and_messages():
    """plan before any observation, plan before the lanes are set, a target lane shorter than 12 points: negative codes and a message, never a
    crash; the planner object plans afterwards as if nothing had happened"""
    from mind_amd import _lib
    _snapshot, _same = _snap()
    pa, sa = _make("demo_1", True)
    pb, sb = _make("demo_1", False)
    nl = pa._native
    assert nl is not None
    lib, ctx = nl.lib, nl.rt.ctx
    out = _lib.PlannerOut()
    st, ct = np.array(sa.world.agent_state(0, 0.0), np.float64), np.zeros(2)
    # a planner that has seen no frame
    d = _lib.PlannerDesc()
    d.time_ahead, d.min_vel, d.dist_thres, d.max_depth, d.max_rounds, d.pred_len = 3.0, 0.5, 2.0, 5, 16, 60
    d.cfg_warm, d.cfg_full = C.addressof(nl._keep["cw"]), C.addressof(nl._keep["cf"])
    h = C.c_void_p()
    assert lib.mind_planner_create(ctx, C.byref(d), C.byref(h)) == 0
    try:
        assert lib.mind_planner_plan(h, st.ctypes.data, ct.ctypes.data, C.byref(out)) == _lib.MIND_ESTATE
        assert b"no observation" in lib.mind_last_error_string(ctx) and out.n_trees == 0
        po, ptr = _lib.AimePlanOut(), [C.c_void_p() for _ in range(6)]
        assert lib.mind_planner_last_plan(h, C.byref(po), *[C.byref(p) for p in ptr], None) == _lib.MIND_ESTATE
        assert b"no plan" in lib.mind_last_error_string(ctx)
    finally:
        lib.mind_planner_destroy(h)
    d.max_rounds = 0
    assert lib.mind_planner_create(ctx, C.byref(d), C.byref(h)) == _lib.MIND_EINVAL and b"bad argument" in lib.mind_last_error_string(ctx)
    # the planner's own object: 40 frames in its windows, no table sent yet (they go with the first plan)
    assert lib.mind_planner_plan(nl.h, st.ctypes.data, ct.ctypes.data, C.byref(out)) == _lib.MIND_ESTATE
    assert b"lane tables are not set" in lib.mind_last_error_string(ctx)
    short, info = np.zeros((11, 2), np.float32), np.zeros((11, 12), np.float32)
    short[:, 0] = np.arange(11)
    assert lib.mind_planner_set_target_lane(nl.h, 11, short.ctypes.data, info.ctypes.data) == _lib.MIND_EINVAL
    assert b"12" in lib.mind_last_error_string(ctx)
    assert lib.mind_planner_set_lanes(nl.h, 0, None, None) == _lib.MIND_EINVAL
    assert lib.mind_planner_set_solve_lane(nl.h, 1, short.ctypes.data, 5.0) == _lib.MIND_EINVAL
    assert lib.mind_planner_set_eval_lane(nl.h, 5, None, 1) == _lib.MIND_EINVAL
    # a sharded context plans through its exchange: the planner refuses it
    for cycle in range(3):
        if cycle == 1:
            cb = _lib.EXCHANGE_FN(lambda user, op, send, recv, nbytes: 0)
            assert lib.mind_set_exchange(ctx, 0, 2, cb, None, 0) == 0
            try:
                assert lib.mind_planner_plan(nl.h, st.ctypes.data, ct.ctypes.data, C.byref(out)) == _lib.MIND_ESTATE
                assert b"sharded" in lib.mind_last_error_string(ctx)
            finally:
                assert lib.mind_set_exchange(ctx, 0, 1, C.cast(None, _lib.EXCHANGE_FN), None, 0) == 0
        sa.run_plans(1)
        a = _snapshot(pa, sa)
        sb.run_plans(1)
        _same(a, _snapshot(pb, sb), cycle)
    assert pa._native is nl and pa.native_plan_stats["fallback"] == 0
