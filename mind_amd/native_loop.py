"""ClosedLoopSim's steps behind one native call (mind_loop_*, include/mind_hip.h; mind_amd/csrc/loop.hip).

The interpreter's share of a planning cycle on the recorded demo scene was 0.7 ms of 3.4 (simulator steps, observation windows, track
marshalling, the two C calls' argument building, result objects, candidate evaluation: profiles/r06j_host_time_demo_1.txt).  With a
`NativeLoop` the library keeps the simulator state and the observation windows itself and runs Simulator.run_sim's step (simulator.py:
51-107) -> MINDAgent.observe / plan (agent.py:317-331) -> MINDPlanner.plan (planner.py:66-145) -> kine_propagate without returning to
Python; the plan's scenario / trajectory trees become Python objects only when `ClosedLoopSim.last_result` is read.

What the library replays is tabulated HERE, once per scene, with the driver's own observation code (`ClosedLoopSim._exo_observation`,
`MINDPlanner.to_object_state`): the windows then hold the float64 values the Python steps would have put there, and every plan is the
same bits as the Python driver's (tests/test_gpu_native_loop.py).

A loop applies while the planner is the plain native case (HIP predictor, native AIME plan with the device-built root, plan-begun
contingency solves, native evaluation, no shard, no scripted modes, no injected solver).  The predicate is re-checked before every call;
when it stops holding -- a test flips `device_root`, a driver calls `step_begin` / `plan_start` itself -- the loop is handed back:
the windows are exported into `planner.agent_obs` and the simulator carries on with its Python steps from the same state.

What a `NativeLoop` shares with `NativePlan` (native_plan.py) -- the planner-side predicate, the staleness check, the cycle's descriptor
fields, the totals bookkeeping, the last plan's trees, the rebuild of `agent_obs` -- is `NativeCycle`, mind_amd/native_cycle.py.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .native_cycle import NativeCycle, lane_reason, planner_reason, rebuild_agent_obs, state_reason


_TRIG_CB = []


def _numpy_trig_callbacks():
    """(tan, sincos) C callbacks into numpy for the functions whose float64 results differ from the C library's on this host, None where they
    are the same routine (probed on 20 000 arguments; numpy 2.2 on an AVX-512 host: tan differs in 0.5 % of them, sin / cos in none)"""
    if not _TRIG_CB:
        import math
        rng = np.random.default_rng(0)
        x = rng.uniform(-0.8, 0.8, 20000)
        same_tan = all(float(a) == math.tan(float(b)) for a, b in zip(np.tan(x), x))
        y = rng.uniform(-7.0, 7.0, 20000)
        same_sc = all(float(a) == math.cos(float(b)) for a, b in zip(np.cos(y), y)) and all(float(a) == math.sin(float(b)) for a, b in zip(np.sin(y), y))
        f64, np_tan, np_sin, np_cos = np.float64, np.tan, np.sin, np.cos

        def tan_cb(v):
            return float(np_tan(f64(v)))

        def sincos_cb(v, out):
            v = f64(v)
            out[0], out[1] = float(np_sin(v)), float(np_cos(v))
        _TRIG_CB.append((None if same_tan else _lib.LOOP_TAN_FN(tan_cb), None if same_sc else _lib.LOOP_SINCOS_FN(sincos_cb)))
    return _TRIG_CB[0]


class NativeLoop(NativeCycle):
    _who = "mind_loop"
    pl = property(lambda self: self.sim.planner)

    @staticmethod
    def why_not(sim):
        """None when the native loop applies to this simulator + planner + world, else the reason (a string)"""
        w = sim.world
        if os.environ.get("MIND_NATIVE_LOOP", "1") == "0":
            return "MIND_NATIVE_LOOP=0"
        why = planner_reason(sim.planner)
        if why is not None:
            return why
        for name in ("agent_state", "object_type", "agent_ids", "n_agents", "target_lane", "target_lane_info", "target_velocity"):
            if not hasattr(w, name):
                return f"the world has no {name}"
        why = state_reason(w.agent_state(0, 0.0))
        if why is not None:
            return why
        if sim.episode_plans is None and not hasattr(w, "max_step"):
            return "an open-ended world without a last step"
        return lane_reason(w.target_lane)

    def __init__(self, sim):
        from types import SimpleNamespace
        from .planners.mind import utils as U
        self.sim = sim
        pl, w = sim.planner, sim.world
        gen = pl.scen_tree_gen
        self._cycle_init(pl)
        # ---- the scene's planner constants, built by the planner's own code
        lcl = SimpleNamespace(target_lane=w.target_lane, target_lane_info=w.target_lane_info, target_velocity=w.target_velocity)
        lane, info = pl.resample_target_lane(lcl)
        gen.set_target_lane(lane, info)
        if len(gen.target_lane) < 12:
            raise ValueError("target lane shorter than 12 points")
        st = U._static_lane_pieces(w, 15.0, 10)
        if st["num_lanes"] == 0:
            raise ValueError("no lanes")
        gen.n_lanes = int(st["num_lanes"])
        keep = self._keep
        f32 = lambda x: np.ascontiguousarray(x, np.float32)
        keep["tl"], keep["ti"] = f32(gen.target_lane), f32(gen.target_lane_info)
        keep["lpts"], keep["lfl"] = np.ascontiguousarray(st["pts"], np.float64), np.ascontiguousarray(st["flags"], np.int32)
        keep["gt"] = np.ascontiguousarray(np.asarray(pl.gt_tgt_lane, np.float64))
        ev = np.asarray(w.target_lane)
        keep["ev"] = np.ascontiguousarray(ev)
        # what must stay the same object for the loop to remain this planner's plan, beside NativeCycle's (ok(), before every call)
        self._gt_obj, self._world_fp = pl.gt_tgt_lane, (w.target_lane, w.target_lane_info, w.target_velocity)
        # ---- the replayed scene, one row per simulator step
        self._tabulate()
        d = _lib.LoopDesc()
        tb = self._tab
        n_steps, n_tracks = tb["ego"].shape[0], tb["valid"].shape[1]
        d.n_tracks, d.n_steps, d.clamp_last = n_tracks, n_steps, int(tb["clamp"])
        d.ego_state, d.exo_obs, d.exo_valid = tb["ego"].ctypes.data, tb["exo"].ctypes.data, tb["valid"].ctypes.data
        d.ego_state_is_f32, d.ego_obs, d.ego_trig32 = int(tb["f32"]), tb["ego_obs"].ctypes.data, tb["trig32"].ctypes.data
        # numpy's elementary functions where they are not the C library's (np.tan on AVX-512 hosts): the plant then calls back into numpy
        self._tan_cb, self._sincos_cb = _numpy_trig_callbacks()
        d.tan_fn = C.cast(self._tan_cb, C.c_void_p) if self._tan_cb is not None else None
        d.sincos_fn = C.cast(self._sincos_cb, C.c_void_p) if self._sincos_cb is not None else None
        d.timestep, d.type_slot = tb["ts"].ctypes.data, tb["slot"].ctypes.data
        d.sim_step, d.plan_step, d.enable_time = float(sim.SIM_STEP), float(sim.PLAN_STEP), float(sim.enable_time)
        d.wheelbase, d.max_speed, d.max_steer, d.max_acc, d.max_dec = float(sim.WB), float(sim.MAX_SPD), float(sim.MAX_STR), 6.0, -6.0
        d.n_lanes, d.lane_pts, d.lane_flags = int(st["num_lanes"]), keep["lpts"].ctypes.data, keep["lfl"].ctypes.data
        d.n_lane_pts, d.target_lane, d.target_lane_info = len(keep["tl"]), keep["tl"].ctypes.data, keep["ti"].ctypes.data
        self._fill_cycle_desc(d)
        d.solve_n_lane_pts, d.solve_lane, d.target_vel = len(keep["gt"]), keep["gt"].ctypes.data, float(w.target_velocity)
        d.eval_n_lane_pts, d.eval_lane_is_f32, d.eval_lane = len(keep["ev"]), int(keep["ev"].dtype == np.float32), keep["ev"].ctypes.data
        self._create(d, _lib.LoopOut())

    # ------------------------------------------------------------------------------------------
    def _tabulate(self):
        """ego_state / exo_obs / exo_valid / timestep per simulator step of an episode, from the simulator's own observation code.  Only the
        steps on which the planner is triggered read the exo rows: with a bounded episode the trigger steps are found by replaying the
        trigger arithmetic (the same float additions the library performs), the other rows stay empty."""
        sim = self.sim
        w, pl = sim.world, sim.planner
        n = int(w.n_agents)
        idx = {aid: i for i, aid in enumerate(w.agent_ids)}
        if len(idx) != n:
            raise ValueError("agent ids are not unique")
        if sim.episode_plans is not None:
            # replay check_enable / check_trigger (closed_loop.py step_begin) until the episode's last plan + one more cycle
            t, last, enabled, plans, trig = 0.0, None, False, 0, []
            k = 0
            while plans <= sim.episode_plans + 1 and k < 1000000:
                if t >= sim.enable_time:
                    enabled = True
                if last is None or (t - last) >= sim.PLAN_STEP:
                    last = t
                    trig.append(k)
                    plans += enabled
                t += sim.SIM_STEP
                k += 1
            n_tab, clamp, full = k, False, set(trig)
        else:
            n_tab, clamp, full = int(w.max_step) + 2, True, None
        ego = np.zeros((n_tab, 4))
        ego_obs = np.zeros((n_tab, 5))
        trig32 = np.zeros((n_tab, 2), np.float32)
        from types import SimpleNamespace
        exo = np.zeros((n_tab, n, 5))
        valid = np.zeros((n_tab, n), np.uint8)
        ts = np.zeros(n_tab, np.int32)
        t = 0.0
        for k in range(n_tab):
            es = w.agent_state(0, t)
            ego[k] = es
            ts[k] = int(round(t / 0.1))
            o = pl.to_object_state(SimpleNamespace(state=es, timestep=int(ts[k])))        # the recorded ego's window entry, by the driver's own code
            ego_obs[k] = (o.position[0], o.position[1], o.heading, o.velocity[0], o.velocity[1])
            if es.dtype == np.float32:
                trig32[k] = (np.cos(es[3]), np.sin(es[3]))          # numpy's float32 routines on the float32 yaw (kine_propagate's first step after the take-over)
            if full is None or k in full:
                for a in sim._exo_observation(t):
                    o = pl.to_object_state(a)
                    i = idx[a.id]
                    exo[k, i] = (o.position[0], o.position[1], o.heading, o.velocity[0], o.velocity[1])
                    valid[k, i] = 1
            t += sim.SIM_STEP
        from .planners.mind.utils import _TYPE_SLOT, _name
        slot = np.array([_TYPE_SLOT.get(_name(w.object_type(i)), 6) for i in range(n)], np.int32)
        self._tab = dict(ego=ego, ego_obs=ego_obs, trig32=trig32, exo=exo, valid=valid, ts=ts, slot=slot, clamp=clamp,
                         f32=w.agent_state(0, 0.0).dtype == np.float32)

    # ------------------------------------------------------------------------------------------
    def ok(self):
        """the planner is still the case this loop was built for (cheap: attribute reads and two small fingerprints)"""
        w = self.sim.world
        return (self.stale() is None and self.pl.gt_tgt_lane is self._gt_obj
                and w.target_lane is self._world_fp[0] and w.target_lane_info is self._world_fp[1] and w.target_velocity == self._world_fp[2])

    def advance(self, until_plans=0, until_time=-1.0, max_steps=1):
        """mind_loop_advance + the simulator's / planner's mirrors of what happened; returns the number of plans computed"""
        sim, o = self.sim, self.out
        p0, s0 = o.n_plans, o.n_steps
        rc = self.lib.mind_loop_advance(self.h, int(until_plans), float(until_time), int(max_steps), self._out_ref)
        if rc != 0:
            if self._unsupported(rc) is not None:
                return self._finish_step_on_the_host(p0, s0)
            _lib.check(self.lib, self.rt.ctx, rc, "mind_loop_advance")
        return self._mirror(p0, s0)

    def _mirror(self, p0, s0):
        sim, o = self.sim, self.out
        sim.sim_time, sim.enabled = o.sim_time, bool(o.enabled)
        sim.last_trigger = o.last_trigger if o.last_trigger >= 0.0 else None
        sim.state, sim.ctrl = np.array(o.state), np.array(o.ctrl)
        sim.n_steps += o.n_steps - s0
        dp = o.n_plans - p0
        if dp:
            sim.n_plans += dp
            self._result = None
            self._mirror_plan(dp)
        return dp

    # ------------------------------------------------------------------------------------------
    def last_result(self):
        """NativeCycle._last_result; None before the first plan"""
        if self._result is None and self.out.n_plans == 0:
            return None
        ids = self.sim.world.agent_ids
        return self._last_result(int(self._keep["lfl"].shape[0]), np.int32, lambda t: "AV" if t == 0 else ids[t])

    # ------------------------------------------------------------------------------------------
    def hand_back(self):
        """the simulator continues with its Python steps: the windows go into planner.agent_obs (Track objects with their array mirrors,
        as MINDPlanner.update_observation keeps them), the simulator's fields are the loop's; the loop is closed"""
        from .planners.mind.planner import TrackCategory
        sim = self.sim
        pl, w = sim.planner, sim.world
        self.lib.mind_loop_state(self.h, self._out_ref)
        o = self.out
        sim.sim_time, sim.enabled = o.sim_time, bool(o.enabled)
        sim.last_trigger = o.last_trigger if o.last_trigger >= 0.0 else None
        sim.state, sim.ctrl = np.array(o.state), np.array(o.ctrl)
        exported = self._exported_windows(self._tab["valid"].shape[1], np.int32)
        pl.agent_obs.clear()
        rebuild_agent_obs(pl, *exported, lambda ti: ("AV" if ti == 0 else w.agent_ids[ti], w.object_type(ti),
                                                     TrackCategory.FOCAL_TRACK if ti == 0 else TrackCategory.TRACK_FRAGMENT))
        if sim.enabled:
            pl.update_state_ctrl(sim.state, sim.ctrl)
        ctx = self.rt.ctx
        if self._result is None and o.n_plans and getattr(sim, "_last_result", None) is None and ctx is not None and ctx.value == self._ctx_value:
            try:
                self.last_result()
            except _lib.MindError:
                pass
        sim._last_result = self._result
        sim._native = None
        self.close()

    def _finish_step_on_the_host(self, p0, s0):
        """the library left this step's plan to the round-by-round path (mind_aime_plan 'unsupported: ...'): its observation update is
        done; the plan and the rest of the step run on the host, and so does everything after it"""
        sim = self.sim
        o = self.out
        sim.n_steps += o.n_steps - s0
        sim.n_plans += o.n_plans - p0
        self.hand_back()
        lcl = sim._observation()
        sim.planner.update_state_ctrl(lcl.ego_agent.state, sim.ctrl)
        sim.step_end(sim.planner.plan(lcl))
        return int(o.n_plans - p0) + 1
