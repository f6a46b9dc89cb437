"""MINDPlanner.update_observation / plan behind one native call each (mind_planner_*, include/mind_hip.h; mind_amd/csrc/loop.hip).

`NativeLoop` (mind_amd/native_loop.py) owns the simulator and replays a scene that was tabulated ahead of time.  A `NativePlan` owns only
what the planner owns -- the 50-frame observation windows and the last plan -- and is fed one frame at a time through the planner's
own call surface (the reference's agent.py:317-331 calls update_observation, update_state_ctrl and plan): noisy observations, agents that
react to the ego, a target lane that changes during the run all reach it, because nothing is tabulated.  The cycle it runs is the native
loop's (one body in the library: cycle_plan), so every plan is the same bits as the Python path's (tests/test_gpu_native_plan.py).

Opt-in: planner config "native_plan": true, `planner.native_plan = True`, or `mind_amd.dropin.install(native_plan=True)`.

Everything copied into the library is fingerprinted and re-checked before every call: the scene tables (lanes, target lane, solve lane,
target velocity) are sent again when they change, a changed planner configuration hands the windows back to `planner.agent_obs` and the
Python path carries on from the same state (`planner.native_plan_stats` counts native and fallback cycles and keeps the last reason).

What a `NativePlan` shares with `NativeLoop` is `NativeCycle`, mind_amd/native_cycle.py (as `struct mind_cycle` in the library).
"""
import os

import numpy as np

from . import _lib
from .native_cycle import NativeCycle, lane_reason, planner_reason, rebuild_agent_obs, state_reason


class LazyPlanResult:
    """MINDPlanner.plan's third return value, [[scenario tree], [trajectory tree]], built from the library's tables when it is first read.
    The tables are the context's: read it before the next plan on that context (a recorder does, every step); afterwards it raises MindError."""
    __slots__ = ("_np", "_gen", "_val")

    def __init__(self, native_plan, gen):
        self._np, self._gen, self._val = native_plan, gen, None

    def _get(self):
        if self._val is None:
            nl = self._np
            if nl is None or nl._gen != self._gen:
                raise _lib.MindError("the planner has planned again since: this plan's tables are gone (read a native plan's trees before the next plan)")
            self._val = nl.last_result()
            self._np = None
        return self._val

    def __iter__(self):
        return iter(self._get())

    def __getitem__(self, i):
        return self._get()[i]

    def __len__(self):
        return 2


class NativePlan(NativeCycle):
    _who = "mind_planner"

    @staticmethod
    def why_not(pl, lcl_smp):
        """None when the native cycle applies to this planner and the scene it is shown, else the reason (a string): the planner-side
        conditions of NativeLoop.why_not -- nothing is asked of the world or the simulator"""
        if os.environ.get("MIND_NATIVE_PLAN", "1") == "0":
            return "MIND_NATIVE_PLAN=0"
        why = planner_reason(pl)
        if why is not None:
            return why
        if pl.gt_tgt_lane is None:
            return "no target lane yet (update_target_lane)"
        return NativePlan._lane_reason(lcl_smp)

    @staticmethod
    def _lane_reason(lcl_smp):
        return lane_reason(lcl_smp.target_lane, 2) or state_reason(lcl_smp.ego_agent.state)

    def __init__(self, pl, lcl_smp):
        from .planners.mind.utils import _TYPE_SLOT, _name
        self.pl = pl
        self._cycle_init(pl)
        self._slot = lambda t: _TYPE_SLOT.get(_name(t), 6)
        self._ego_type = lcl_smp.ego_agent.type
        d = _lib.PlannerDesc()
        self._fill_cycle_desc(d)
        d.ego_type_slot = self._slot(self._ego_type)
        self._keys, self._ids, self._types = {}, [], []        # track id -> key (= index into _ids / _types)
        self._gen = 0
        # fingerprints of the scene tables in the library (None = not sent yet)
        self._st = self._tl = self._gt_bytes = self._tv = None
        self._create(d, _lib.PlannerOut())

    # ------------------------------------------------------------------------------------------
    def ok(self):
        return self.stale() is None

    def reset(self):
        """ClosedLoopSim._start_episode (planner.agent_obs.clear()): windows cleared, last plan forgotten"""
        self.lib.mind_planner_reset(self.h)
        self._gen += 1
        self._result = None

    # ------------------------------------------------------------------------------------------
    def observe(self, lcl_smp):
        """MINDPlanner.update_observation for one frame: one mind_planner_observe call"""
        pl = self.pl
        to_state = pl.to_object_state
        ego = lcl_smp.ego_agent
        o = to_state(ego)
        ego_row = np.array((o.position[0], o.position[1], o.heading, o.velocity[0], o.velocity[1]), np.float64)
        keys, rows, slots = [], [], []
        key_of = self._keys
        for a in lcl_smp.exo_agents:
            k = key_of.get(a.id)
            if k is None:
                k = key_of[a.id] = len(self._ids)
                self._ids.append(a.id)
                self._types.append(a.type)
            o = getattr(a, "obj_state", None) or to_state(a)
            keys.append(k)
            slots.append(self._slot(self._types[k]))
            rows.append((o.position[0], o.position[1], o.heading, o.velocity[0], o.velocity[1]))
        n = len(keys)
        ka, sa, ra = np.array(keys, np.int64), np.array(slots, np.int32), np.array(rows, np.float64).reshape(n, 5)
        rc = self.lib.mind_planner_observe(self.h, int(ego.timestep), ego_row.ctypes.data, n, ka.ctypes.data, sa.ctypes.data, ra.ctypes.data)
        _lib.check(self.lib, self.rt.ctx, rc, "mind_planner_observe")

    def sync_tables(self, lcl_smp):
        """the scene tables of this cycle, sent to the library where they differ from what it holds; returns None, or the reason why this
        scene is not one the native cycle takes"""
        from .planners.mind import utils as U
        pl, lib, h = self.pl, self.lib, self.h
        gen = pl.scen_tree_gen
        st = U._static_lane_pieces(lcl_smp.map_data, 15.0, 10)
        if st is not self._st:
            if st["num_lanes"] == 0:
                return "no lanes"
            pts, fl = np.ascontiguousarray(st["pts"], np.float64), np.ascontiguousarray(st["flags"], np.int32)
            _lib.check(lib, self.rt.ctx, lib.mind_planner_set_lanes(h, int(st["num_lanes"]), pts.ctypes.data, fl.ctypes.data), "mind_planner_set_lanes")
            self._st, self._n_lanes = st, int(st["num_lanes"])
        gen.n_lanes = self._n_lanes
        # (resample_target_lane keeps its result while the lane and its info are the same content: a new object = a changed lane)
        lane, info = pl.resample_target_lane(lcl_smp)
        if lane is not self._tl:
            why = self._lane_reason(lcl_smp)
            if why is not None:
                return why
            gen.set_target_lane(lane, info)
            if len(gen.target_lane) < 12:
                return "target lane shorter than 12 points"
            tl, ti = np.ascontiguousarray(gen.target_lane, np.float32), np.ascontiguousarray(gen.target_lane_info, np.float32)
            _lib.check(lib, self.rt.ctx, lib.mind_planner_set_target_lane(h, len(tl), tl.ctypes.data, ti.ctypes.data), "mind_planner_set_target_lane")
            ev = np.ascontiguousarray(np.asarray(lcl_smp.target_lane))
            _lib.check(lib, self.rt.ctx, lib.mind_planner_set_eval_lane(h, len(ev), ev.ctypes.data, int(ev.dtype == np.float32)), "mind_planner_set_eval_lane")
            self._tl = lane
        gt = np.ascontiguousarray(np.asarray(pl.gt_tgt_lane, np.float64))
        gb, tv = gt.tobytes(), float(lcl_smp.target_velocity)
        if gb != self._gt_bytes or tv != self._tv:
            if gt.ndim != 2 or gt.shape[1] != 2 or len(gt) < 2:
                return "gt_tgt_lane is not a polyline"
            _lib.check(lib, self.rt.ctx, lib.mind_planner_set_solve_lane(h, len(gt), gt.ctypes.data, tv), "mind_planner_set_solve_lane")
            self._gt_bytes, self._tv = gb, tv
        return None

    def plan(self, lcl_smp):
        """one mind_planner_plan call; returns MINDPlanner.plan's result, or the reason (a string) why this cycle is the Python path's"""
        pl = self.pl
        if pl.state is None or pl.ctrl is None:
            return "no ego state (update_state_ctrl)"
        state, ctrl = np.ascontiguousarray(pl.state, np.float64), np.ascontiguousarray(pl.ctrl, np.float64)
        if state.shape != (4,) or ctrl.shape != (2,) or float(lcl_smp.ego_agent.state[2]) != float(state[2]):
            return "the planner's state is not the observed ego's"
        why = self.sync_tables(lcl_smp)
        if why is not None:
            return why
        self._gen += 1
        self._result = None
        rc = self.lib.mind_planner_plan(self.h, state.ctypes.data, ctrl.ctypes.data, self._out_ref)
        if rc != 0:
            why = self._unsupported(rc)
            if why is not None:
                return why
            _lib.check(self.lib, self.rt.ctx, rc, "mind_planner_plan")
        self._mirror_plan(1)
        self._lazy = LazyPlanResult(self, self._gen)
        return True, np.array(self.out.ctrl), self._lazy

    def _track_id(self, key):
        return "AV" if key == _lib.PLANNER_EGO_KEY else self._ids[key]

    def last_result(self):
        """[[scenario tree], [trajectory tree]] of the last plan, built from the library's tables (NativeCycle._last_result)"""
        return self._last_result(self._n_lanes, np.int64, self._track_id)

    # ------------------------------------------------------------------------------------------
    def hand_back(self, reason):
        """the planner continues on its Python path: the windows go into planner.agent_obs; this object is closed"""
        pl = self.pl
        lazy = getattr(self, "_lazy", None)
        if lazy is not None and lazy._val is None and lazy._gen == self._gen:       # a plan somebody may still hold unread: its tables are still there
            try:
                lazy._get()
            except _lib.MindError:
                pass
        self.export_windows()
        pl._native = None
        pl.native_plan_stats["reason"] = reason
        self.close()

    def export_windows(self):
        """planner.agent_obs as MINDPlanner.update_observation would hold it for the frames seen so far (the library keeps its own windows)"""
        from .planners.mind.planner import TrackCategory
        exported = self._exported_windows(len(self._ids) + 1, np.int64)
        dict.clear(self.pl.agent_obs)          # (not agent_obs.clear(): that resets the library's windows)
        ego = _lib.PLANNER_EGO_KEY
        rebuild_agent_obs(self.pl, *exported, lambda k: ("AV", self._ego_type, TrackCategory.FOCAL_TRACK) if k == ego else
                          (self._ids[k], self._types[k], TrackCategory.TRACK_FRAGMENT))
