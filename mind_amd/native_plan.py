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
"""
import ctypes as C
import os

import numpy as np

from . import _lib


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


class NativePlan:
    @staticmethod
    def why_not(pl, lcl_smp):
        """None when the native cycle applies to this planner and the scene it is shown, else the reason (a string): the planner-side
        conditions of NativeLoop.why_not -- nothing is asked of the world or the simulator"""
        from .planners.mind.planner import MINDPlanner
        if os.environ.get("MIND_NATIVE_PLAN", "1") == "0":
            return "MIND_NATIVE_PLAN=0"
        if type(pl) is not MINDPlanner:
            return "the planner is not a MINDPlanner"
        gen, opt, net = pl.scen_tree_gen, pl.traj_tree_opt, pl.network
        if gen.network is not net or type(net).__name__ != "ScenePredNet" or getattr(net, "rt", None) is None or not getattr(net, "_loaded", False):
            return "the generator's network is not the HIP predictor itself"
        if not (gen.native_aime and gen.device_glue and gen.device_select and gen.device_root) or gen.shard is not None or gen.ego_idx != 0 or gen.config is None:
            return "the native AIME plan with the device-built root is not selected"
        if gen.obs_len != 50 or pl.obs_len != 50 or not (2 <= gen.pred_len <= 60):
            return "horizons"
        if opt.solver is not None or opt.shard is not None or not opt.overlap or opt._runtime() is not net.rt:
            return "the contingency solves are not the plain case"
        if os.environ.get("MIND_PLAN_BEGINS_SOLVES", "1") == "0" or not getattr(pl, "_native_eval", True):
            return "plan-begun solves / native evaluation switched off"
        if pl.gt_tgt_lane is None:
            return "no target lane yet (update_target_lane)"
        return NativePlan._lane_reason(lcl_smp)

    @staticmethod
    def _lane_reason(lcl_smp):
        lane = np.asarray(lcl_smp.target_lane)
        if lane.dtype not in (np.float32, np.float64) or lane.ndim != 2 or lane.shape[1] != 2 or len(lane) < 2 or np.any(np.all(lane[1:] == lane[:-1], axis=1)):
            return "the target lane is not a float polyline without zero-length segments"
        if np.asarray(lcl_smp.ego_agent.state).dtype not in (np.float32, np.float64):
            return "agent states are neither float32 nor float64"
        return None

    def __init__(self, pl, lcl_smp):
        from .planners.mind.trajectory_tree import ilqr_cfg_from, _cfg_fingerprint
        from .planners.mind.utils import _TYPE_SLOT, _name
        self.pl, self.lib = pl, _lib.load()
        gen, opt = pl.scen_tree_gen, pl.traj_tree_opt
        self.rt = pl.network.rt
        self._slot = lambda t: _TYPE_SLOT.get(_name(t), 6)
        self._fp = _cfg_fingerprint
        keep = self._keep = {}
        keep["cw"], keep["cf"] = ilqr_cfg_from(opt.config, "w_opt_cfg"), ilqr_cfg_from(opt.config, "opt_cfg")
        # what is copied at creation and must stay as it is (checked before every call)
        self._gen_cfg, self._opt_cfg, self._net = gen.config, opt.config, pl.network
        self._scen_fp = (gen.config.tar_time_ahead, gen.config.tar_dist_thres, gen.config.max_depth, gen.pred_len)
        self._opt_fp = (_cfg_fingerprint(opt.config, "w_opt_cfg"), _cfg_fingerprint(opt.config, "opt_cfg"))
        self._ego_type = lcl_smp.ego_agent.type
        cfg = gen.config
        d = _lib.PlannerDesc()
        d.time_ahead, d.min_vel, d.dist_thres = float(cfg.tar_time_ahead), 0.5, float(cfg.tar_dist_thres)
        d.max_depth, d.max_rounds, d.pred_len, d.prob_floor = int(cfg.max_depth), 16, int(gen.pred_len), 0.0
        d.cfg_warm, d.cfg_full = C.addressof(keep["cw"]), C.addressof(keep["cf"])
        # the speculative warm start inside the library: opt-in as for the native loop (MIND_NATIVE_SPECULATE=1)
        self.speculative = bool(opt.speculative) and os.environ.get("MIND_NATIVE_SPECULATE", "0") == "1"
        d.speculative, d.ego_type_slot = int(self.speculative), self._slot(self._ego_type)
        h = C.c_void_p()
        rc = self.lib.mind_planner_create(self.rt.ctx, C.byref(d), C.byref(h))
        _lib.check(self.lib, self.rt.ctx, rc, "mind_planner_create")
        self.h = h
        self._ctx_value = self.rt.ctx.value
        self.out = _lib.PlannerOut()
        self._out_ref = C.byref(self.out)
        self._keys, self._ids, self._types = {}, [], []        # track id -> key (= index into _ids / _types)
        self._gen, self._result = 0, None
        # fingerprints of the scene tables in the library (None = not sent yet)
        self._st = self._tl = self._gt_bytes = self._tv = None
        cn, ts = opt.counters, pl.timing_sum
        self._base = dict(plans=ts["plans"], aime_s=ts["aime_s"], ilqr_s=ts["ilqr_s"], total_s=ts["total_s"], n_expanded=gen.n_expanded, solves=cn["solves"],
                          iterations=cn["iterations"], node_iterations=cn.get("node_iterations", 0), node_iterations_exo=cn.get("node_iterations_exo", 0),
                          warm_speculated=cn.get("warm_speculated", 0), warm_hits=cn.get("warm_hits", 0))

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h is not None:
            self.lib.mind_planner_destroy(h)          # (host memory only unless the speculation's side context exists)

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

    # ------------------------------------------------------------------------------------------
    def stale(self):
        """None while the planner is still the case this object was built for, else what changed (cheap: attribute reads, two small fingerprints)"""
        pl = self.pl
        gen, opt = pl.scen_tree_gen, pl.traj_tree_opt
        cfg = gen.config
        ctx = self.rt.ctx
        if self.h is None or ctx is None or ctx.value != self._ctx_value:
            return "the runtime was closed or re-created"
        if not (gen.native_aime and gen.device_root and gen.device_glue and gen.device_select) or gen.shard is not None:
            return "the native AIME plan with the device-built root is no longer selected"
        if gen.network is not self._net or pl.network is not self._net:
            return "the network was replaced"
        if opt.solver is not None or opt.shard is not None or not opt.overlap or (self.speculative and not opt.speculative) or not pl._native_eval:
            return "the contingency solves are no longer the plain case"
        if cfg is not self._gen_cfg or (cfg.tar_time_ahead, cfg.tar_dist_thres, cfg.max_depth, gen.pred_len) != self._scen_fp:
            return "the scenario tree configuration changed"
        if opt.config is not self._opt_cfg or (self._fp(self._opt_cfg, "w_opt_cfg"), self._fp(self._opt_cfg, "opt_cfg")) != self._opt_fp:
            return "the optimizer configuration changed"
        return None

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
            msg = self.lib.mind_last_error_string(self.rt.ctx) or b""
            if rc == _lib.MIND_ESTATE and msg.startswith(b"unsupported"):
                return msg.decode()
            _lib.check(self.lib, self.rt.ctx, rc, "mind_planner_plan")
        o = self.out
        gen, opt = pl.scen_tree_gen, pl.traj_tree_opt
        nt = o.n_trees
        pl.timing = {"aime_s": o.aime_s, "ilqr_s": o.ilqr_s, "total_s": o.total_s, "nodes_expanded": o.n_expanded, "n_scen_trees": nt,
                     "best_traj_idx": o.best, "tree_costs": o.costs[:nt]}
        t, b = o.tot, self._base
        ts, cn = pl.timing_sum, opt.counters
        ts["plans"], ts["aime_s"], ts["ilqr_s"], ts["total_s"] = b["plans"] + t.plans, b["aime_s"] + t.aime_s, b["ilqr_s"] + t.ilqr_s, b["total_s"] + t.total_s
        gen.n_expanded = b["n_expanded"] + t.expansions
        cn["solves"], cn["iterations"] = b["solves"] + 2 * t.scen_trees, b["iterations"] + t.iterations
        cn["node_iterations"], cn["node_iterations_exo"] = b["node_iterations"] + t.node_iterations, b["node_iterations_exo"] + t.node_iterations_exo
        cn["warm_speculated"], cn["warm_hits"] = b["warm_speculated"] + t.warm_speculated, b["warm_hits"] + t.warm_hits
        gen.n_native_plans += 1
        gen.branch_depth = o.n_rounds
        self._lazy = LazyPlanResult(self, self._gen)
        return True, np.array(o.ctrl), self._lazy

    def totals(self):
        """mind_loop_totals of this planner's cycles as a dict (kernel durations only while profiling is on)"""
        t = self.out.tot
        d = {k: getattr(t, k) for k, _ in _lib.LoopTotals._fields_ if k != "ilqr_prof"}
        d["ilqr_prof"] = list(t.ilqr_prof)
        return d

    # ------------------------------------------------------------------------------------------
    def last_result(self):
        """[[scenario tree], [trajectory tree]] of the last plan, built from the library's tables (as NativeLoop.last_result)"""
        if self._result is not None:
            return self._result
        if self.rt.ctx is None or self.rt.ctx.value != self._ctx_value:
            raise _lib.MindError("the runtime of this planner was closed: its last plan can no longer be read")
        from .planners.mind.trajectory_tree import to_traj_tree
        pl = self.pl
        gen, opt = pl.scen_tree_gen, pl.traj_tree_opt
        po = _lib.AimePlanOut()
        ptr = [C.c_void_p() for _ in range(6)]
        x0 = np.zeros(6)
        rc = self.lib.mind_planner_last_plan(self.h, C.byref(po), *[C.byref(p) for p in ptr], x0.ctypes.data)
        _lib.check(self.lib, self.rt.ctx, rc, "mind_planner_last_plan")
        a, nt = self.out.n_agents, po.n_trees
        res = self.rt._aime_plan_result(0, po, a, self._n_lanes)
        keys = np.frombuffer(C.string_at(ptr[4], a * 8), np.int64)
        types = np.frombuffer(C.string_at(ptr[5], a * 50 * 7 * 4), np.float32).reshape(a, 50, 7).astype(np.int16)
        root = {"TRAJS_TYPE": types, "TRAJS_TID": ["AV" if k == _lib.PLANNER_EGO_KEY else self._ids[k] for k in keys.tolist()],
                "TRAJS_CAT": ["av" if i == 0 else "exo" for i in range(a)]}
        scen = gen._native_trees(res, root, None, count=False)
        off = np.frombuffer(C.string_at(po.tree_off, (nt + 1) * 4), np.int32)
        M = int(off[-1])
        xs = np.frombuffer(C.string_at(ptr[0], M * 48), np.float64).reshape(M, 6)
        us = np.frombuffer(C.string_at(ptr[1], M * 16), np.float64).reshape(M, 2)
        stats = lambda p: [dict(iterations=s.iterations, converged=s.converged, J=s.J, mu=s.mu)
                           for s in C.cast(p, C.POINTER(_lib.IlqrStats * nt)).contents]
        opt.debug = dict(warm=stats(ptr[2]), full=stats(ptr[3]))
        trajs = [to_traj_tree(t._flat, x0, xs[off[i]:off[i + 1]], us[off[i]:off[i + 1]], opt.config.action_size) for i, t in enumerate(scen)]
        self._all = (scen, trajs)
        b = self.out.best
        self._result = [[scen[b]], [trajs[b]]]
        return self._result

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

    def rebase(self):
        """after a cycle the Python path computed between two native ones: the planner's running totals moved without the library's"""
        pl = self.pl
        gen, cn, ts, t = pl.scen_tree_gen, pl.traj_tree_opt.counters, pl.timing_sum, self.out.tot
        self._base = dict(plans=ts["plans"] - t.plans, aime_s=ts["aime_s"] - t.aime_s, ilqr_s=ts["ilqr_s"] - t.ilqr_s, total_s=ts["total_s"] - t.total_s,
                          n_expanded=gen.n_expanded - t.expansions, solves=cn["solves"] - 2 * t.scen_trees, iterations=cn["iterations"] - t.iterations,
                          node_iterations=cn.get("node_iterations", 0) - t.node_iterations, node_iterations_exo=cn.get("node_iterations_exo", 0) - t.node_iterations_exo,
                          warm_speculated=cn.get("warm_speculated", 0) - t.warm_speculated, warm_hits=cn.get("warm_hits", 0) - t.warm_hits)

    def export_windows(self):
        """planner.agent_obs as MINDPlanner.update_observation would hold it for the frames seen so far: Track objects with their array
        mirrors, exactly as NativeLoop.hand_back rebuilds them (the library keeps its own windows)"""
        from .planners.mind.planner import ObjectState, Track, TrackCategory
        pl = self.pl
        cap = len(self._ids) + 1
        n = C.c_int(0)
        key, count = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        rows = np.zeros((cap, 50, 7))
        rc = self.lib.mind_planner_export(self.h, cap, C.byref(n), key.ctypes.data, count.ctypes.data, rows.ctypes.data)
        _lib.check(self.lib, self.rt.ctx, rc, "mind_planner_export")
        dict.clear(pl.agent_obs)
        for s in range(n.value):
            k, cn = int(key[s]), int(count[s])
            ego = k == _lib.PLANNER_EGO_KEY
            tid = "AV" if ego else self._ids[k]
            tr = Track(tid, [ObjectState(bool(r[0]), int(r[6]), (r[1], r[2]), r[3], (r[4], r[5])) for r in rows[s, :cn]], self._ego_type if ego else self._types[k],
                       TrackCategory.FOCAL_TRACK if ego else TrackCategory.TRACK_FRAGMENT)
            try:
                buf = np.empty((4 * pl.obs_len, 6))
                buf[:cn] = rows[s, :cn, :6]
                tr._buf, tr._i, tr._n, tr._arr = buf, cn, cn, buf[0:cn]
            except AttributeError:
                pass
            pl.agent_obs[tid] = tr
