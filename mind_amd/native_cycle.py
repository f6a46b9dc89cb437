"""What the Python owner of a native planning cycle needs, whoever feeds the windows: the counterpart of `struct mind_cycle` in
mind_amd/csrc/loop.hip.  `NativeLoop` (native_loop.py: the library keeps the simulator too) and `NativePlan` (native_plan.py: the caller
pushes one frame at a time) derive from `NativeCycle`; where the two differ, the difference is a class attribute, an argument or stays
in the subclass.  A subclass provides `self.pl` (the MINDPlanner) and `_who`, the prefix of its entry points in the library."""
import ctypes as C
import os

import numpy as np

from . import _lib


def _ts(pl):
    return pl.timing_sum


def _cn(pl):
    return pl.traj_tree_opt.counters


def _gen(pl):
    return vars(pl.scen_tree_gen)


# the planner's running totals that the library keeps while it plans: (where the counter lives, its name, mind_loop_totals field, factor)
_TOTALS = ((_ts, "plans", "plans", 1), (_ts, "aime_s", "aime_s", 1), (_ts, "ilqr_s", "ilqr_s", 1), (_ts, "total_s", "total_s", 1),
           (_gen, "n_expanded", "expansions", 1), (_cn, "solves", "scen_trees", 2), (_cn, "iterations", "iterations", 1),
           (_cn, "node_iterations", "node_iterations", 1), (_cn, "node_iterations_exo", "node_iterations_exo", 1),
           (_cn, "warm_speculated", "warm_speculated", 1), (_cn, "warm_hits", "warm_hits", 1))


def planner_reason(pl):
    """None when the planner is the plain native case (HIP predictor, native AIME plan with the device-built root, plan-begun contingency
    solves, native evaluation, no shard, no injected solver), else the reason (a string)"""
    from .planners.mind.planner import MINDPlanner
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
    return None


def lane_reason(lane, min_points=0):
    lane = np.asarray(lane)
    if lane.dtype not in (np.float32, np.float64) or lane.ndim != 2 or lane.shape[1] != 2 or len(lane) < min_points or np.any(np.all(lane[1:] == lane[:-1], axis=1)):
        return "the target lane is not a float polyline without zero-length segments"
    return None


def state_reason(state):
    if np.asarray(state).dtype not in (np.float32, np.float64):
        return "agent states are neither float32 nor float64"
    return None


def rebuild_agent_obs(pl, n, ident, count, rows, describe):
    """the first `n` exported windows (`*_export`: identifier, row count, rows [50, 7] per track) into `pl.agent_obs`, in the library's
    track order, as MINDPlanner.update_observation would hold them; describe(identifier) -> (track id, object type, category)"""
    from .planners.mind.planner import track_from_rows
    for s in range(n):
        tid, otype, cat = describe(int(ident[s]))
        pl.agent_obs[tid] = track_from_rows(tid, rows[s, :int(count[s])], otype, cat, pl.obs_len)


class NativeCycle:
    def _cycle_init(self, pl):
        """what is copied into the library at creation and must stay as it is (stale(), before every call)"""
        from .planners.mind.trajectory_tree import ilqr_cfg_from, _cfg_fingerprint
        self.lib, self.rt = _lib.load(), pl.network.rt
        gen, opt = pl.scen_tree_gen, pl.traj_tree_opt
        self._keep = {"cw": ilqr_cfg_from(opt.config, "w_opt_cfg"), "cf": ilqr_cfg_from(opt.config, "opt_cfg")}
        self._gen_cfg, self._opt_cfg, self._net, self._fp = gen.config, opt.config, pl.network, _cfg_fingerprint
        self._scen_fp = (gen.config.tar_time_ahead, gen.config.tar_dist_thres, gen.config.max_depth, gen.pred_len)
        self._opt_fp = (_cfg_fingerprint(opt.config, "w_opt_cfg"), _cfg_fingerprint(opt.config, "opt_cfg"))

    def _fill_cycle_desc(self, d):
        """the cycle's fields of mind_loop_desc / mind_planner_desc"""
        cfg, keep = self._gen_cfg, self._keep
        d.time_ahead, d.min_vel, d.dist_thres = float(cfg.tar_time_ahead), 0.5, float(cfg.tar_dist_thres)
        d.max_depth, d.max_rounds, d.pred_len, d.prob_floor = int(cfg.max_depth), 16, int(self.pl.scen_tree_gen.pred_len), 0.0
        d.cfg_warm, d.cfg_full = C.addressof(keep["cw"]), C.addressof(keep["cf"])
        # the optimizer's speculative warm start inside the library (a second context of the object's own): opt-in, MIND_NATIVE_SPECULATE=1 --
        # a lone loop gains nothing from it (profiles/r06q_*), several loops sharing the device do
        self.speculative = bool(self.pl.traj_tree_opt.speculative) and os.environ.get("MIND_NATIVE_SPECULATE", "0") == "1"
        d.speculative = int(self.speculative)

    def _create(self, d, out):
        h = C.c_void_p()
        self._check(getattr(self.lib, self._who + "_create")(self.rt.ctx, C.byref(d), C.byref(h)), "create")
        self.h, self._ctx_value = h, self.rt.ctx.value
        self.out, self._out_ref = out, C.byref(out)
        self._result = None            # the last plan's [[scenario tree], [trajectory tree]] once somebody asked for it
        self.rebase()

    def _check(self, rc, what):
        _lib.check(self.lib, self.rt.ctx, rc, f"{self._who}_{what}")

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h is not None:
            getattr(self.lib, self._who + "_destroy")(h)      # (host memory, and the speculation's side context where one exists)

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
        ctx = self.rt.ctx         # (a runtime that was closed, or re-created, under this object: the library's holds the old context)
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

    def _unsupported(self, rc):
        """the library's message when it leaves this cycle to the Python path (mind_aime_plan 'unsupported: ...'), else None"""
        msg = self.lib.mind_last_error_string(self.rt.ctx) or b""
        return msg.decode() if rc == _lib.MIND_ESTATE and msg.startswith(b"unsupported") else None

    # ------------------------------------------------------------------------------------------
    def rebase(self):
        """base values of the planner's running totals = what they are now less the library's sums: at creation, and after a cycle the
        Python path computed between two native ones (the planner's totals moved without the library's)"""
        pl, t = self.pl, self.out.tot
        self._base = [where(pl).get(key, 0) - k * getattr(t, field) for where, key, field, k in _TOTALS]

    def _mirror_plan(self, dp):
        """the planner's and the generator's record of the last of `dp` plans the library just computed"""
        pl, o = self.pl, self.out
        gen = pl.scen_tree_gen
        nt = o.n_trees
        pl.timing = {"aime_s": o.aime_s, "ilqr_s": o.ilqr_s, "total_s": o.total_s, "nodes_expanded": o.n_expanded, "n_scen_trees": nt,
                     "best_traj_idx": o.best, "tree_costs": o.costs[:nt]}
        # the running totals are the library's (several plans may have run in one call): base values + its sums
        t = o.tot
        for (where, key, field, k), b in zip(_TOTALS, self._base):
            where(pl)[key] = b + k * getattr(t, field)
        gen.n_native_plans += dp
        gen.branch_depth = o.n_rounds

    def totals(self):
        """mind_loop_totals as a dict (running sums over this object's plans; kernel durations only while profiling is on)"""
        t = self.out.tot
        d = {k: getattr(t, k) for k, _ in _lib.LoopTotals._fields_ if k != "ilqr_prof"}
        d["ilqr_prof"] = list(t.ilqr_prof)
        return d

    # ------------------------------------------------------------------------------------------
    def _last_result(self, n_lanes, id_dtype, track_id):
        """[[scenario tree], [trajectory tree]] of the last plan (MINDPlanner.plan's third return value), built from the library's tables (raises
        MindError when another planner has planned on the shared context since: read the result before that, as a recorder does every step).
        id_dtype: what `*_last_plan` names the plan's agents with, track_id(identifier) -> the track id"""
        if self._result is not None:
            return self._result
        if self.rt.ctx is None or self.rt.ctx.value != self._ctx_value:
            raise _lib.MindError(f"the runtime of this {self._who[5:]} was closed: its last plan can no longer be read")
        from .planners.mind.trajectory_tree import to_traj_tree
        gen, opt = self.pl.scen_tree_gen, self.pl.traj_tree_opt
        po = _lib.AimePlanOut()
        ptr = [C.c_void_p() for _ in range(6)]
        x0 = np.zeros(6)
        self._check(getattr(self.lib, self._who + "_last_plan")(self.h, C.byref(po), *[C.byref(p) for p in ptr], x0.ctypes.data), "last_plan")
        a, nt = self.out.n_agents, po.n_trees
        res = self.rt._aime_plan_result(0, po, a, n_lanes)
        idents = np.frombuffer(C.string_at(ptr[4], a * np.dtype(id_dtype).itemsize), id_dtype)
        types = np.frombuffer(C.string_at(ptr[5], a * 50 * 7 * 4), np.float32).reshape(a, 50, 7).astype(np.int16)
        root = {"TRAJS_TYPE": types, "TRAJS_TID": [track_id(i) for i in idents.tolist()], "TRAJS_CAT": ["av" if i == 0 else "exo" for i in range(a)]}
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

    def _exported_windows(self, cap, id_dtype):
        """(n, identifier[cap], count[cap], rows[cap, 50, 7]) of `*_export`"""
        n = C.c_int(0)
        ident, count, rows = np.zeros(cap, id_dtype), np.zeros(cap, np.int32), np.zeros((cap, 50, 7))
        self._check(getattr(self.lib, self._who + "_export")(self.h, cap, C.byref(n), ident.ctypes.data, count.ctypes.data, rows.ctypes.data), "export")
        return n.value, ident, count, rows
