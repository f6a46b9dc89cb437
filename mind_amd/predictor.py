"""Host-side handle on the HIP scene predictor (one context per process/GPU)."""
import ctypes as C

import numpy as np
import torch

from . import _lib


# record layout of mind_aime_node (include/mind_hip.h)
AIME_NODE_DTYPE = np.dtype({"names": ["round", "scene", "mode", "parent", "prob", "cur_t", "end_t", "flags", "dur", "row_off", "tgt_pts"],
                            "formats": ["<i4", "<i4", "<i4", "<i4", "<f4", "<i4", "<i4", "<i4", "<i4", "<i8", ("<f4", (22,))],
                            "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48], "itemsize": 136})


class IlqrCall:
    """One tree-iLQR call split into its three parts, so that a caller can prepare the arguments on its own thread, hand
    only ``run`` (a single C call, which releases the GIL) to another thread / context and read the results later.
    cfg_full given: mind_ilqr_contingency (warm-start fit with ``cfg``, then full fit with ``cfg_full``); otherwise
    mind_ilqr_solve_trees with ``use_exo`` / ``us_init``."""

    def __init__(self, lib, cfg, flats, x0, lane, target_vel, cfg_full=None, use_exo=1, us_init=None, background=False):
        self.lib, self.cfg, self.cfg_full, self.use_exo = lib, cfg, cfg_full, int(use_exo)
        # a fit that runs beside the predictor (speculative warm start) stays on one workgroup per tree: the multi-workgroup
        # kernel's barrier spins would hold CUs the predictor needs
        self.background = bool(background)
        n = self.n = len(flats)
        self.trees = (_lib.CostTree * n)()
        self.keep, self.Ms = [], []
        for i, f in enumerate(flats):
            par = np.ascontiguousarray(f["parent"], np.int32)
            prob = np.ascontiguousarray(f["prob"], np.float32)
            mean = np.ascontiguousarray(f["mean"], np.float32)
            cov = np.ascontiguousarray(f["cov"], np.float32)
            self.keep += [par, prob, mean, cov]
            t = self.trees[i]
            t.n_nodes = len(par)
            t.parent = par.ctypes.data_as(C.POINTER(C.c_int32))
            t.prob = prob.ctypes.data_as(C.POINTER(C.c_float))
            t.n_agents = mean.shape[1]
            t.agent_mean = mean.ctypes.data_as(C.POINTER(C.c_float))
            t.agent_cov = cov.ctypes.data_as(C.POINTER(C.c_float))
            self.Ms.append(len(par))
        Mt = int(sum(self.Ms))
        self.x0 = np.ascontiguousarray(x0, np.float64)
        self.lane = np.ascontiguousarray(lane, np.float64)
        self.tv = C.c_double(float(target_vel))
        self.xs, self.us = np.zeros((Mt, 6)), np.zeros((Mt, 2))
        self.st = (_lib.IlqrStats * n)()
        self.st_full = (_lib.IlqrStats * n)() if cfg_full is not None else None
        self.ui = None if us_init is None else np.ascontiguousarray(np.concatenate(us_init), np.float64)
        self.rc, self.ctx = None, None

    def run(self, rt):
        """the launch (+ its synchronisation) on ``rt``'s context; nothing else happens here"""
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        self.ctx = rt.ctx
        rt.ilqr_background(self.background)
        if self.cfg_full is not None:
            self.rc = self.lib.mind_ilqr_contingency(rt.ctx, C.byref(self.cfg), C.byref(self.cfg_full), self.trees, self.n, dp(self.x0),
                                                     dp(self.lane), len(self.lane), self.tv, dp(self.xs), dp(self.us), self.st, self.st_full)
        else:
            self.rc = self.lib.mind_ilqr_solve_trees(rt.ctx, C.byref(self.cfg), self.trees, self.n, dp(self.x0), dp(self.lane),
                                                     len(self.lane), self.tv, self.use_exo, dp(self.ui), dp(self.xs), dp(self.us), self.st)
        return self

    def begin(self, rt):
        """upload + launch + queued read-backs of a contingency call (mind_ilqr_contingency_begin): returns without waiting for the
        kernel; ``wait`` collects it.  The caller's thread is free in between (the planner builds its Python trees there)."""
        assert self.cfg_full is not None and not self.background
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        self.ctx = rt.ctx
        self._rt = rt
        rt.ilqr_background(False)
        self.rc = self.lib.mind_ilqr_contingency_begin(rt.ctx, C.byref(self.cfg), C.byref(self.cfg_full), self.trees, self.n, dp(self.x0),
                                                       dp(self.lane), len(self.lane), self.tv, dp(self.xs), dp(self.us), self.st, self.st_full)
        self._begun = self.rc == 0
        return self

    def wait(self):
        if getattr(self, "_begun", False):
            self._begun = False
            rt = getattr(self, "_rt", None)
            if rt is not None and (rt.ctx is None or rt.ctx.value != self.ctx.value):
                # the runtime was closed (mind_ctx_destroy drained the stream and dropped the pending half): nothing to collect
                self.rc = _lib.MIND_ESTATE
            else:
                self.rc = self.lib.mind_ilqr_finish(self.ctx)
        return self

    def finish(self):
        name = "mind_ilqr_contingency" if self.cfg_full is not None else "mind_ilqr_solve_trees"
        _lib.check(self.lib, self.ctx, self.rc, name)
        offs = np.cumsum([0] + self.Ms)
        n = self.n
        stats = lambda s_: [dict(iterations=s_[i].iterations, converged=s_[i].converged, J=s_[i].J, mu=s_[i].mu) for i in range(n)]
        xs = [self.xs[offs[i]:offs[i + 1]] for i in range(n)]
        us = [self.us[offs[i]:offs[i + 1]] for i in range(n)]
        if self.cfg_full is not None:
            return xs, us, stats(self.st), stats(self.st_full)
        return xs, us, stats(self.st)


class PlanIlqrCall(IlqrCall):
    """The contingency call on the cost trees the context's last mind_aime_plan flattened (mind_ilqr_contingency_begin_plan): the tree
    arrays never leave the library, only the node counts are needed here to size and split the results."""

    def __init__(self, lib, cfg, cfg_full, node_counts, x0, lane, target_vel):
        self.lib, self.cfg, self.cfg_full, self.use_exo, self.background = lib, cfg, cfg_full, 1, False
        self.Ms = [int(m) for m in node_counts]
        n = self.n = len(self.Ms)
        Mt = int(sum(self.Ms))
        self.x0 = np.ascontiguousarray(x0, np.float64)
        self.lane = np.ascontiguousarray(lane, np.float64)
        self.tv = float(target_vel)
        self.xs, self.us = np.zeros((Mt, 6)), np.zeros((Mt, 2))
        self.st, self.st_full = (_lib.IlqrStats * n)(), (_lib.IlqrStats * n)()
        self.ui, self.rc, self.ctx = None, None, None

    def begin(self, rt):
        self.ctx = rt.ctx
        self._rt = rt              # (wait() refuses to collect from a runtime that was closed meanwhile)
        rt.ilqr_background(False)
        self.rc = self.lib.mind_ilqr_contingency_begin_plan(rt.ctx, C.byref(self.cfg), C.byref(self.cfg_full), self.x0.ctypes.data, self.lane.ctypes.data,
                                                            len(self.lane), self.tv, self.xs.ctypes.data, self.us.ctypes.data, self.st, self.st_full)
        self._begun = self.rc == 0
        return self

    def run(self, rt):
        return self.begin(rt).wait()


class BegunPlanIlqrCall(PlanIlqrCall):
    """The contingency call mind_aime_plan began itself behind its plan (mind_aime_plan_in.solve_*, out.solves_begun): nothing to launch
    here, ``wait`` collects it (mind_ilqr_finish_plan copies the results out of the library)."""

    def __init__(self, rt, cfg, cfg_full, node_counts, x0, lane, target_vel):
        super().__init__(rt.lib, cfg, cfg_full, node_counts, x0, lane, target_vel)
        self.ctx, self._rt, self._begun, self.rc = rt.ctx, rt, True, 0

    def begin(self, rt):
        return self

    def wait(self):
        if getattr(self, "_begun", False):
            self._begun = False
            rt = self._rt
            if rt.ctx is None or rt.ctx.value != self.ctx.value:
                self.rc = _lib.MIND_ESTATE
            else:
                self.rc = self.lib.mind_ilqr_finish_plan(self.ctx, int(sum(self.Ms)), self.n, self.xs.ctypes.data, self.us.ctypes.data,
                                                         C.cast(self.st, C.c_void_p), C.cast(self.st_full, C.c_void_p))
        return self


class HipPredictor:
    """Owns a ``mind_ctx`` bound to ``device`` and the current torch stream; ``load_state_dict`` mirrors
    ``ScenePredNet.load_state_dict`` (reference planners/mind/planner.py:46-48), ``predict`` mirrors
    ``ScenePredNet.forward`` over a collated batch (planners/mind/networks/network.py:582-595)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("HipPredictor needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", device if isinstance(device, int) else (device.index or 0))
        torch.cuda.set_device(self.device)
        self.ctx = C.c_void_p()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        # the legacy default stream couples every synchronisation and kernel of this context to the other streams of the process
        # (measured: the device-side window assembly of mind_aime_rebase then stalls for 10-25 ms on entry)
        self.on_default_stream = int(stream or 0) == 0
        rc = self.lib.mind_ctx_create(self.device.index, C.c_void_p(stream), C.byref(self.ctx))
        _lib.check(self.lib, None, rc, "mind_ctx_create")
        self._keep = []

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mind_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd, param_out=None):
        """``param_out``: the curve basis the checkpoint was trained with ('bezier' | 'monomial', SceneDecoder's param_out), set before the
        load; None keeps the context's (Bezier unless set_decoder_basis said otherwise).  The two bases have the same tensor shapes, so the
        state dict cannot tell."""
        if param_out is not None:
            self.set_decoder_basis(param_out)
        descs, keep = _lib.tensor_descs(sd)
        rc = self.lib.mind_weights_load(self.ctx, descs, len(sd))
        _lib.check(self.lib, self.ctx, rc, "mind_weights_load")

    PAIR_PREC = ("f32", "bf16x3", "bf16", "bf16x6")

    def pair_precision(self):
        """arithmetic of the predictor's MFMA contractions: 'bf16x6' (default: exact three-way split, fp32 class) | 'f32' | 'bf16x3' | 'bf16' (include/mind_hip.h)"""
        return self.PAIR_PREC[self.lib.mind_get_pair_precision(self.ctx)]

    def set_tuning(self, name, value):
        """one tuning knob (mind_set_tuning); ``_lib.knobs()`` lists them, include/mind_hip.h says what each does"""
        _lib.check(self.lib, self.ctx, self.lib.mind_set_tuning(self.ctx, name.encode(), int(value)), "mind_set_tuning")
        if name == "ilqr_wgs":
            self._ilqr_wgs_saved = None         # (what the user asks for is not undone by the next foreground solve)

    def get_tuning(self, name):
        """the value the knob holds now (mind_get_tuning): a flag as 0 / 1"""
        v = C.c_int()
        _lib.check(self.lib, self.ctx, self.lib.mind_get_tuning(self.ctx, name.encode(), C.byref(v)), "mind_get_tuning")
        return v.value

    _ilqr_wgs_saved = None

    def ilqr_background(self, on):
        """entering a background tree-iLQR fit saves "ilqr_wgs" and sets 1; the next foreground call puts the saved value back"""
        if on and self._ilqr_wgs_saved is None:
            self._ilqr_wgs_saved = self.get_tuning("ilqr_wgs")
            self.lib.mind_set_tuning(self.ctx, b"ilqr_wgs", 1)
        elif not on and self._ilqr_wgs_saved is not None:
            self.lib.mind_set_tuning(self.ctx, b"ilqr_wgs", self._ilqr_wgs_saved)
            self._ilqr_wgs_saved = None

    def set_pair_precision(self, name):
        _lib.check(self.lib, self.ctx, self.lib.mind_set_pair_precision(self.ctx, self.PAIR_PREC.index(name)), "mind_set_pair_precision")

    def set_decoder_basis(self, name):
        """the decoder's curve basis, 'bezier' (default) | 'monomial' (mind_set_decoder_basis): holds for every predictor call on this context
        and across load_state_dict.  The context must be idle."""
        if name not in _lib.BASIS:
            raise ValueError(f"unknown decoder basis {name!r}: one of {_lib.BASIS}")
        _lib.check(self.lib, self.ctx, self.lib.mind_set_decoder_basis(self.ctx, _lib.BASIS.index(name)), "mind_set_decoder_basis")

    def get_decoder_basis(self):
        return _lib.BASIS[self.lib.mind_get_decoder_basis(self.ctx)]

    def curve_eval(self, param, tau, basis=None, want=("reg", "vel", "cov_vel")):
        """The decoder's curves at the times ``tau`` (fractions of the 6 s horizon, each in [0, 1]) from control points ``param`` [..., 8, 5]
        (float32, this device; predict(aux=True)["param"]): dict of reg [..., n_tau, 5] = (x, y, exp sx, exp sy, exp rho), vel [..., n_tau, 2],
        cov_vel [..., n_tau, 3] as named in ``want``.  ``basis``: 'bezier' | 'monomial' | None = the context's.  At tau = linspace(0, 1, 60) the
        results are the decoder's own, bit for bit (mind_curve_eval)."""
        assert param.device == self.device and param.dtype == torch.float32 and tuple(param.shape[-2:]) == (8, 5), (param.device, param.dtype, param.shape)
        if basis is not None and basis not in _lib.BASIS:
            raise ValueError(f"unknown decoder basis {basis!r}: one of {_lib.BASIS}")
        widths = {"reg": 5, "vel": 2, "cov_vel": 3}
        if any(k not in widths for k in want):
            raise ValueError(f"curve_eval: want names {tuple(want)!r}, of {tuple(widths)}")
        param = param.contiguous()
        tau = np.ascontiguousarray(tau, np.float64).ravel()
        lead, n = tuple(param.shape[:-2]), param.numel() // 40
        out = {k: torch.empty(lead + (tau.size, w), device=self.device) for k, w in widths.items() if k in want}
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out and out[k].numel() > 0 else None
        rc = self.lib.mind_curve_eval(self.ctx, -1 if basis is None else _lib.BASIS.index(basis), C.c_void_p(param.data_ptr()) if n else None, n,
                                      tau.ctypes.data_as(C.POINTER(C.c_double)), tau.size, ptr("reg"), ptr("vel"), ptr("cov_vel"))
        _lib.check(self.lib, self.ctx, rc, "mind_curve_eval")
        return out

    def set_profiling(self, on):
        self.lib.mind_set_profiling(self.ctx, 1 if on else 0)

    def ilqr_stats(self):
        """(kernel ms, cost trees, workgroups per tree) of the last tree-iLQR call on this context (ms = 0 unless profiling)"""
        ms, n, g = C.c_float(), C.c_int(), C.c_int()
        self.lib.mind_last_ilqr_stats(self.ctx, C.byref(ms), C.byref(n), C.byref(g))
        return ms.value, n.value, g.value

    def ilqr_profile(self):
        """phase cycles of the critical cost tree of the last tree-iLQR launch (mind_last_ilqr_profile)"""
        v = (C.c_double * 9)()
        self.lib.mind_last_ilqr_profile(self.ctx, v)
        keys = ("nodes", "depth", "passes", "derivatives", "backward", "state_chain", "cost_pass", "selection", "trees")
        return dict(zip(keys, [float(x) for x in v]))

    def ilqr_trace(self, tree, phase=0):
        """[iterations, 4] float64 per-iteration trace of one fit of the last tree-iLQR call (mind_last_ilqr_trace): mu, J of the nominal
        trajectory, accepted step index (-1 rejected, -2 singular Q_uu), J of the accepted candidate"""
        n = C.c_int()
        buf = np.zeros((256, 4), np.float64)
        _lib.check(self.lib, self.ctx, self.lib.mind_last_ilqr_trace(self.ctx, int(tree), int(phase), buf.ctypes.data_as(C.POINTER(C.c_double)), 256,
                                                                    C.byref(n)), "mind_last_ilqr_trace")
        return buf[:min(n.value, 256)].copy()

    def fusion_stats(self):
        n = C.c_int()
        ms = C.c_float()
        pairs = C.c_double()
        self.lib.mind_last_fusion_stats(self.ctx, C.byref(n), C.byref(ms), C.byref(pairs))
        return n.value, ms.value, pairs.value

    def launch_times(self, kind="pair"):
        """(by the launch clock, by HIP events): ms per timed launch of the last read, in launch order (mind_debug_launch_times; kind "pair" or
        "actor").  Either list is empty when its mechanism was not armed: mind_set_tuning("prof_clock", 0 events | 1 clock | 2 both)"""
        cap = 4096
        ck, ev = (C.c_float * cap)(), (C.c_float * cap)()
        nc, ne = C.c_int(), C.c_int()
        _lib.check(self.lib, self.ctx, self.lib.mind_debug_launch_times(self.ctx, {"pair": 0, "actor": 1}[kind], ck, ev, cap, C.byref(nc), C.byref(ne)),
                   "mind_debug_launch_times")
        return [float(v) for v in ck[:min(nc.value, cap)]], [float(v) for v in ev[:min(ne.value, cap)]]

    def last_actor_stats(self):
        """ActorNet of the last predictor call (mind_last_actor_stats): dict(layerwise = 1 when the layer-wise batched kernels ran, launches,
        chunks, ms = first launch to last on the context stream, 0 unless profiling)"""
        lw, n, ch, ms = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        _lib.check(self.lib, self.ctx, self.lib.mind_last_actor_stats(self.ctx, C.byref(lw), C.byref(n), C.byref(ch), C.byref(ms)), "mind_last_actor_stats")
        return dict(layerwise=lw.value, launches=n.value, chunks=ch.value, ms=ms.value)

    def last_token_stats(self):
        """Token stage of the last predictor call (mind_last_token_stats): dict(layerwise = 1 when a run took the layer-wise kernels, launches of
        all token steps, chunks of the layer-wise runs, ms = summed launch times, stage_ms = by kernel (mind_last_token_stage_ms); 0 unless
        profiling)"""
        lw, n, ch, ms = C.c_int(), C.c_int(), C.c_int(), C.c_float()
        _lib.check(self.lib, self.ctx, self.lib.mind_last_token_stats(self.ctx, C.byref(lw), C.byref(n), C.byref(ch), C.byref(ms)), "mind_last_token_stats")
        st = (C.c_float * 8)()
        self.lib.mind_last_token_stage_ms(self.ctx, st, 8)
        return dict(layerwise=lw.value, launches=n.value, chunks=ch.value, ms=ms.value, stage_ms=[float(v) for v in st])

    def debug_set_layers(self, n):
        _lib.check(self.lib, self.ctx, self.lib.mind_debug_set_layers(self.ctx, n), "mind_debug_set_layers")

    def debug_read(self, name):
        n = self.lib.mind_debug_read(self.ctx, name.encode(), None, 0)
        if n < 0:
            raise _lib.MindError(f"mind_debug_read({name}) -> {n}")
        buf = np.empty(n, np.float32)
        got = self.lib.mind_debug_read(self.ctx, name.encode(), buf.ctypes.data_as(C.POINTER(C.c_float)), n)
        assert got == n, (got, n)
        return buf

    def synchronize(self):
        _lib.check(self.lib, self.ctx, self.lib.mind_ctx_synchronize(self.ctx), "mind_ctx_synchronize")

    def predict(self, actors, actor_off, lanes, lane_off, actor_ctrs, actor_vecs, lane_ctrs, lane_vecs,
                tgt_nodes, tgt_rpe, rpe=None, lane_feat=None, want_lane_feat=False, taps=False, aux=False):
        """All tensors fp32 contiguous on ``self.device``; actor_off/lane_off are int prefix-sum lists [B+1].
        Returns dict(cls [B,6], reg [A,6,60,5], vel [A,6,60,2], ...); with ``aux`` also cov_vel [A,6,60,3] and param [A,6,8,5] (the control
        points, agent-major: the rest of the reference's res_aux, network.py:554)."""
        dev = self.device
        B = len(actor_off) - 1
        A, L = int(actor_off[-1]), int(lane_off[-1])

        def f32(t):
            if t is None:
                return None
            assert t.device == dev and t.dtype == torch.float32, (t.device, t.dtype)
            return t.contiguous()

        actors, lanes, lane_feat = f32(actors), f32(lanes), f32(lane_feat)
        actor_ctrs, actor_vecs, lane_ctrs, lane_vecs = f32(actor_ctrs), f32(actor_vecs), f32(lane_ctrs), f32(lane_vecs)
        tgt_nodes, tgt_rpe = f32(tgt_nodes), f32(tgt_rpe)
        assert actors.shape == (A, 14, 48) and tgt_nodes.shape == (B, 10, 16) and tgt_rpe.shape == (B, 20)
        ao = (C.c_int32 * (B + 1))(*[int(v) for v in actor_off])
        lo = (C.c_int32 * (B + 1))(*[int(v) for v in lane_off])
        sb = _lib.SceneBatch()
        sb.n_scenes = B
        sb.actor_off, sb.lane_off = ao, lo

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None

        sb.actors, sb.lanes, sb.lane_feat = ptr(actors), ptr(lanes), ptr(lane_feat)
        sb.actor_ctrs, sb.actor_vecs, sb.lane_ctrs, sb.lane_vecs = ptr(actor_ctrs), ptr(actor_vecs), ptr(lane_ctrs), ptr(lane_vecs)
        rpe_keep = None
        if rpe is not None:
            rpe_keep = [f32(r) for r in rpe]
            arr = (C.c_void_p * B)(*[r.data_ptr() for r in rpe_keep])
            sb.rpe = arr
        sb.tgt_nodes, sb.tgt_rpe = ptr(tgt_nodes), ptr(tgt_rpe)
        out = {"cls": torch.empty(B, 6, device=dev), "reg": torch.empty(A, 6, 60, 5, device=dev),
               "vel": torch.empty(A, 6, 60, 2, device=dev)}
        po = _lib.PredOut()
        po.cls, po.reg, po.vel = ptr(out["cls"]), ptr(out["reg"]), ptr(out["vel"])
        if want_lane_feat and lane_feat is None and L > 0:
            out["lane_feat"] = torch.empty(L, 128, device=dev)
            po.lane_feat = ptr(out["lane_feat"])
        if taps:
            out["actor_emb"] = torch.empty(A, 128, device=dev)
            out["cls_emb"] = torch.empty(B, 128, device=dev)
            po.actor_emb, po.cls_emb = ptr(out["actor_emb"]), ptr(out["cls_emb"])
        if aux:
            out["cov_vel"] = torch.empty(A, 6, 60, 3, device=dev)
            out["param"] = torch.empty(A, 6, 8, 5, device=dev)
            pa = _lib.PredAux(ptr(out["cov_vel"]), ptr(out["param"]))
            rc = self.lib.mind_predict_batch_aux(self.ctx, C.byref(sb), C.byref(po), C.byref(pa))
        else:
            rc = self.lib.mind_predict_batch(self.ctx, C.byref(sb), C.byref(po))
        _lib.check(self.lib, self.ctx, rc, "mind_predict_batch")
        return out

    # ------------------------------------------------------------------------------------------
    def ilqr_contingency(self, cfg_warm, cfg_full, flats, x0, lane, target_vel):
        """Warm-start fit + full fit of all cost trees of a plan in one launch (mind_ilqr_contingency).
        Returns (xs list[[M,6]], us list[[M,2]], stats_warm list[dict], stats_full list[dict])."""
        call = IlqrCall(self.lib, cfg_warm, flats, x0, lane, target_vel, cfg_full=cfg_full)
        call.run(self)
        return call.finish()

    def ilqr_solve(self, cfg, flats, x0, lane, target_vel, use_exo, us_init=None):
        """Solve all cost trees of a plan in one launch.  ``flats``: list of dicts with parent int32 [M],
        prob f32 [M], mean f32 [M,a,2], cov f32 [M,a] (trajectory-node arrays in creation order);
        ``cfg``: ``_lib.IlqrCfg``.  Returns (xs list[[M,6]], us list[[M,2]], stats list[dict])."""
        call = IlqrCall(self.lib, cfg, flats, x0, lane, target_vel, use_exo=use_exo, us_init=us_init)
        call.run(self)
        return call.finish()

    # ---- planners/ilqr surface: arbitrary materialised fields + per-node quadratic potentials -------------
    @staticmethod
    def _generic_tree(tree, keep):
        """tree: dict(parent int32 [M], field f64 [M,H,W], node_w f64 [M,32]) -> CostTree."""
        ct = _lib.CostTree()
        par = np.ascontiguousarray(tree["parent"], np.int32)
        fld = np.ascontiguousarray(tree["field"], np.float64)
        nw = np.ascontiguousarray(tree["node_w"], np.float64)
        if fld.ndim != 3 or fld.shape[0] != len(par) or nw.shape != (len(par), 32):
            raise ValueError("generic cost tree: field [M,H,W] / node_w [M,32] do not match parent [M]")
        keep += [par, fld, nw]
        ct.n_nodes, ct.n_agents = len(par), 0
        ct.parent = par.ctypes.data_as(C.POINTER(C.c_int32))
        ct.field = fld.ctypes.data_as(C.POINTER(C.c_double))
        ct.node_w = nw.ctypes.data_as(C.POINTER(C.c_double))
        return ct

    @staticmethod
    def _grid(grid, keep):
        """grid: dict(offset [2], res, gx [W], gy [H]) as PotentialField receives them."""
        g = _lib.FieldGrid()
        gx = np.ascontiguousarray(grid["gx"], np.float64)
        gy = np.ascontiguousarray(grid["gy"], np.float64)
        keep += [gx, gy]
        g.W, g.H, g.res = len(gx), len(gy), float(grid["res"])
        g.off_x, g.off_y = float(grid["offset"][0]), float(grid["offset"][1])
        g.gx = gx.ctypes.data_as(C.POINTER(C.c_double))
        g.gy = gy.ctypes.data_as(C.POINTER(C.c_double))
        return g

    def ilqr_solve_fields(self, cfg, grid, tree, x0, us_init=None):
        """iLQR.fit on ONE tree with materialised fields (mind_ilqr_solve_fields).  Returns (xs [M,6], us [M,2], stats)."""
        keep = []
        ct = self._generic_tree(tree, keep)
        g = self._grid(grid, keep)
        M = ct.n_nodes
        x0 = np.ascontiguousarray(x0, np.float64)
        xs, us = np.zeros((M, 6)), np.zeros((M, 2))
        st = _lib.IlqrStats()
        ui = None if us_init is None else np.ascontiguousarray(us_init, np.float64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        rc = self.lib.mind_ilqr_solve_fields(self.ctx, C.byref(cfg), C.byref(g), C.byref(ct), 1, dp(x0), dp(ui), dp(xs), dp(us),
                                             C.byref(st))
        _lib.check(self.lib, self.ctx, rc, "mind_ilqr_solve_fields")
        return xs, us, dict(iterations=st.iterations, converged=st.converged, J=st.J, mu=st.mu)

    def cost_eval(self, cfg, node, x, u, tree, grid=None, x0=None, lane=None, target_vel=0.0, use_exo=0):
        """TreeCost.l/l_x/l_u/l_xx/l_uu of ``tree`` at (x[q], u[q]) for node[q] (mind_cost_eval).
        grid given: generic tree dict; grid None: planner-mode flat dict (parent, prob, mean, cov) + x0, lane.
        Returns dict(l [Q], l_x [Q,6], l_u [Q,2], l_xx [Q,6,6], l_uu [Q,2,2])."""
        keep = []
        if grid is not None:
            ct = self._generic_tree(tree, keep)
            g = C.byref(self._grid(grid, keep))
            x0 = np.zeros(6) if x0 is None else x0
        else:
            ct = _lib.CostTree()
            par = np.ascontiguousarray(tree["parent"], np.int32)
            prob = np.ascontiguousarray(tree["prob"], np.float32)
            mean = np.ascontiguousarray(tree["mean"], np.float32)
            cov = np.ascontiguousarray(tree["cov"], np.float32)
            keep += [par, prob, mean, cov]
            ct.n_nodes, ct.n_agents = len(par), mean.shape[1]
            ct.parent = par.ctypes.data_as(C.POINTER(C.c_int32))
            ct.prob = prob.ctypes.data_as(C.POINTER(C.c_float))
            ct.agent_mean = mean.ctypes.data_as(C.POINTER(C.c_float))
            ct.agent_cov = cov.ctypes.data_as(C.POINTER(C.c_float))
            g = None
        node = np.ascontiguousarray(node, np.int32)
        x = np.ascontiguousarray(x, np.float64).reshape(len(node), 6)
        u = np.ascontiguousarray(u, np.float64).reshape(len(node), 2)
        x0 = np.ascontiguousarray(x0, np.float64)
        lane_a = None if lane is None else np.ascontiguousarray(lane, np.float64)
        out = np.zeros((len(node), 47))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        rc = self.lib.mind_cost_eval(self.ctx, C.byref(cfg), g, C.byref(ct), dp(x0), dp(lane_a), 0 if lane_a is None else len(lane_a),
                                     C.c_double(float(target_vel)), int(use_exo), len(node),
                                     node.ctypes.data_as(C.POINTER(C.c_int32)), dp(x), dp(u), dp(out))
        _lib.check(self.lib, self.ctx, rc, "mind_cost_eval")
        luu = np.zeros((len(node), 2, 2))
        luu[:, 0, 0], luu[:, 1, 1] = out[:, 45], out[:, 46]
        return dict(l=out[:, 0].copy(), l_x=out[:, 1:7].copy(), l_u=out[:, 7:9].copy(), l_xx=out[:, 9:45].reshape(-1, 6, 6).copy(), l_uu=luu)

    def ilqr_score(self, cfg, flats, x0, lane, target_vel, use_exo, us_cand, grid=None, want_xs=True, want_L=True):
        """Rollout + TreeCost of C candidate control trees on every cost tree of ``flats`` in one launch, no optimisation
        (mind_ilqr_score_trees).  grid None: planner-mode flat dicts as ``ilqr_solve`` takes them; grid given: generic tree dicts
        (parent, field, node_w) as ``ilqr_solve_fields`` takes one, ``lane`` / ``use_exo`` ignored.  ``us_cand``: [C, sum M, 2], or one
        array [C, M_t, 2] per tree.  Returns (xs list[[C, M_t, 6]], L list[[C, M_t]], J [C, n_trees]); J[c, t] is the J a fit of one
        iteration from candidate c reports.  want_xs / want_L False: that output is not read back (None in its place)."""
        n = len(flats)
        keep = []
        trees, Ms = self._cost_trees(flats, grid, keep)
        Mt = int(sum(Ms))
        if isinstance(us_cand, (list, tuple)):
            us_cand = np.concatenate([np.asarray(u, np.float64) for u in us_cand], axis=1)
        uc = np.ascontiguousarray(us_cand, np.float64)
        if uc.ndim != 3 or uc.shape[1:] != (Mt, 2):
            raise ValueError(f"us_cand must be [C, {Mt}, 2] for these cost trees, got {uc.shape}")
        nc = uc.shape[0]
        g = C.byref(self._grid(grid, keep)) if grid is not None else None
        x0 = np.ascontiguousarray(x0, np.float64)
        lane_a = None if lane is None or grid is not None else np.ascontiguousarray(lane, np.float64)
        xs = np.zeros((nc, Mt, 6)) if want_xs else None
        L = np.zeros((nc, Mt)) if want_L else None
        J = np.zeros((nc, n))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        rc = self.lib.mind_ilqr_score_trees(self.ctx, C.byref(cfg), g, trees, n, dp(x0), dp(lane_a), 0 if lane_a is None else len(lane_a),
                                            C.c_double(float(target_vel)), int(use_exo), nc, dp(uc), dp(xs), dp(L), dp(J))
        _lib.check(self.lib, self.ctx, rc, "mind_ilqr_score_trees")
        offs = np.cumsum([0] + Ms)
        split = lambda a: None if a is None else [a[:, offs[i]:offs[i + 1]].copy() for i in range(n)]
        return split(xs), split(L), J

    def _cost_trees(self, flats, grid, keep):
        """flats -> (CostTree array, node counts): planner-mode flat dicts (grid None) or generic tree dicts, as ``ilqr_score`` takes them"""
        trees = (_lib.CostTree * max(len(flats), 1))()
        Ms = []
        for i, f in enumerate(flats):
            if grid is not None:
                trees[i] = self._generic_tree(f, keep)
            else:
                par = np.ascontiguousarray(f["parent"], np.int32)
                prob = np.ascontiguousarray(f["prob"], np.float32)
                mean = np.ascontiguousarray(f["mean"], np.float32)
                cov = np.ascontiguousarray(f["cov"], np.float32)
                keep += [par, prob, mean, cov]
                t = trees[i]
                t.n_nodes, t.n_agents = len(par), mean.shape[1]
                t.parent = par.ctypes.data_as(C.POINTER(C.c_int32))
                t.prob = prob.ctypes.data_as(C.POINTER(C.c_float))
                t.agent_mean = mean.ctypes.data_as(C.POINTER(C.c_float))
                t.agent_cov = cov.ctypes.data_as(C.POINTER(C.c_float))
            Ms.append(int(trees[i].n_nodes))
        return trees, Ms

    @staticmethod
    def _per_node(a, Mt, tail, name):
        """one [sum M, *tail] array from one array or one array per tree"""
        if isinstance(a, (list, tuple)):
            a = np.concatenate([np.asarray(v, np.float64).reshape((-1,) + tail) for v in a], axis=0)
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != (Mt,) + tail:
            raise ValueError(f"{name} must be {[Mt] + list(tail)} for these cost trees, got {list(a.shape)}")
        return a

    def ilqr_gains(self, cfg, flats, x0, lane, target_vel, use_exo, us, mu, grid=None):
        """The gains of one backward pass about the controls ``us`` ([sum M, 2], or one [M_t, 2] per tree) with the regularisation ``mu``
        (a number or one per tree) on every cost tree of ``flats`` in one launch (mind_ilqr_gains, k_ilqr_gains); flats / grid as
        ``ilqr_score``.  Returns a dict of per-tree lists k [M_t,2], K [M_t,2,6], dV [M_t], V_x [M_t,6], V_xx [M_t,6,6] (after the node's own
        update; no alias row), xs [M_t,6], L [M_t], plus J [n_trees] and bad_node int32 [n_trees] (-1: fine; else the tree's gains are zeros)."""
        n = len(flats)
        keep = []
        trees, Ms = self._cost_trees(flats, grid, keep)
        Mt = int(sum(Ms))
        u = self._per_node(us, Mt, (2,), "us")
        mu_a = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, np.float64), (n,)))
        g = C.byref(self._grid(grid, keep)) if grid is not None else None
        x0 = np.ascontiguousarray(x0, np.float64)
        lane_a = None if lane is None or grid is not None else np.ascontiguousarray(lane, np.float64)
        shapes = dict(k=(Mt, 2), K=(Mt, 2, 6), dV=(Mt,), V_x=(Mt, 6), V_xx=(Mt, 6, 6), xs=(Mt, 6), L=(Mt,), J=(n,))
        res = {name: np.zeros(s) for name, s in shapes.items()}
        bad = np.full(n, -1, np.int32)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        out = _lib.IlqrGainsOut()
        for name, a in res.items():
            setattr(out, name, dp(a))
        out.bad_node = bad.ctypes.data_as(C.POINTER(C.c_int32))
        rc = self.lib.mind_ilqr_gains(self.ctx, C.byref(cfg), g, trees, n, dp(x0), dp(lane_a), 0 if lane_a is None else len(lane_a),
                                      C.c_double(float(target_vel)), int(use_exo), dp(u), dp(mu_a), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_ilqr_gains")
        offs = np.cumsum([0] + Ms)
        ret = {name: [a[offs[i]:offs[i + 1]].copy() for i in range(n)] for name, a in res.items() if name != "J"}
        ret["J"], ret["bad_node"] = res["J"], bad
        return ret

    def ilqr_policy_rollouts(self, cfg, flats, x0, lane, target_vel, use_exo, us, k, K, alpha, dx0=None, grid=None, want_xs=True,
                             want_us=True, want_L=True):
        """Closed-loop rollouts under the gains (k, K) about ``us`` on every cost tree of ``flats`` in one launch (mind_ilqr_policy_rollouts,
        k_ilqr_policy): candidate c applies u = us + alpha[c] k + K (x - xs_nominal) from the start state x0 + dx0[c].  us / k / K: [sum M, ..]
        or one array per tree; alpha [C]; dx0 [C, 6] or None (zeros).  Returns (xs list[[C, M_t, 6]], us list[[C, M_t, 2]], L list[[C, M_t]],
        J [C, n_trees]); J is the line search's sequential sum of L.  want_* False: that output is not read back (None in its place)."""
        n = len(flats)
        keep = []
        trees, Ms = self._cost_trees(flats, grid, keep)
        Mt = int(sum(Ms))
        u = self._per_node(us, Mt, (2,), "us")
        k_a = self._per_node(k, Mt, (2,), "k")
        K_a = self._per_node(K, Mt, (2, 6), "K")
        al = np.ascontiguousarray(alpha, np.float64)
        if al.ndim != 1:
            raise ValueError(f"alpha must be [C], got {list(al.shape)}")
        nc = len(al)
        d0 = None if dx0 is None else np.ascontiguousarray(dx0, np.float64)
        if d0 is not None and d0.shape != (nc, 6):
            raise ValueError(f"dx0 must be [{nc}, 6], got {list(d0.shape)}")
        g = C.byref(self._grid(grid, keep)) if grid is not None else None
        x0 = np.ascontiguousarray(x0, np.float64)
        lane_a = None if lane is None or grid is not None else np.ascontiguousarray(lane, np.float64)
        xs = np.zeros((nc, Mt, 6)) if want_xs else None
        uo = np.zeros((nc, Mt, 2)) if want_us else None
        L = np.zeros((nc, Mt)) if want_L else None
        J = np.zeros((nc, n))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
        rc = self.lib.mind_ilqr_policy_rollouts(self.ctx, C.byref(cfg), g, trees, n, dp(x0), dp(lane_a), 0 if lane_a is None else len(lane_a),
                                                C.c_double(float(target_vel)), int(use_exo), dp(u), dp(k_a), dp(K_a), nc, dp(al), dp(d0),
                                                dp(xs), dp(uo), dp(L), dp(J))
        _lib.check(self.lib, self.ctx, rc, "mind_ilqr_policy_rollouts")
        offs = np.cumsum([0] + Ms)
        split = lambda a: None if a is None else [a[:, offs[i]:offs[i + 1]].copy() for i in range(n)]
        return split(xs), split(uo), split(L), J

    # ---- clearance audit (mind_audit_plan / mind_audit_episode): outside every planning cycle -------------
    @staticmethod
    def _audit_box(box, name):
        """(length, width[, center_offset]) -> mind_audit_box"""
        return _lib.audit_box(box, name)

    @staticmethod
    def _audit_xs(xs, Mt):
        """``xs`` of a plan audit -- [C, sum M, 6], or one [C, M_t, 6] per tree -> the checked contiguous [C, Mt, 6] array"""
        if isinstance(xs, (list, tuple)):
            xs = np.concatenate([np.asarray(x, np.float64) for x in xs], axis=1)
        x = np.ascontiguousarray(xs, np.float64)
        if x.ndim != 3 or x.shape[1:] != (Mt, 6):
            raise ValueError(f"xs must be [C, {Mt}, 6] for these cost trees, got {list(x.shape)}")
        return x

    @staticmethod
    def _split_nodes(res, Ms):
        """the node_* arrays [C, sum M] of a plan audit's results, in place -> per-tree lists of [C, M_t]"""
        offs = np.cumsum([0] + list(Ms))
        for name in res:
            if name.startswith("node_"):
                res[name] = [res[name][:, offs[i]:offs[i + 1]].copy() for i in range(len(Ms))]
        return res

    @staticmethod
    def _ego_traces(ego_states):
        """``ego_states`` of an episode audit -- [E, S, 4] or [S, 4] -> the checked contiguous [E, S, 4] array"""
        eg = np.ascontiguousarray(ego_states, np.float64)
        if eg.ndim == 2:
            eg = eg[None]
        if eg.ndim != 3 or eg.shape[2] != 4:
            raise ValueError(f"ego_states must be [E, S, 4], got {list(eg.shape)}")
        return eg

    def audit_plan(self, flats, xs, ego_box, exo_margin):
        """Clearance of C candidate state sets on every cost tree of ``flats`` (planner-mode flat dicts as ``ilqr_solve`` takes them) in one
        call (mind_audit_plan, k_audit_plan).  ``xs``: [C, sum M, 6], or one [C, M_t, 6] per tree, as ``ilqr_score`` returns them; ``ego_box``:
        (length, width[, center_offset]); ``exo_margin``: what is added to every agent's max-sigma.  Returns a dict: per-tree lists node_clear
        [C, M_t] / node_agent int32 [C, M_t], and tree_min, tree_node, tree_agent, tree_hits, tree_first, tree_mass [C, n_trees]."""
        n = len(flats)
        keep = []
        trees, Ms = self._cost_trees(flats, None, keep)
        x = self._audit_xs(xs, int(sum(Ms)))
        for i, f in enumerate(flats):
            a = trees[i].n_agents
            if np.shape(f["mean"]) != (Ms[i], a, 2) or np.shape(f["cov"]) != (Ms[i], a) or np.shape(f["prob"]) != (Ms[i],):
                raise ValueError(f"cost tree {i}: prob [M] / mean [M, a, 2] / cov [M, a] do not match parent [M = {Ms[i]}]")
        margin = float(exo_margin)
        if not np.isfinite(margin) or margin < 0.0:
            raise ValueError(f"exo_margin must be finite and >= 0, got {exo_margin!r}")
        box = self._audit_box(ego_box, "ego_box")
        nc = x.shape[0]
        out, res = _lib.out_record(_lib.AuditPlanOut, lambda k: (nc, x.shape[1]) if k.startswith("node_") else (nc, n))
        rc = self.lib.mind_audit_plan(self.ctx, C.byref(box), C.c_double(margin), trees, n, nc, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_plan")
        return self._split_nodes(res, Ms)

    def audit_episode(self, ego_states, exo, valid, boxes, ego_box):
        """Clearance of E ego traces against one replayed scene in one call (mind_audit_episode, k_audit_episode).  ``ego_states``: [E, S, 4]
        (or [S, 4]) = (x, y, v, yaw); ``exo`` [S, n, 5] = (x, y, heading, vx, vy) and ``valid`` [S, n], the layouts of the native loop's
        tables (row 0 is the ego's: not read); ``boxes`` [n, 2] = (length, width) per track; ``ego_box``: (length, width[, center_offset]).
        Returns a dict: step_clear [E, S], step_track int32 [E, S], ego_min [E], ego_step, ego_track, ego_hits, ego_first int32 [E]."""
        eg = self._ego_traces(ego_states)
        E, S = eg.shape[:2]
        ex, va, bx, nt = self._scene_tables(S, exo, valid, boxes)
        box = self._audit_box(ego_box, "ego_box")
        out, res = _lib.out_record(_lib.AuditEpisodeOut, lambda k: (E, S) if k.startswith("step_") else (E,))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc = self.lib.mind_audit_episode(self.ctx, C.byref(box), E, S, nt, dp(eg), dp(ex), va.ctypes.data_as(C.POINTER(C.c_uint8)), dp(bx), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_episode")
        return res

    @staticmethod
    def _scene_tables(S, exo, valid, boxes):
        """the replayed scene of an episode audit -> the checked contiguous exo [S, n, 5], valid uint8 [S, n], boxes [n, 2] and n"""
        ex = np.ascontiguousarray(exo, np.float64)
        va = np.ascontiguousarray(valid, np.uint8)
        bx = np.ascontiguousarray(boxes, np.float64)
        if ex.ndim != 3 or ex.shape[0] != S or ex.shape[2] != 5 or ex.shape[1] < 1:
            raise ValueError(f"exo must be [S = {S}, n >= 1, 5], got {list(ex.shape)}")
        nt = ex.shape[1]
        if va.shape != (S, nt) or bx.shape != (nt, 2):
            raise ValueError(f"valid must be [{S}, {nt}] and boxes [{nt}, 2], got {list(va.shape)} and {list(bx.shape)}")
        if not np.all(np.isfinite(bx[1:])) or np.any(bx[1:] < 0.0):
            raise ValueError("boxes must be finite and >= 0")
        return ex, va, bx, nt

    # ---- time-to-collision audit (mind_audit_ttc): outside every planning cycle ------------------------------
    def audit_ttc(self, ego_states, exo, valid, boxes, ego_box, horizon=3.0, bound=0.95, lanes=0):
        """Time to collision of E ego traces against one replayed scene in one call (mind_audit_ttc, k_audit_ttc): per step, the first time
        at which the ego box and a track's box overlap when both keep the velocity they have at that step (ttc_geom.h; exact, no time
        sampling).  The arguments of ``audit_episode``; ``horizon``: a time above it counts as never (+inf), ``bound``: a step with
        ttc < bound is a hit (both in seconds, both defaults only); ``lanes``: the kernel's layout -- 0 = the library's rule, 1 = thread
        per ego, 2 = lanes over tracks -- which changes no result.  Returns a dict: step_ttc [E, S] (0.0: overlapping now; +inf: none within
        the horizon), step_track int32 [E, S] (-1 for +inf), ego_min [E], ego_step, ego_track, ego_hits, ego_first int32 [E]."""
        eg = self._ego_traces(ego_states)
        E, S = eg.shape[:2]
        ex, va, bx, nt = self._scene_tables(S, exo, valid, boxes)
        horizon, bound = float(horizon), float(bound)
        if not np.isfinite(horizon) or horizon <= 0.0:
            raise ValueError(f"horizon must be finite and > 0, got {horizon!r}")
        if not np.isfinite(bound) or bound < 0.0:
            raise ValueError(f"bound must be finite and >= 0, got {bound!r}")
        if lanes not in (0, 1, 2):
            raise ValueError(f"lanes must be 0 (the library's rule), 1 (thread per ego) or 2 (lanes over tracks), got {lanes!r}")
        box = self._audit_box(ego_box, "ego_box")
        cfg = _lib.AuditTtcCfg(horizon, bound, int(lanes))
        out, res = _lib.out_record(_lib.AuditTtcOut, lambda k: (E, S) if k.startswith("step_") else (E,))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc = self.lib.mind_audit_ttc(self.ctx, C.byref(box), C.byref(cfg), E, S, nt, dp(eg), dp(ex), va.ctypes.data_as(C.POINTER(C.c_uint8)), dp(bx), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_ttc")
        return res

    # ---- road audit (mind_audit_road_plan / mind_audit_road_episode): outside every planning cycle ---------
    def audit_road_plan(self, flats, xs, verts, poly_off, ego_box):
        """Road margin of C candidate state sets on every cost tree of ``flats`` in one call (mind_audit_road_plan, k_road_boxes): the ego
        box at every trajectory node against the drivable area ``verts`` [V, 2] / ``poly_off`` [P + 1] (mind_amd.audit.Road).  ``xs``:
        [C, sum M, 6], or one [C, M_t, 6] per tree; only ``parent`` (for M) and ``prob`` of the trees are read.  Returns a dict: per-tree
        lists node_margin [C, M_t] / node_corner, node_ring, node_edge int32 [C, M_t], and tree_min, tree_node, tree_corner, tree_hits,
        tree_first, tree_mass [C, n_trees]."""
        n = len(flats)
        keep = []
        trees, Ms = self._cost_trees(flats, None, keep)
        x = self._audit_xs(xs, int(sum(Ms)))
        for i, f in enumerate(flats):
            if np.shape(f["prob"]) != (Ms[i],):
                raise ValueError(f"cost tree {i}: prob [M] does not match parent [M = {Ms[i]}]")
        v, off, vp, op, P = _lib.road_args(verts, poly_off)
        box = self._audit_box(ego_box, "ego_box")
        nc = x.shape[0]
        out, res = _lib.out_record(_lib.AuditRoadPlanOut, lambda k: (nc, x.shape[1]) if k.startswith("node_") else (nc, n))
        rc = self.lib.mind_audit_road_plan(self.ctx, C.byref(box), vp, op, P, trees, n, nc, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_road_plan")
        return self._split_nodes(res, Ms)

    def audit_road_episode(self, ego_states, verts, poly_off, ego_box):
        """Road margin of E ego traces in one call (mind_audit_road_episode, k_road_boxes).  ``ego_states``: [E, S, 4] (or [S, 4]) =
        (x, y, v, yaw); the road as ``audit_road_plan`` takes it.  Returns a dict: step_margin [E, S], step_corner, step_ring, step_edge
        int32 [E, S], ego_min [E], ego_step, ego_corner, ego_hits, ego_first int32 [E]."""
        eg = self._ego_traces(ego_states)
        E, S = eg.shape[:2]
        v, off, vp, op, P = _lib.road_args(verts, poly_off)
        box = self._audit_box(ego_box, "ego_box")
        out, res = _lib.out_record(_lib.AuditRoadEpisodeOut, lambda k: (E, S) if k.startswith("step_") else (E,))
        rc = self.lib.mind_audit_road_episode(self.ctx, C.byref(box), vp, op, P, E, S, eg.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_road_episode")
        return res

    # ---- lane audit (mind_audit_lane_plan / mind_audit_lane_episode): outside every planning cycle ---------
    def audit_lane_plan(self, flats, xs, verts, lane_off, ego_box, cos_flow, bound, form=0):
        """Lane offset, heading and progress of C candidate state sets on every cost tree of ``flats`` in one call (mind_audit_lane_plan,
        k_lane_boxes): the ego box's centre at every trajectory node against the lane centrelines ``verts`` [V, 2] / ``lane_off`` [P + 1]
        (mind_amd.audit.Lanes).  ``xs``: [C, sum M, 6], or one [C, M_t, 6] per tree; ``parent`` and ``prob`` of the trees are read.
        ``cos_flow``: a segment goes the ego's way when the heading's cosine against it is at least this; ``bound``: a node further than this
        from every such segment is a hit; ``form``: the kernel's shape -- 0 = the library's rule, 1 = thread per box, 2 = one wavefront per
        box -- which changes no result.  Returns a dict: per-tree lists node_lat, node_s, node_along, node_across [2, C, M_t] / node_lane,
        node_edge int32 [2, C, M_t] (0 = any segment, 1 = with the flow), node_margin [C, M_t], and tree_min, tree_node, tree_lane, tree_hits,
        tree_first, tree_mass, tree_progress [C, n_trees]."""
        n = len(flats)
        keep = []
        trees, Ms = self._cost_trees(flats, None, keep)
        x = self._audit_xs(xs, int(sum(Ms)))
        for i, f in enumerate(flats):
            if np.shape(f["prob"]) != (Ms[i],):
                raise ValueError(f"cost tree {i}: prob [M] does not match parent [M = {Ms[i]}]")
        v, off, vp, op, P = _lib.lane_args(verts, lane_off)
        box, cfg = self._audit_box(ego_box, "ego_box"), _lib.lane_cfg(cos_flow, bound, form)
        nc, Mt = x.shape[0], x.shape[1]
        out, res = _lib.out_record(_lib.AuditLanePlanOut,
                                   lambda k: (nc, Mt) if k == "node_margin" else (2, nc, Mt) if k.startswith("node_") else (nc, n))
        rc = self.lib.mind_audit_lane_plan(self.ctx, C.byref(box), C.byref(cfg), vp, op, P, trees, n, nc, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_lane_plan")
        offs = np.cumsum([0] + list(Ms))
        for name in res:
            if name.startswith("node_"):
                res[name] = [res[name][..., offs[i]:offs[i + 1]].copy() for i in range(n)]
        return res

    def audit_lane_episode(self, ego_states, verts, lane_off, ego_box, cos_flow, bound, form=0):
        """Lane offset, heading and progress of E ego traces in one call (mind_audit_lane_episode, k_lane_boxes).  ``ego_states``: [E, S, 4]
        (or [S, 4]) = (x, y, v, yaw); the lanes and the configuration as ``audit_lane_plan`` takes them.  Returns a dict: step_lat, step_s,
        step_along, step_across [2, E, S] / step_lane, step_edge int32 [2, E, S] (0 = any segment, 1 = with the flow), step_margin [E, S],
        ego_min [E], ego_step, ego_lane, ego_hits, ego_first int32 [E], ego_progress, ego_back [E]."""
        eg = self._ego_traces(ego_states)
        E, S = eg.shape[:2]
        v, off, vp, op, P = _lib.lane_args(verts, lane_off)
        box, cfg = self._audit_box(ego_box, "ego_box"), _lib.lane_cfg(cos_flow, bound, form)
        out, res = _lib.out_record(_lib.AuditLaneEpisodeOut, lambda k: (E, S) if k == "step_margin" else (2, E, S) if k.startswith("step_") else (E,))
        rc = self.lib.mind_audit_lane_episode(self.ctx, C.byref(box), C.byref(cfg), vp, op, P, E, S, eg.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_audit_lane_episode")
        return res

    # ---- forecast scoring (mind_forecast_score): outside every planning cycle ------------------------------
    def forecast_score(self, reg, cls, actor_off, gt, valid, scored=None, horizons=(60,), miss_radius=2.0, disc_scale=1.0, disc_offset=0.0,
                       want=None):
        """Score a forecast against recorded futures in one call (mind_forecast_score, k_forecast_modes / k_forecast_scenes); the forecast
        never leaves the device.  ``reg`` [A, K, T, 5] / ``cls`` [B, K]: the device tensors ``predict()`` returns; ``actor_off`` [B + 1];
        ``gt`` [A, T, 2] float64 in the agents' local frames and ``valid`` [A, T] (mind_amd.forecast.ground_truth); ``scored`` [A] or None =
        all; ``horizons``: up to four ascending sample counts; ``disc_scale`` / ``disc_offset``: the disc max(sx, sy) * scale + offset.
        Returns a dict of numpy arrays: ade, fde, cover, first_out [A, n_h, K]; n_valid, last, k_ade, k_fde, brier_fde [A, n_h];
        s_n_scored, s_k_ade, s_k_fde, s_k_top, s_brier_fde, s_miss_rate, s_miss_top [B, n_h]; s_ade, s_fde [B, n_h, K]; and the values at the
        arg-minima min_ade, min_fde [A, n_h], s_min_ade, s_min_fde [B, n_h] (NaN for -1).  ``want``: names of the outputs to read back."""
        for t, name in ((reg, "reg"), (cls, "cls")):
            assert t.device == self.device and t.dtype == torch.float32, (name, t.device, t.dtype)
        if reg.dim() != 4 or reg.shape[3] != 5 or cls.dim() != 2 or cls.shape[1] != reg.shape[1]:
            raise ValueError(f"reg must be [A, K, T, 5] and cls [B, K], got {list(reg.shape)} and {list(cls.shape)}")
        reg, cls = reg.contiguous(), cls.contiguous()
        K, T = int(reg.shape[1]), int(reg.shape[2])
        cfg, B, off, g, v, sc, out, res, keep = _lib.forecast_args(K, T, actor_off, gt, valid, scored, horizons, miss_radius, disc_scale, disc_offset,
                                                                   want)
        if reg.shape[0] != int(keep[0][-1]) or cls.shape[0] != B:
            raise ValueError(f"reg holds {reg.shape[0]} agents and cls {cls.shape[0]} scenes, actor_off says {int(keep[0][-1])} and {B}")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() > 0 else None
        rc = self.lib.mind_forecast_score(self.ctx, C.byref(cfg), B, off, ptr(reg), ptr(cls), g, v, sc, C.byref(out))
        _lib.check(self.lib, self.ctx, rc, "mind_forecast_score")
        return _lib.forecast_gather(res)

    def aime_world(self, reg, vel, actor_ctrs, actor_vecs, a_off, rots, origs, cov_last, last, target_lane=None, cls=None,
                   scen_prob=None, dist_thres=None):
        """k7 on the device (mind_aime_world): reg [A,6,60,5] / vel [A,6,60,2] / actor_ctrs, actor_vecs [A,2] device
        tensors; a_off [B+1]; rots [B,2,2], origs [B,2], cov_last [A] host float32; last [B] int.
        target_lane [P,2] float32 (optional).  Returns device tensors world [A,6,60,6] (x,y,vx,vy,heading,max-sigma),
        topo [A,6], ego_end [B,6,4] (ego x, y, max-sigma at step `last`, distance of that point to the target lane).
        With ``cls`` [B,6] (device) and ``scen_prob`` [B] the pruning decisions are taken on the device as well (k_aime_select):
        ``sel`` [2,B,6] = (mode index or -1, path probability) of the kept modes in visiting order; ``dist_thres`` switches the
        target-lane test on (needs target_lane and last >= 0 everywhere)."""
        dev = self.device
        B, A = len(a_off) - 1, int(a_off[-1])
        for t_ in (reg, vel, actor_ctrs, actor_vecs):
            assert t_.device == dev and t_.dtype == torch.float32 and t_.is_contiguous()
        assert reg.shape == (A, 6, 60, 5) and vel.shape == (A, 6, 60, 2) and actor_ctrs.shape == (A, 2)
        wi, wo = _lib.WorldIn(), _lib.WorldOut()
        ao = (C.c_int32 * (B + 1))(*[int(v) for v in a_off])
        rot = np.ascontiguousarray(rots, np.float32).reshape(B, 4)
        org = np.ascontiguousarray(origs, np.float32).reshape(B, 2)
        cvl = np.ascontiguousarray(cov_last, np.float32).reshape(A)
        lst = np.ascontiguousarray(last, np.int32).reshape(B)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        wi.n_scenes, wi.actor_off = B, ao
        wi.reg, wi.vel = C.c_void_p(reg.data_ptr()), C.c_void_p(vel.data_ptr())
        wi.actor_ctrs, wi.actor_vecs = C.c_void_p(actor_ctrs.data_ptr()), C.c_void_p(actor_vecs.data_ptr())
        wi.rot, wi.orig, wi.cov_last = fp(rot), fp(org), fp(cvl)
        wi.last = lst.ctypes.data_as(C.POINTER(C.c_int32))
        if target_lane is not None:
            tl = np.ascontiguousarray(target_lane, np.float32).reshape(-1, 2)
            wi.target_lane, wi.n_lane_pts = fp(tl), len(tl)
        # topo and ego_end live in one buffer behind a copy of cls, so that the host fetches all three with one copy
        if cls is not None and scen_prob is not None:
            small = torch.empty(B * 6 + A * 6 + B * 24, device=dev)     # the host only reads `sel`
        else:
            small = torch.zeros(B * 6 + A * 6 + B * 24, device=dev)
            if cls is not None:
                small[:B * 6] = cls.reshape(-1)
        out = dict(world=torch.empty(A, 6, 60, 6, device=dev), small=small, topo=small[B * 6:B * 6 + A * 6].view(A, 6),
                   ego_end=small[B * 6 + A * 6:].view(B, 6, 4))
        wo.world, wo.topo, wo.ego_end = (C.c_void_p(out[k].data_ptr()) for k in ("world", "topo", "ego_end"))
        if cls is not None and scen_prob is not None:
            cls = cls.contiguous()
            assert cls.device == dev and cls.dtype == torch.float32 and cls.numel() == B * 6
            out["_cls"] = cls                       # keeps the (possibly fresh) buffer alive until the kernel ran
            sp = np.ascontiguousarray(scen_prob, np.float32).reshape(B)
            out["sel"] = torch.empty(2, B, 6, device=dev)
            wi.cls, wi.scen_prob = C.c_void_p(cls.data_ptr()), fp(sp)
            wi.lane_check = int(dist_thres is not None)
            wi.dist_thres = float(dist_thres) if dist_thres is not None else 0.0
            wo.sel, wo.sel_prob = C.c_void_p(out["sel"][0].data_ptr()), C.c_void_p(out["sel"][1].data_ptr())
        rc = self.lib.mind_aime_world(self.ctx, C.byref(wi), C.byref(wo))
        _lib.check(self.lib, self.ctx, rc, "mind_aime_world")
        return out

    def aime_decide(self, a_off, cmp, cls, scen_prob, topo, ego_end, world, dist_thres=None, prob_floor=0.001, fused=True, by_value=False):
        """The decision kernels of an AIME round on given inputs (mind_debug_aime_decide; tests).  a_off [B+1], cmp [B] int, scen_prob [B]:
        host; cls [B,6], topo [A,6], ego_end [B,6,4], world [A,6,60,6]: device float32 tensors or host arrays (uploaded here).  ``dist_thres``
        switches the target-lane test on.  Returns host arrays sel [B,6] (kept mode or -1), sel_prob [B,6] float32, hit [B,6,2] uint32."""
        dev = self.device
        B, A = len(a_off) - 1, int(a_off[-1])
        up = lambda x: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
        cls, topo, ego_end, world = up(cls), up(topo), up(ego_end), up(world)
        for t_, n in ((cls, B * 6), (topo, A * 6), (ego_end, B * 24), (world, A * 6 * 60 * 6)):
            assert t_.device == dev and t_.dtype == torch.float32 and t_.is_contiguous() and t_.numel() == n
        ao = np.ascontiguousarray(a_off, np.int32)
        cm = np.ascontiguousarray(cmp, np.int32).reshape(B)
        sp = np.ascontiguousarray(scen_prob, np.float32).reshape(B)
        sel = torch.empty(2, B, 6, device=dev)
        hit = torch.zeros(B, 6, 2, dtype=torch.int32, device=dev)
        ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        rc = self.lib.mind_debug_aime_decide(self.ctx, B, ip(ao), ip(cm), C.c_void_p(cls.data_ptr()), sp.ctypes.data_as(C.POINTER(C.c_float)),
                                             C.c_void_p(topo.data_ptr()), C.c_void_p(ego_end.data_ptr()), C.c_void_p(world.data_ptr()),
                                             int(dist_thres is not None), float(dist_thres) if dist_thres is not None else 0.0, float(prob_floor),
                                             int(bool(fused)), int(bool(by_value)), C.c_void_p(sel[0].data_ptr()), C.c_void_p(sel[1].data_ptr()),
                                             C.c_void_p(hit.data_ptr()))
        _lib.check(self.lib, self.ctx, rc, "mind_debug_aime_decide")
        s = sel.cpu().numpy()
        return s[0].astype(np.int64), s[1], hit.cpu().numpy().view(np.uint32)

    def aime_rebase(self, pos, ang, vel, types, lane_ctrs, lane_vecs, target_lane, target_lane_info, pad=None,
                    time_ahead=5.0, min_vel=0.5, dev_src=None):
        """update_obser for S child scenes on the device (mind_aime_rebase).  pos [S,a,50,2], ang [S,a,50], vel [S,a,50,2]
        (world-frame windows), types [a,50,7], lane_ctrs / lane_vecs [l,2], target_lane [P,2], target_lane_info [P,12]: host
        float32.  Returns device tensors actors [S*a,14,48], actor_ctrs, actor_vecs [S*a,2], lane_ctrs, lane_vecs [S*l,2],
        tgt_nodes [S,10,16], tgt_rpe [S,20], frames [S,28] (ROT, ORIG, TGT_PTS) and ``gen``, the call's generation.
        ``dev_src`` = dict(rows=device [R,60,6], parent_slot, row0, dur: int [S], gen, a): the windows are assembled on the device
        from the parents' windows of the previous call (generation ``gen``) and the kept rows; pos / ang / vel are ignored."""
        dev = self.device
        f = lambda x: np.ascontiguousarray(x, np.float32)
        types = f(types)
        lane_ctrs, lane_vecs, tl, ti = f(lane_ctrs), f(lane_vecs), f(target_lane), f(target_lane_info)
        ri, ro = _lib.RebaseIn(), _lib.RebaseOut()
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
        keep = []
        if dev_src is not None:
            rows = dev_src["rows"]
            assert rows.device == dev and rows.dtype == torch.float32 and rows.is_contiguous() and tuple(rows.shape[1:]) == (60, 6)
            ps, r0, du = (np.ascontiguousarray(dev_src[k], np.int32) for k in ("parent_slot", "row0", "dur"))
            S, a = len(ps), int(dev_src["a"])
            assert len(r0) == S and len(du) == S and int(r0.max()) + a <= rows.shape[0]
            ri.rows_dev, ri.parent_slot, ri.row0, ri.dur, ri.prev_gen = C.c_void_p(rows.data_ptr()), ip(ps), ip(r0), ip(du), int(dev_src["gen"])
            keep += [ps, r0, du, rows]
        else:
            # lists of per-scene windows are stacked here (page-locked staging buffers were measured slower than the runtime's own
            # pageable path: 15 vs 10 ms per plan at 216 scenes x 64 agents)
            stk = lambda x: f(np.stack(x) if isinstance(x, (list, tuple)) else x)
            pos, ang, vel = stk(pos), stk(ang), stk(vel)
            S, a = pos.shape[:2]
            assert pos.shape == (S, a, 50, 2) and ang.shape == (S, a, 50) and vel.shape == (S, a, 50, 2)
            ri.pos, ri.ang, ri.vel = fp(pos), fp(ang), fp(vel)
        l = lane_ctrs.shape[0]
        assert types.shape == (a, 50, 7) and tl.ndim == 2 and ti.shape == (len(tl), 12)
        ri.n_scenes, ri.n_agents, ri.n_lanes = S, a, l
        ri.types = fp(types)
        padk = None
        if pad is not None:
            padk = f(pad)
            ri.pad = fp(padk)
        ri.lane_ctrs, ri.lane_vecs, ri.target_lane, ri.target_lane_info, ri.n_lane_pts = fp(lane_ctrs), fp(lane_vecs), fp(tl), fp(ti), len(tl)
        ri.time_ahead, ri.min_vel = float(time_ahead), float(min_vel)
        out = dict(actors=torch.empty(S * a, 14, 48, device=dev), actor_ctrs=torch.empty(S * a, 2, device=dev),
                   actor_vecs=torch.empty(S * a, 2, device=dev), lane_ctrs=torch.empty(S * l, 2, device=dev),
                   lane_vecs=torch.empty(S * l, 2, device=dev), tgt_nodes=torch.empty(S, 10, 16, device=dev),
                   tgt_rpe=torch.empty(S, 20, device=dev), frames=torch.empty(S, 28, device=dev))
        for k in out:
            setattr(ro, k, C.c_void_p(out[k].data_ptr()))
        gen = C.c_int32(0)
        ro.gen = C.pointer(gen)
        rc = self.lib.mind_aime_rebase(self.ctx, C.byref(ri), C.byref(ro))
        _lib.check(self.lib, self.ctx, rc, "mind_aime_rebase")
        out["gen"] = self._rebase_gen = int(gen.value)      # the arena of THIS call is what a device-source call can build on next
        return out

    def aime_plan(self, root, hist, lane_ctrs, lane_vecs, target_lane, target_lane_info, time_ahead, dist_thres, max_depth,
                  pred_len=50, min_vel=0.5, max_rounds=16, raw=None, script=None, prob_floor=None, solve=None):
        """ScenarioTreeGenerator.branch_aime in one call (mind_aime_plan).  Host-built root: ``root`` = the root scene dict of
        process_data (ACTORS, TRAJS_CTRS, TRAJS_VECS, LANES, TGT_NODES, TGT_RPE, ROT, ORIG, TGT_PTS, TRAJS_TYPE), ``hist`` [a,50,6] its
        world-frame history (x, y, vx, vy, heading, max-sigma), lane_ctrs / lane_vecs the lane graph's anchors.  Device-built root:
        ``raw`` = dict(pos [a,50,2], ang [a,50], vel [a,50,2], pad [a,50], types [a,50,7] as get_agent_trajectories returns them,
        lane_pts [l,11,2] float64, lane_flags [l,6] int, travel0) and root / hist / lane_ctrs / lane_vecs are ignored.
        Returns (nodes: structured array, one record per internal tree node in creation order, rows: float32 [n], info dict) or None
        when the library reports a situation only the round-by-round path handles.  ``script``: see mind_aime_plan_in.script_cls."""
        pi, keep, a, l = self._aime_plan_args(root, hist, lane_ctrs, lane_vecs, target_lane, target_lane_info, time_ahead, dist_thres, max_depth,
                                              pred_len, min_vel, max_rounds, raw, script, prob_floor, solve)
        po = _lib.AimePlanOut()
        rc = self.lib.mind_aime_plan(self.ctx, C.byref(pi), C.byref(po))
        return self._aime_plan_result(rc, po, a, l)

    def aime_plan_begin(self, *args, **kw):
        """aime_plan in two halves (mind_aime_plan_begin / _finish: the plan runs on a thread of the library, this call returns at once):
        same arguments as aime_plan; aime_plan_ready() tells whether aime_plan_finish() would block."""
        pi, keep, a, l = self._aime_plan_args(*args, **kw)
        rc = self.lib.mind_aime_plan_begin(self.ctx, C.byref(pi))
        _lib.check(self.lib, self.ctx, rc, "mind_aime_plan_begin")
        self._aime_pending = (pi, keep, a, l)         # (the input arrays stay alive until the plan is collected)

    def aime_plan_ready(self):
        return self.lib.mind_aime_plan_poll(self.ctx) == 0

    def aime_plan_finish(self):
        pi, keep, a, l = self._aime_pending
        self._aime_pending = None
        po = _lib.AimePlanOut()
        rc = self.lib.mind_aime_plan_finish(self.ctx, C.byref(po))
        return self._aime_plan_result(rc, po, a, l)

    def busy(self):
        """work queued on this context (a begun plan, begun contingency solves) has not completed yet"""
        rc = self.lib.mind_ctx_busy(self.ctx)
        if rc < 0:
            _lib.check(self.lib, self.ctx, rc, "mind_ctx_busy")
        return rc == 1

    def _aime_plan_args(self, root, hist, lane_ctrs, lane_vecs, target_lane, target_lane_info, time_ahead, dist_thres, max_depth,
                        pred_len=50, min_vel=0.5, max_rounds=16, raw=None, script=None, prob_floor=None, solve=None):
        f = lambda x: np.ascontiguousarray(x, np.float32)
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        pi = _lib.AimePlanIn()
        keep = []
        if raw is not None:
            arrs = dict(raw_pos=f(raw["pos"]), raw_ang=f(raw["ang"]), raw_vel=f(raw["vel"]), raw_pad=f(raw["pad"]), types=f(raw["types"]),
                        target_lane=f(target_lane), target_lane_info=f(target_lane_info))
            lpts = np.ascontiguousarray(raw["lane_pts"], np.float64)
            lfl = np.ascontiguousarray(raw["lane_flags"], np.int32)
            a, l, P = arrs["raw_pos"].shape[0], lpts.shape[0], arrs["target_lane"].shape[0]
            assert arrs["raw_pos"].shape == (a, 50, 2) and arrs["raw_ang"].shape == (a, 50) and arrs["raw_pad"].shape == (a, 50)
            assert arrs["types"].shape == (a, 50, 7) and lpts.shape == (l, 11, 2) and lfl.shape == (l, 6)
            pi.lane_pts, pi.lane_flags = lpts.ctypes.data_as(C.POINTER(C.c_double)), lfl.ctypes.data_as(C.POINTER(C.c_int32))
            pi.travel0 = float(raw["travel0"])
            keep += [lpts, lfl]
        else:
            arrs = dict(actors=f(root["ACTORS"]), actor_ctrs=f(root["TRAJS_CTRS"]), actor_vecs=f(root["TRAJS_VECS"]), lanes=f(root["LANES"]),
                        lane_ctrs=f(lane_ctrs), lane_vecs=f(lane_vecs), tgt_nodes=f(root["TGT_NODES"]), tgt_rpe=f(root["TGT_RPE"]),
                        rot=f(root["ROT"]), orig=f(root["ORIG"]), tgt_pts=f(root["TGT_PTS"]), hist=f(hist), types=f(root["TRAJS_TYPE"]),
                        target_lane=f(target_lane), target_lane_info=f(target_lane_info))
            a, l, P = arrs["actors"].shape[0], arrs["lanes"].shape[0], arrs["target_lane"].shape[0]
            assert arrs["actors"].shape == (a, 14, 48) and arrs["hist"].shape == (a, 50, 6) and arrs["types"].shape == (a, 50, 7)
            assert arrs["lanes"].shape == (l, 10, 16) and arrs["lane_ctrs"].shape == (l, 2)
        assert arrs["target_lane_info"].shape == (P, 12)
        pi.n_agents, pi.n_lanes, pi.n_lane_pts = a, l, P
        for k, v in arrs.items():
            setattr(pi, k, fp(v))
        pi.time_ahead, pi.min_vel, pi.dist_thres = float(time_ahead), float(min_vel), float(dist_thres)
        pi.max_depth, pi.max_rounds, pi.pred_len = int(max_depth), int(max_rounds), int(pred_len)
        pi.prob_floor = 0.0 if prob_floor is None else float(prob_floor)      # (0 = the reference's 0.001)
        if script is not None:        # (cls [1,6], reg [a,6,60,5], vel [a,6,60,2]) float32 device tensors: scripted modes (synth.ScriptedBranching)
            sc, sr, sv = script
            assert tuple(sr.shape) == (a, 6, 60, 5) and tuple(sv.shape) == (a, 6, 60, 2) and sc.numel() == 6
            assert all(t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 for t in script)
            pi.script_cls, pi.script_reg, pi.script_vel = sc.data_ptr(), sr.data_ptr(), sv.data_ptr()
            keep += list(script)
        if solve is not None:         # (cfg_warm, cfg_full, x0 [6], lane [P,2], target velocity): the plan begins its contingency solves itself
            cw, cf, x0, lane_s, tv = solve
            x0 = np.ascontiguousarray(x0, np.float64)
            lane_s = np.ascontiguousarray(lane_s, np.float64)
            pi.solve_cfg_warm, pi.solve_cfg_full = C.addressof(cw), C.addressof(cf)
            pi.solve_x0, pi.solve_lane, pi.solve_n_lane_pts, pi.solve_target_vel = x0.ctypes.data, lane_s.ctypes.data, len(lane_s), float(tv)
            keep += [cw, cf, x0, lane_s]
        keep.append(arrs)
        return pi, keep, a, l

    def _aime_plan_result(self, rc, po, a, l):
        if rc == _lib.MIND_ESTATE:
            msg = self.lib.mind_last_error_string(self.ctx) or b""
            if msg.startswith(b"unsupported"):
                self.last_aime_fallback = msg.decode()
                return None
        _lib.check(self.lib, self.ctx, rc, "mind_aime_plan")
        n = po.n_nodes
        nodes = np.frombuffer(C.string_at(po.nodes, n * C.sizeof(_lib.AimeNode)), dtype=AIME_NODE_DTYPE) if n else np.zeros(0, AIME_NODE_DTYPE)
        nf = int(po.n_row_floats)
        rows = np.frombuffer(C.string_at(po.rows, nf * 4), dtype=np.float32) if nf else np.zeros(0, np.float32)
        # the flattened cost trees (what flatten_scenario_tree builds from the returned scenario trees), one dict per scenario tree
        flats, nt = [], po.n_trees
        if nt:
            off = np.frombuffer(C.string_at(po.tree_off, (nt + 1) * 4), dtype=np.int32)
            top = np.frombuffer(C.string_at(po.tree_top, nt * 4), dtype=np.int32)
            Mt = int(off[-1])
            par = np.frombuffer(C.string_at(po.flat_parent, Mt * 4), dtype=np.int32)
            prob = np.frombuffer(C.string_at(po.flat_prob, Mt * 4), dtype=np.float32)
            mean = np.frombuffer(C.string_at(po.flat_mean, Mt * a * 8), dtype=np.float32).reshape(Mt, a, 2)
            cov = np.frombuffer(C.string_at(po.flat_cov, Mt * a * 4), dtype=np.float32).reshape(Mt, a)
            for t in range(nt):
                lo, hi = int(off[t]), int(off[t + 1])
                flats.append((int(top[t]), dict(parent=par[lo:hi], prob=prob[lo:hi], mean=mean[lo:hi], cov=cov[lo:hi])))
        info = dict(n_expanded=po.n_expanded, n_rounds=po.n_rounds, root_flags=po.root_flags, a=a, l=l, flats=flats,
                    round_scenes=[po.round_scenes[i] for i in range(po.n_rounds)], pair_ms=po.pair_ms, pair_launches=po.pair_launches,
                    solves_begun=bool(po.solves_begun))
        self.last_aime_info = info
        return nodes, rows, info

    def lane_dist_field(self, ego_xy, lane, W, H, res):
        """gen_dist_field (ilqr/utils.py:5-22) -> (offset [2], gx [W], gy [H], dist [H,W])."""
        ego = np.ascontiguousarray(np.asarray(ego_xy, np.float64)[:2])
        lane = np.ascontiguousarray(lane, np.float64)
        off, gx, gy, dist = np.zeros(2), np.zeros(W), np.zeros(H), np.zeros((H, W))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc = self.lib.mind_lane_dist_field(self.ctx, dp(ego), dp(lane), len(lane), int(W), int(H), C.c_double(float(res)),
                                           dp(off), dp(gx), dp(gy), dp(dist))
        _lib.check(self.lib, self.ctx, rc, "mind_lane_dist_field")
        return off, gx, gy, dist

    def predict_numpy_batch(self, pb, use_rpe=False, **kw):
        """Convenience for tests: ``pb`` as produced by ``mind_amd.synth.predictor_batch`` (numpy)."""
        dev = self.device
        B = len(pb["ACTOR_IDCS"])
        a_off = [0] + list(np.cumsum([len(x) for x in pb["ACTOR_IDCS"]]))
        l_off = [0] + list(np.cumsum([len(x) for x in pb["LANE_IDCS"]]))
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        actr = np.concatenate([pb["CTRS"][b][:a_off[b + 1] - a_off[b]] for b in range(B)])
        avec = np.concatenate([pb["VECS"][b][:a_off[b + 1] - a_off[b]] for b in range(B)])
        lctr = np.concatenate([pb["CTRS"][b][a_off[b + 1] - a_off[b]:] for b in range(B)])
        lvec = np.concatenate([pb["VECS"][b][a_off[b + 1] - a_off[b]:] for b in range(B)])
        rpe = None
        if use_rpe:
            rpe = [t(r) for r in pb["RPE"]]
        return self.predict(t(pb["ACTORS"]), a_off, t(pb["LANES"]), l_off, t(actr), t(avec), t(lctr), t(lvec),
                            t(pb["TGT_NODES"]), t(pb["TGT_RPE"]), rpe=rpe, **kw)
