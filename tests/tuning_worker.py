"""Child process of tests/test_gpu_tuning.py, one mode per test (argv[1]); prints one JSON line.
  knobs       a context created under the caller's MIND_* variables: every knob read with mind_get_tuning, then set to each int of argv[2]
              (JSON list) and read back, what get and set answer to an unknown name.  Launches no kernel.
  handles     mind_debug_live_handles around contexts that predict, solve, audit and plan, around one destroyed at once and around one
              destroyed with a begun tree-iLQR call pending
  background  the "ilqr_wgs" switch of a background solve (HipPredictor.ilqr_background) and the bits of the solves around it"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mind_amd import _lib, runtime                    # noqa: E402
from mind_amd.predictor import HipPredictor, IlqrCall  # noqa: E402
from mind_amd.synth import predictor_batch, scripted_scenario_tree  # noqa: E402
from oracle import ilqr as oi                          # noqa: E402


def lead_tree():
    sst = scripted_scenario_tree("lead", 4)
    return oi.flatten(sst["nodes"]), oi.init_state(sst["state"], sst["ctrl"]), sst["target_lane"], sst["target_vel"]


def contingency(hp, max_iter=20):
    flat, x0, lane, tv = lead_tree()
    return IlqrCall(hp.lib, oi.default_cfg(max_iter=max_iter), [flat], x0, lane, tv, cfg_full=oi.default_cfg(max_iter=max_iter))


def knobs(values):
    hp = HipPredictor(0)
    names = [k for k, _, _ in _lib.knobs()]
    out = dict(created={k: hp.get_tuning(k) for k in names}, pair_prec=hp.pair_precision(), set={})
    for v in values:
        for k in names:
            hp.set_tuning(k, v)
        out["set"][str(v)] = {k: hp.get_tuning(k) for k in names}
    import ctypes as C
    got = C.c_int(-77)
    out["unknown_set"] = [hp.lib.mind_set_tuning(hp.ctx, b"no_such_knob", 1), hp.lib.mind_last_error_string(hp.ctx).decode()]
    out["unknown_get"] = [hp.lib.mind_get_tuning(hp.ctx, b"no_such_knob", C.byref(got)), hp.lib.mind_last_error_string(hp.ctx).decode(), got.value]
    hp.close()
    return out


def handles():
    import audit_cases as ac
    from bench import WORKLOADS, make_closed_loop
    os.environ["MIND_NATIVE_PLAN"] = "0"               # the planner's Python steps: its plan is one mind_aime_plan on the thread's context, no mind_planner
    live = _lib.load().mind_debug_live_handles
    out = dict(base=live(), used=[], after=[])
    for _ in range(2):
        # everything on the thread's context: the planner's predictor and solver share it
        pl, sim, _w = make_closed_loop(dict(WORKLOADS["demo1"]), speculative=False)
        hp = runtime.get_runtime()
        assert pl.network.rt is hp
        hp.set_profiling(True)
        hp.predict_numpy_batch(predictor_batch(6, 10, 2, seed=1))
        xs = contingency(hp).run(hp).finish()[0]
        flat = lead_tree()[0]
        hp.audit_plan([flat], [xs[0][None]], ac.EGO_BOX, 2.5)
        sim.run_plans(1)                                # mind_aime_plan and the contingency solves of its trees
        assert pl.scen_tree_gen.n_native_plans == 1
        out["used"].append(live())
        runtime.reset_runtime()
        out["after"].append(live())
        del pl, sim
    hp = HipPredictor(0)
    out["fresh"] = live()
    hp.close()
    out["after_fresh"] = live()
    hp = HipPredictor(0)
    call = contingency(hp).begin(hp)
    assert call.rc == 0
    out["pending"] = live()
    hp.close()                                          # (never collected)
    out["after_pending"] = live()
    return out


def background():
    flat, x0, lane, tv = lead_tree()
    cfg = oi.default_cfg(max_iter=20)
    digest = lambda call: hashlib.sha256(call.xs.tobytes() + call.us.tobytes()).hexdigest()
    warm = lambda bg: IlqrCall(_lib.load(), cfg, [flat], x0, lane, tv, use_exo=0, background=bg)
    hp, out = HipPredictor(0), dict(wgs=[], got=[], want=[])
    hp.set_tuning("ilqr_wgs", 8)
    steps = []
    steps.append(warm(True).run(hp));                     out["wgs"].append(hp.get_tuning("ilqr_wgs"))      # 1
    steps.append(contingency(hp).begin(hp).wait());       out["wgs"].append(hp.get_tuning("ilqr_wgs"))      # 8
    steps.append(warm(True).run(hp));                     out["wgs"].append(hp.get_tuning("ilqr_wgs"))      # 1
    hp.set_tuning("ilqr_wgs", 4);                         out["wgs"].append(hp.get_tuning("ilqr_wgs"))      # 4: the user's
    steps.append(contingency(hp).begin(hp).wait());       out["wgs"].append(hp.get_tuning("ilqr_wgs"))      # 4
    steps.append(warm(False).run(hp));                    out["wgs"].append(hp.get_tuning("ilqr_wgs"))      # 4
    for c in steps:
        c.finish()
    out["got"] = [digest(c) for c in steps]
    hp.close()
    ref = HipPredictor(0)           # never switched
    ref.set_tuning("ilqr_wgs", 8)
    for c in (warm(False).run(ref), contingency(ref).begin(ref).wait()):
        c.finish()
        out["want"].append(digest(c))
    out["ref_wgs"] = ref.get_tuning("ilqr_wgs")
    ref.close()
    return out


if __name__ == "__main__":
    mode = sys.argv[1]
    print(json.dumps(knobs(json.loads(sys.argv[2])) if mode == "knobs" else handles() if mode == "handles" else background()))
