"""What the clearance audit's device calls cost: device events on the context's stream around each call (upload, kernels, read-back), after a
warm-up call, median of `--reps`:

  plan     HipPredictor.audit_plan (mind_audit_plan) with `--cands` candidate state sets on the scripted branch3 tree (70 nodes, 12 agents)
  episode  HipPredictor.audit_episode (mind_audit_episode) on the recorded demo_1 scene (546 steps x 40 tracks) with 1 and 64 ego traces

The candidates are the states of a six-iteration solve shifted rigidly by a centimetre per copy, the further ego traces likewise; the first
copy's results must equal the host evaluation of the same header (mind_debug_box_clearance + the rules of tests/box_geom_restate.py).

  python tools/audit_rate.py [--cands 4096] [--reps 20] [--out profiles/audit_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    """median / min / max ms of fn() between two events on the current stream (the context's), after one warm-up call"""
    import torch
    fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms))), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audit_rate.json"))
    args = ap.parse_args()
    import audit_cases as ac
    from mind_amd.runtime import get_runtime
    from mind_amd.synth import scripted_scenario_tree
    from oracle import ilqr as oi
    rt = get_runtime()
    sst = scripted_scenario_tree("branch3", 12)
    flat = oi.flatten(sst["nodes"])
    xs0 = rt.ilqr_solve(oi.default_cfg(max_iter=6), [flat], oi.init_state(sst["state"], sst["ctrl"]), sst["target_lane"], sst["target_vel"], 1)[0][0]
    xs = np.stack([xs0] * args.cands)
    xs[:, :, 0] += 0.01 * np.arange(args.cands)[:, None]
    out = {"reps": args.reps}
    t, res = timed(lambda: rt.audit_plan([flat], [xs], ac.EGO_BOX, 2.5), args.reps)
    want = ac.host_plan([flat], [xs[:1]])
    same = all(np.array_equal(res[k][0][0] if k.startswith("node_") else res[k][0], want[k][0][0] if k.startswith("node_") else want[k][0]) for k in want)
    out["plan"] = dict(t, candidates=args.cands, nodes=len(flat["parent"]), agents=int(flat["cov"].shape[1]), same_as_host=bool(same))
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_1")
    for n_ego in (1, 64):
        egos = np.stack([ego + np.array([0.01 * k, 0.0, 0.0, 0.0]) for k in range(n_ego)])
        t, res = timed(lambda: rt.audit_episode(egos, exo, valid, boxes, ac.EGO_BOX), args.reps)
        want = ac.host_episode(egos[:1], exo, valid, boxes)
        ok = all(np.array_equal(res[k][:1], want[k]) for k in want)
        same = same and ok
        out[f"episode_{n_ego}"] = dict(t, n_ego=n_ego, steps=int(exo.shape[0]), tracks=int(exo.shape[1]), same_as_host=bool(ok))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
