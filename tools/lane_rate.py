"""What the lane audit's device calls cost in the two forms of k_lane_boxes, next to the road audit at the same rows from the same run: device
events on the context's stream around each call (upload, kernels, read-back), after a warm-up call, median of `--reps`:

  form1  HipPredictor.audit_lane_episode / audit_lane_plan with form = 1: k_lane_boxes<1>, a workgroup = 256 boxes, thread = box
  form2  the same with form = 2: k_lane_boxes<2>, one wavefront per box, its lanes over the segments
  road   HipPredictor.audit_road_episode / audit_road_plan (k_road_boxes) against the demo_1 drivable area

against the demo_1 lanes (21 lanes, 1 395 vertices): the recorded trace (1 x 546 rows) and 8, 64 and 512 copies of it, and 64, 512, 4 096 and
14 000 candidate state sets on the scripted branch3 tree (70 nodes), their nodes placed on the recorded trace.  The further copies are shifted
by a centimetre each.  The two forms must agree bit for bit, and the first trace's / candidate's results must equal the host evaluation of
the same header (mind_debug_lane_project + the rules of tests/lane_geom_restate.py).

  python tools/lane_rate.py [--reps 20] [--out profiles/lane_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audit_rate import timed  # noqa: E402

EPISODES = (1, 8, 64, 512)
PLANS = (64, 512, 4096, 14000)


def _equal(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype == np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lane_rate.json"))
    args = ap.parse_args()
    import audit_cases as ac
    import ilqr_policy_restate as pr
    import lane_cases as lc
    import road_cases as rc
    from mind_amd.runtime import get_runtime
    rt = get_runtime()
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_1")
    lanes, road = lc.demo_lanes("demo_1"), rc.demo_road("demo_1")
    out, same = {"reps": args.reps, "lanes": int(lanes.n_lanes), "vertices": int(len(lanes.verts)), "road_vertices": int(len(road.verts))}, True
    lane_ep = lambda e, form: rt.audit_lane_episode(e, lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, lc.BOUND, form)
    for n_ego in EPISODES:
        egos = np.stack([ego + np.array([0.01 * k, 0.0, 0.0, 0.0]) for k in range(n_ego)])
        calls = dict(form1=lambda: lane_ep(egos, 1), form2=lambda: lane_ep(egos, 2), road=lambda: rt.audit_road_episode(egos, road.verts, road.poly_off, lc.EGO_BOX))
        row, res = dict(kind="episode", n_ego=n_ego, steps=len(ego), rows=n_ego * len(ego)), {}
        for name, fn in calls.items():
            row[name], res[name] = timed(fn, args.reps)
        want = lc.host_episode(egos[:1], lanes)
        ok = all(_equal(res["form1"][k], res["form2"][k]) for k in want) and all(_equal(res["form2"][k][..., :1, :] if k.startswith("step_") else res["form2"][k][:1], want[k]) for k in want)
        row["forms_agree_and_same_as_host"] = bool(ok)
        same = same and ok
        out[f"episode_{n_ego}x{len(ego)}"] = row
        print(f"episode {n_ego:5d} x {len(ego)}: form 1 {row['form1']['median_ms']:.3f} ms, form 2 {row['form2']['median_ms']:.3f} ms, road {row['road']['median_ms']:.3f} ms, same {ok}",
              flush=True)
    flat = pr.scene("branch3", 12)["flat"]
    M = len(flat["parent"])
    lane_pl = lambda x, form: rt.audit_lane_plan([flat], [x], lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, lc.BOUND, form)
    for n_cand in PLANS:
        xs = np.zeros((n_cand, M, 6))
        pick = (7 * np.arange(M)[None, :] + np.arange(n_cand)[:, None]) % len(ego)
        xs[:, :, [0, 1, 2, 3]] = ego[pick]
        xs[:, :, 0] += 0.01 * (np.arange(n_cand) // len(ego))[:, None]
        calls = dict(form1=lambda: lane_pl(xs, 1), form2=lambda: lane_pl(xs, 2), road=lambda: rt.audit_road_plan([flat], [xs], road.verts, road.poly_off, lc.EGO_BOX))
        row, res = dict(kind="plan", n_cand=n_cand, nodes=M, rows=n_cand * M), {}
        for name, fn in calls.items():
            row[name], res[name] = timed(fn, args.reps)
        want = lc.host_plan([flat], [xs[:1]], lanes)
        first = lambda r, k: r[k][0][..., :1, :] if k.startswith("node_") else r[k][:1]
        ok = all(_equal(res["form1"][k][0], res["form2"][k][0]) if k.startswith("node_") else _equal(res["form1"][k], res["form2"][k]) for k in want)
        ok = ok and all(_equal(first(res["form2"], k), want[k][0] if k.startswith("node_") else want[k]) for k in want)
        row["forms_agree_and_same_as_host"] = bool(ok)
        same = same and ok
        out[f"plan_{n_cand}x{M}"] = row
        print(f"plan {n_cand:5d} x {M}: form 1 {row['form1']['median_ms']:.3f} ms, form 2 {row['form2']['median_ms']:.3f} ms, road {row['road']['median_ms']:.3f} ms, same {ok}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
