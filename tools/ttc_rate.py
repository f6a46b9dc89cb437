"""What the time-to-collision audit's device call costs in its two lane layouts, next to the clearance audit at the same shapes from the same
run: device events on the context's stream around each call (upload, kernels, read-back), after a warm-up call, median of `--reps`:

  ttc_lanes1  HipPredictor.audit_ttc (mind_audit_ttc) with lanes = 1: k_audit_ttc<1>, a workgroup = (step, 64 egos), thread = ego
  ttc_lanes2  the same with lanes = 2: k_audit_ttc<2>, one wavefront per (step, ego), its lanes over the tracks
  episode     HipPredictor.audit_episode (mind_audit_episode, k_audit_episode)

on the recorded demo_1 scene (546 steps x 40 tracks) with 1, 8, 16, 32 and 64 ego traces, and on its first 100 steps with 4 096.  The further
traces are the recorded one shifted by a centimetre per copy.  The two layouts must agree bit for bit, and the first trace's results must
equal the host evaluation of the same header (mind_debug_box_ttc + the rules of tests/ttc_geom_restate.py).

  python tools/ttc_rate.py [--reps 20] [--out profiles/ttc_rate.json]
  python tools/ttc_rate.py --once          every (shape, layout) once after a warm-up and nothing written: for a kernel trace
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

SHAPES = ((1, 546), (8, 546), (16, 546), (32, 546), (64, 546), (4096, 100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ttc_rate.json"))
    args = ap.parse_args()
    import audit_cases as ac
    import ttc_cases as tc
    from mind_amd.runtime import get_runtime
    rt = get_runtime()
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_1")
    out, same = {"reps": args.reps, "tracks": int(exo.shape[1])}, True
    for n_ego, S in SHAPES:
        egos = np.stack([ego[:S] + np.array([0.01 * k, 0.0, 0.0, 0.0]) for k in range(n_ego)])
        ex, va = exo[:S], valid[:S]
        calls = dict(ttc_lanes1=lambda: rt.audit_ttc(egos, ex, va, boxes, tc.EGO_BOX, lanes=1), ttc_lanes2=lambda: rt.audit_ttc(egos, ex, va, boxes, tc.EGO_BOX, lanes=2),
                     episode=lambda: rt.audit_episode(egos, ex, va, boxes, tc.EGO_BOX))
        if args.once:
            for fn in calls.values():
                fn()
                fn()
            continue
        row, res = dict(n_ego=n_ego, steps=S), {}
        for name, fn in calls.items():
            row[name], res[name] = timed(fn, args.reps)
        want = tc.host_ttc(egos[:1], ex, va, boxes)
        ok = all(np.array_equal(res["ttc_lanes1"][k], res["ttc_lanes2"][k]) for k in want) and all(np.array_equal(res["ttc_lanes2"][k][:1], want[k]) for k in want)
        row["layouts_agree_and_same_as_host"] = bool(ok)
        same = same and ok
        out[f"{n_ego}x{S}"] = row
        print(f"{n_ego:5d} egos x {S} steps: lanes 1 {row['ttc_lanes1']['median_ms']:.3f} ms, lanes 2 {row['ttc_lanes2']['median_ms']:.3f} ms, "
              f"mind_audit_episode {row['episode']['median_ms']:.3f} ms, same {ok}", flush=True)
    if args.once:
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
