"""GPU-box measurement: the ActorNet alone, per-actor kernel (k_actor_mfma<NP>) against the layer-wise batched kernels
(actor_lw_kernels.hip), at A = 64 ... 16 384 actors per call in interleaved blocks -- the crossover from which "actor_lw_min" pays.

    python tools/actor_lw_crossover.py [precision=bf16x6] [repetitions=5] [out.json]

Each figure is HipPredictor.last_actor_stats()["ms"] (HIP events around the ActorNet's launches on the context stream, profiling on) of a
predictor call of A / 64 scenes of 64 actors and 4 polylines with the fusion layers switched off (debug_set_layers(0)), so a call is
little more than its encoders.  Per size: `reps` blocks of (old, new), one warm-up pair first; the new path "wins" at a size when it is
faster in EVERY repetition.  One JSON line on stdout (and in out.json)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEVER = 1 << 30


def main():
    prec = sys.argv[1] if len(sys.argv) > 1 else "bf16x6"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    from mind_amd.predictor import HipPredictor
    from mind_amd.synth import predictor_batch
    from mind_amd.weights import formula_state_dict
    hp = HipPredictor(0)
    hp.load_state_dict(formula_state_dict(as_torch=True))
    hp.set_pair_precision(prec)
    hp.set_profiling(True)
    hp.debug_set_layers(0)
    rows = []
    for A in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 13824, 16384):
        pb = predictor_batch(64, 4, A // 64, seed=7)
        t = {"old": [], "new": []}
        launches = 0
        for rep in range(reps + 1):
            for name, knob in (("old", NEVER), ("new", 0)):
                hp.set_tuning("actor_lw_min", knob)
                hp.predict_numpy_batch(pb)
                st = hp.last_actor_stats()
                assert st["layerwise"] == (1 if name == "new" else 0)
                if name == "new":
                    launches = st["launches"]
                if rep > 0:
                    t[name].append(st["ms"])
        wins = all(n < o for o, n in zip(t["old"], t["new"]))
        rows.append(dict(A=A, old_ms=[round(x, 4) for x in t["old"]], new_ms=[round(x, 4) for x in t["new"]],
                         old_median=round(float(np.median(t["old"])), 4), new_median=round(float(np.median(t["new"])), 4),
                         new_launches=launches, new_wins_every_rep=wins))
        print(f"A={A:6d}  k_actor_mfma {np.median(t['old']):8.3f} ms   layer-wise {np.median(t['new']):8.3f} ms ({launches} launches)   "
              f"new wins every repetition: {wins}", file=sys.stderr, flush=True)
    hp.set_tuning("actor_lw_min", NEVER)
    hp.close()
    winners = [r["A"] for r in rows if r["new_wins_every_rep"]]
    # the crossover: the smallest size from which the new path wins at every larger measured size too
    cross = None
    for r in reversed(rows):
        if not r["new_wins_every_rep"]:
            break
        cross = r["A"]
    line = json.dumps(dict(precision=prec, repetitions=reps, sizes=rows, sizes_won=winners, crossover_A=cross))
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
