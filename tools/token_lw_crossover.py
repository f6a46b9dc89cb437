"""GPU-box measurement: the token stage alone in its three forms -- k_token<8> (the default), k_token_mfma<0> ("tok_mfma" 1) and the
layer-wise kernels (token_lw_kernels.hip; "tok_lw_min_n" 0, "tok_lw_min" 0) -- at 2 k ... 70 k tokens per call in scenes of N = 321
(64 actors, 256 polylines: the cfg4 scene), in interleaved blocks in one process; then one cfg4 full-tree plan per block with and
without the two knobs.

    python tools/token_lw_crossover.py [precision=bf16x6] [repetitions=5] [out.json=profiles/token_lw_crossover.json] [plan_cycles=3]

Each figure comes from HipPredictor.last_token_stats() with profiling on (HIP events around every token launch on the context stream).
A call with the fusion layers switched off (debug_set_layers(0)) runs the init step only, a call with two layers runs init + two
steps of mode 2|4 behind real pair-kernel partials: step_ms = (ms(2 layers) - ms(0 layers)) / 2 is the time of one epilogue + prologue
launch (the 14-per-plan launch of the cfg4 profile); for the layer-wise form stage_ms carries the same difference per stage, so the
stage that bounds it can be named.  Per size: `reps` blocks of (valu, mfma, lw), one warm-up block first; the layer-wise form "wins" at
a size when its step is faster than k_token<8>'s in EVERY repetition.  One JSON line on stdout (and in out.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEVER = 1 << 30
FORMS = (("valu", dict(tok_mfma=0, tok_lw_min_n=NEVER, tok_lw_min=NEVER)), ("mfma", dict(tok_mfma=1, tok_lw_min_n=NEVER, tok_lw_min=NEVER)),
         ("lw", dict(tok_mfma=0, tok_lw_min_n=0, tok_lw_min=0)))
STAGES = ("init", "merge_v", "out_ln2", "ffn1", "ffn2_ln3", "stq", "kq", "one_kernel")


def set_form(hp, knobs):
    for k, v in knobs.items():
        hp.set_tuning(k, v)


def sizes(hp, prec, reps):
    from mind_amd.synth import predictor_batch
    hp.set_pair_precision(prec)
    hp.set_profiling(True)
    rows = []
    for B in (6, 12, 36, 72, 108, 216):
        pb = predictor_batch(64, 256, B, seed=21)
        t = {f: {0: [], 2: []} for f, _ in FORMS}
        stage = {0: [], 2: []}
        launches = chunks = 0
        for rep in range(reps + 1):
            for layers in (0, 2):
                hp.debug_set_layers(layers)
                for name, knobs in FORMS:
                    set_form(hp, knobs)
                    hp.predict_numpy_batch(pb)
                    st = hp.last_token_stats()
                    assert st["layerwise"] == (1 if name == "lw" else 0)
                    if rep == 0:
                        continue
                    t[name][layers].append(st["ms"])
                    if name == "lw":
                        stage[layers].append(st["stage_ms"])
                        launches, chunks = st["launches"], st["chunks"]
        step = {f: [(b - a) / 2 for a, b in zip(t[f][0], t[f][2])] for f, _ in FORMS}
        st_step = (np.median(np.array(stage[2]), axis=0) - np.median(np.array(stage[0]), axis=0)) / 2
        wins = all(n < o for o, n in zip(step["valu"], step["lw"]))
        row = dict(tokens=B * 321, scenes=B, lw_launches_2_layers=launches, lw_chunks=chunks, lw_wins_every_rep=wins)
        for f, _ in FORMS:
            row[f + "_step_ms"] = [round(x, 4) for x in step[f]]
            row[f + "_step_median"] = round(float(np.median(step[f])), 4)
            row[f + "_init_median"] = round(float(np.median(t[f][0])), 4)
        row["lw_stage_step_ms"] = {STAGES[i]: round(float(st_step[i]), 4) for i in range(1, 7)}
        rows.append(row)
        print(f"tokens={B * 321:6d}  k_token<8> {row['valu_step_median']:7.4f}  k_token_mfma<0> {row['mfma_step_median']:7.4f}  layer-wise "
              f"{row['lw_step_median']:7.4f} ms per step ({row['lw_stage_step_ms']})  lw wins every repetition: {wins}", file=sys.stderr, flush=True)
    hp.debug_set_layers(6)
    hp.set_profiling(False)
    set_form(hp, FORMS[0][1])
    return rows


def cfg4_plan(cycles):
    """consecutive cycles of the cfg4 full-tree closed loop (rounds of 1 / 6 / 36 / 216 scenes of N = 321), the knobs alternating cycle by cycle"""
    from bench import WORKLOADS, make_closed_loop
    pl, sim, _ = make_closed_loop(dict(WORKLOADS["cfg4tree"]), full_tree=True)
    rt = pl.network.rt
    wall = {"valu": [], "lw": []}
    for cyc in range(2 * (cycles + 1)):
        name = "lw" if cyc & 1 else "valu"
        set_form(rt, dict(FORMS)[name])
        t0 = time.perf_counter()
        sim.run_plans(1)
        dt = (time.perf_counter() - t0) * 1e3
        if cyc >= 2:
            wall[name].append(round(dt, 3))
    set_form(rt, FORMS[0][1])
    return dict(workload="cfg4tree", expanded_per_plan=int(pl.timing.get("nodes_expanded", 0)), plan_wall_ms=wall,
                valu_median=round(float(np.median(wall["valu"])), 3), lw_median=round(float(np.median(wall["lw"])), 3))


def main():
    prec = sys.argv[1] if len(sys.argv) > 1 else "bf16x6"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "token_lw_crossover.json")
    cycles = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    from mind_amd.predictor import HipPredictor
    from mind_amd.weights import formula_state_dict
    hp = HipPredictor(0)
    hp.load_state_dict(formula_state_dict(as_torch=True))
    rows = sizes(hp, prec, reps)
    hp.close()
    plan = cfg4_plan(cycles) if cycles > 0 else None
    cross = None
    for r in reversed(rows):
        if not r["lw_wins_every_rep"]:
            break
        cross = r["tokens"]
    line = json.dumps(dict(precision=prec, repetitions=reps, scene_tokens=321, sizes=rows, sizes_won=[r["tokens"] for r in rows if r["lw_wins_every_rep"]],
                           crossover_tokens=cross, cfg4_plan=plan))
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
