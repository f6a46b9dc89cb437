"""What the plan() surface costs: three drivers of the same recorded scene in ONE process, in interleaved blocks.

  (a) loop         ClosedLoopSim(native=None): mind_loop_*, the simulator and the planner behind one native call per cycle (the bench headline)
  (b) plan_python  ClosedLoopSim(native=False), native_plan off: the Python steps calling MINDPlanner.update_observation / plan in Python
  (c) plan_native  the same Python steps, native_plan on: update_observation = one mind_planner_observe, plan = one mind_planner_plan

Recorded demo_1, branching formula weights, the bench's planner configuration.  A block = one episode (60 planning cycles, 300 simulator
steps) after a reset; the blocks of the three drivers alternate a, b, c, a, b, c, ... on one context, so the box, the process and the
clocks are shared and only the driver differs (separate runs differ by more than the drivers do).  Every block replays the same plans:
the three drivers' ego state and control at the end of every block are compared bit for bit.

  python tools/plan_surface_rate.py [--blocks 8] [--plans 60] [--out profiles/plan_surface.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--plans", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_surface.json"))
    args = ap.parse_args()
    from bench import BRANCHING_WEIGHTS, WORKLOADS, make_closed_loop
    drivers = {}
    for name, native in (("loop", None), ("plan_python", False), ("plan_native", False)):
        pl, sim, _ = make_closed_loop(dict(WORKLOADS["demo_1"]), ckpt=BRANCHING_WEIGHTS, native=native)
        if name == "plan_native":
            pl.native_plan = True          # engages on the first frame of the next episode (the warm-up's reset below)
        drivers[name] = (pl, sim)
    assert drivers["loop"][1]._native is not None, drivers["loop"][1].native_reason
    for name, (pl, sim) in drivers.items():          # warm-up: one short episode each (first-use allocations, the library's staging)
        sim.reset()
        sim.run_plans(10)
    pn = drivers["plan_native"][0]
    assert pn._native is not None, pn.native_plan_stats
    assert drivers["plan_python"][0]._native is None
    rates = {k: [] for k in drivers}
    cycle_ms = {k: [] for k in drivers}
    same = True
    for b in range(args.blocks):
        ends = []
        for name, (pl, sim) in drivers.items():
            sim.reset()
            t0 = time.perf_counter()
            steps = sim.run_plans(args.plans)
            dt = time.perf_counter() - t0
            rates[name].append(steps / dt)
            cycle_ms[name].append(dt / args.plans * 1e3)
            ends.append((np.array(sim.state), np.array(sim.ctrl), sim.n_steps))
        same = same and all(np.array_equal(e[0], ends[0][0]) and np.array_equal(e[1], ends[0][1]) for e in ends[1:])
    st = pn.native_plan_stats
    out = {"scene": "demo_1", "weights": BRANCHING_WEIGHTS, "blocks": args.blocks, "plans_per_block": args.plans, "same_plans": bool(same),
           "native_plan_stats": {"native": st["native"], "fallback": st["fallback"]}, "drivers": {}}
    for name in drivers:
        r = np.array(rates[name])
        out["drivers"][name] = {"sim_steps_per_s": float(r.mean()), "ms_per_cycle": float(np.mean(cycle_ms[name])),
                                "spread_steps_per_s": float(r.max() - r.min()), "spread_pct": float((r.max() - r.min()) / r.mean() * 100.0),
                                "block_steps_per_s": [float(x) for x in r]}
    a, bb, c = (out["drivers"][k] for k in ("loop", "plan_python", "plan_native"))
    out["c_minus_b_steps_per_s"] = c["sim_steps_per_s"] - bb["sim_steps_per_s"]
    out["c_beats_b_by_more_than_b_spread"] = bool(out["c_minus_b_steps_per_s"] > bb["spread_steps_per_s"])
    out["c_below_a_pct"] = (1.0 - c["sim_steps_per_s"] / a["sim_steps_per_s"]) * 100.0
    out["c_minus_a_us_per_cycle"] = (c["ms_per_cycle"] - a["ms_per_cycle"]) * 1e3
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name in drivers:
        d = out["drivers"][name]
        print(f"{name:12s} {d['sim_steps_per_s']:8.1f} sim steps/s  {d['ms_per_cycle']:.4f} ms per cycle  spread over {args.blocks} blocks {d['spread_steps_per_s']:.1f} steps/s ({d['spread_pct']:.2f} %)")
    print(f"plan_native - plan_python = {out['c_minus_b_steps_per_s']:+.1f} steps/s (spread of plan_python {bb['spread_steps_per_s']:.1f}); "
          f"plan_native is {out['c_below_a_pct']:.2f} % below the loop ({out['c_minus_a_us_per_cycle']:+.1f} us per cycle); same plans: {same}")
    print(json.dumps({k: out[k] for k in ("c_beats_b_by_more_than_b_spread", "c_below_a_pct", "same_plans")}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
