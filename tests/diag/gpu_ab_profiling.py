"""GPU-box diagnostic: what the library's own launch timing (mind_set_profiling) costs the headline loop (native closed loop, recorded
demo_1, branching weights).  Blocks of whole episodes alternate between two arms on ONE context, first in the order a/b, then b/a, so the box,
the process and the scene history are shared and only the instrumentation differs.
  python tests/diag/gpu_ab_profiling.py [blocks per arm and order] [plans per block] [knob=a,b]
Without a knob the arms are set_profiling(True) and set_profiling(False); with one (prof_clock=0,1) both arms run with profiling ON and differ
in the knob's value (gpu_ab_tuning.py prices a knob with profiling off, where this one does nothing).  Prints us per cycle of every block, both
arms' means and block-to-block spreads, and checks that every block ends in the same simulator state and control (every block replays the same
episode, so any difference is the instrumentation's)."""
import os
import sys
import time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import BRANCHING_WEIGHTS, WORKLOADS, make_closed_loop
pos = [a for a in sys.argv[1:] if "=" not in a]
knob = [a for a in sys.argv[1:] if "=" in a]
blocks = int(pos[0]) if len(pos) > 0 else 5
per = int(pos[1]) if len(pos) > 1 else 60                 # one recorded episode (bench.make_closed_loop): every block replays the same plans
pl, sim, w = make_closed_loop(dict(WORKLOADS["demo_1"]), ckpt=BRANCHING_WEIGHTS, native=None)
assert sim._native is not None
rt = pl.network.rt
if knob:
    name, vals = knob[0].split("=")
    va, vb = (int(v) for v in vals.split(","))
    arms = [(f"profiling on, {name} = {va}", True, va), (f"profiling on, {name} = {vb}", True, vb)]
else:
    name = None
    arms = [("profiling on ", True, None), ("profiling off", False, None)]
sim.run_plans(10)
us = {0: [], 1: []}
ends = []
for order in ((0, 1), (1, 0)):
    for b in range(2 * blocks):
        k = order[b % 2]
        label, on, v = arms[k]
        if name is not None:
            rt.set_tuning(name, v)
        rt.set_profiling(on)
        sim.reset()
        t0 = time.perf_counter()
        sim.run_plans(per)
        dt = time.perf_counter() - t0
        rt.set_profiling(False)
        us[k].append(dt / per * 1e6)
        ends.append((np.array(sim.state, np.float64).tobytes(), np.array(sim.ctrl, np.float64).tobytes()))
        print(f"order {'a/b' if order[0] == 0 else 'b/a'} block {b:2d} {label}: {dt / per * 1e6:9.2f} us per cycle")
same = all(e == ends[0] for e in ends)
for k in (0, 1):
    a = np.array(us[k])
    print(f"{arms[k][0]}: mean {a.mean():9.2f} median {np.median(a):9.2f} min {a.min():9.2f} max {a.max():9.2f} "
          f"block-to-block spread (max - min) {a.max() - a.min():7.2f} us per cycle over {len(a)} blocks of {per} plans")
print(f"difference a - b: mean {np.mean(us[0]) - np.mean(us[1]):+.2f} median {np.median(us[0]) - np.median(us[1]):+.2f} us per cycle")
print(f"end of every block (state, control) identical: {same}")
assert same, "the arms' episodes ended in different states"
