"""GPU-box diagnostic: same-process A/B of the small, merged token launches' kernel (mind_debug_token_form: 0 the rule, 1 k_token_m,
2 / 3 k_token_s on four / two tokens per workgroup) on the headline loop (native closed loop, recorded demo_1).  Blocks of one whole
60-cycle episode alternate between the two forms on ONE context -- a b a b ... in the first half, b a b a ... in the second, so that
neither arm always follows the other -- and every block replays the same plans (the forms are bit-identical).
  python tests/diag/gpu_ab_token_form.py [form a = 1] [form b = 0] [blocks per arm = 10] [plans per block = 60]
Prints every block, then per arm the median us per cycle and the block-to-block spread (max - min), and the difference of the medians."""
import os
import statistics
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import BRANCHING_WEIGHTS, WORKLOADS, make_closed_loop
from mind_amd import _lib
fa = int(sys.argv[1]) if len(sys.argv) > 1 else 1
fb = int(sys.argv[2]) if len(sys.argv) > 2 else 0
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 10
per = int(sys.argv[4]) if len(sys.argv) > 4 else 60          # one recorded episode (bench.make_closed_loop)
assert fa != fb and blocks >= 2
pl, sim, w = make_closed_loop(dict(WORKLOADS["demo_1"]), ckpt=BRANCHING_WEIGHTS, native=None)
assert sim._native is not None
rt = pl.network.rt
sim.run_plans(10)
us = {fa: [], fb: []}
order = [(fa, fb)] * (blocks // 2) + [(fb, fa)] * (blocks - blocks // 2)
try:
    for pair in order:
        for f in pair:
            assert _lib.token_form(f, ctx=rt.ctx) == f
            sim.reset()
            t0 = time.perf_counter()
            sim.run_plans(per)
            us[f].append((time.perf_counter() - t0) / per * 1e6)
            print(f"block {len(us[fa]) + len(us[fb]):3d} form {f} ({_lib.TOKEN_FORMS[f]}): {us[f][-1]:8.1f} us per cycle")
finally:
    _lib.token_form(0, ctx=rt.ctx)
med = {f: statistics.median(v) for f, v in us.items()}
for f in (fa, fb):
    print(f"form {f} ({_lib.TOKEN_FORMS[f]}): median {med[f]:.1f} us per cycle over {len(us[f])} blocks of {per}, spread {max(us[f]) - min(us[f]):.1f} "
          f"(min {min(us[f]):.1f}, max {max(us[f]):.1f})")
print(f"difference of the medians (b - a): {med[fb] - med[fa]:+.1f} us per cycle; larger spread {max(max(v) - min(v) for v in us.values()):.1f}")
