"""Child process of test_gpu_ilqr.py::test_context_knobs_reach_the_launch_choice: a context created under the caller's MIND_ILQR_*
variables, the mind_set_tuning pairs of argv[1] (JSON) applied, one warm-start solve of the scripted `lead` tree.  Prints one JSON line:
workgroups per tree of that launch, what mind_set_tuning answers to an unknown name, the distance to the golden trajectory."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mind_amd.predictor import HipPredictor       # noqa: E402
from mind_amd.synth import scripted_scenario_tree  # noqa: E402
from oracle import ilqr as oi                      # noqa: E402

hp = HipPredictor(0)
for name, value in json.loads(sys.argv[1]).items():
    hp.set_tuning(name, value)
rc = hp.lib.mind_set_tuning(hp.ctx, b"ilqr_no_such_knob", 1)
msg = hp.lib.mind_last_error_string(hp.ctx).decode()
sst = scripted_scenario_tree("lead", 4)
flat = oi.flatten(sst["nodes"])
x0 = oi.init_state(sst["state"], sst["ctrl"])
xs, us, st = hp.ilqr_solve(oi.default_cfg(max_iter=100), [flat], x0, sst["target_lane"], sst["target_vel"], 0)
golden = np.load(os.path.join(ROOT, "tests", "golden", "ilqr.npz"))["lead_a4_it100_xs_w"]
print(json.dumps(dict(workgroups_per_tree=hp.ilqr_stats()[2], unknown_rc=rc, unknown_msg=msg, max_abs_err_xs_w=float(np.abs(xs[0] - golden).max()))))
hp.close()
