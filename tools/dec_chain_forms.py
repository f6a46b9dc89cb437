#!/usr/bin/env python3
"""Times the decoder's scene part alone in each of its forms (mind_debug_dec_scene): the one-workgroup kernel k_dec_scene (form 0) and the launch
chain k_dec_chain1..4 with 8 / 16 / 32 workgroups per scene, at 1 and 5 scenes (the two rounds of the headline loop) and at the batch sizes
where the rule of dec_chain.h changes G.  Per form: a warm-up, then 30 launches each between two events on the context's stream; the median,
the minimum and the maximum in microseconds.  The results of all forms are compared bit for bit on the way.

    python tools/dec_chain_forms.py [--scenes 1 5 9 17 32] [--reps 30] > profiles/dec_chain_forms.txt"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[1, 5, 9, 17, 32])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    import torch
    from mind_amd import _lib
    from mind_amd.predictor import HipPredictor
    from mind_amd.weights import formula_state_dict
    hp = HipPredictor(0)
    hp.load_state_dict(formula_state_dict(as_torch=True))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"# {torch.cuda.get_device_name(0)}, {n_cu} compute units; microseconds per launch of the scene part, median [min .. max] of {a.reps} launches, each between two events")
    print("# scenes   rule's G   " + "   ".join(f"{'form ' + str(f):>24}" for f in (0, 8, 16, 32)))
    for B in a.scenes:
        rows = np.random.default_rng(B).standard_normal((B, 128)).astype(np.float32)
        ref, cells = None, []
        for form in (0, 8, 16, 32):
            _lib.dec_scene(hp.lib, hp.ctx, rows, form, reps=a.warmup)
            cout, cls, ms = _lib.dec_scene(hp.lib, hp.ctx, rows, form, reps=a.reps, timed=True)
            if ref is None:
                ref = (cout, cls)
            same = np.array_equal(cout.view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(cls.view(np.uint32), ref[1].view(np.uint32))
            us = np.sort(ms.astype(np.float64)) * 1e3
            cells.append(f"{np.median(us):7.1f} [{us[0]:6.1f} .. {us[-1]:6.1f}]" + ("" if same else " BITS DIFFER"))
        g = next((g for g in (32, 16, 8) if B * g <= n_cu), 0)
        print(f"{B:8d} {g:10d}   " + "   ".join(f"{c:>24}" for c in cells), flush=True)
    hp.close()


if __name__ == "__main__":
    main()
