"""The bits of the six launchable pair-kernel forms, pinned: SHA-256 of the raw bytes of cls, reg, vel and of the edge tensor after five
fusion layers, against hashes recorded from a build of an earlier commit on the MI355X (tests/golden/pair_bits_parent.json).  The existing
tests hold f32, bf16 and bf16x6 to a tolerance against the oracle; a refactor of the pair kernels has to keep every bit, and this is
where a "bit-identical" claim is checked.  A change that means to alter the arithmetic re-records the file
(python tests/test_gpu_pair_bits.py, on the GPU) and says so."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mind_amd.synth import predictor_batch
from oracle import predictor as op

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "pair_bits_parent.json")

# (arithmetic, pair_tile): k_pair | k_pair_bf<3>, k_pair_t<3> | k_pair_bf<1>, k_pair_t<1> | k_pair_t6
FORMS = {"f32": ("f32", 1), "bf16x3-tile0": ("bf16x3", 0), "bf16x3-tile1": ("bf16x3", 1), "bf16-tile0": ("bf16", 0), "bf16-tile1": ("bf16", 1),
         "bf16x6": ("bf16x6", 1)}
# N = 3: one ragged tile, the cls row and column dominate | N = 48: whole tiles, eight one-tile jobs per column, padding jobs, prefetch
# across job boundaries | N = 256: first size of the seven-tile rule (jobs of 5 / 5 / 6 tiles) | N = 31 beside N = 321: Jn of another scene
SHAPES = ["1-1-1-5", "17-30-3-4", "16-239-2-25", "mixed-31-321"]


@functools.lru_cache(maxsize=None)
def _batch(shape):
    if shape.startswith("mixed"):           # the batch of test_gpu_predictor._mixed_check
        small, big = predictor_batch(9, 21, 1, seed=2), predictor_batch(64, 256, 1, seed=21)
        pb = {"ACTORS": np.concatenate([small["ACTORS"], big["ACTORS"]]), "LANES": np.concatenate([small["LANES"], big["LANES"]]),
              "ACTOR_IDCS": [np.arange(9), np.arange(9, 73)], "LANE_IDCS": [np.arange(21), np.arange(21, 277)],
              "CTRS": small["CTRS"] + big["CTRS"], "VECS": small["VECS"] + big["VECS"],
              "TGT_NODES": np.concatenate([small["TGT_NODES"], big["TGT_NODES"]]), "TGT_RPE": np.concatenate([small["TGT_RPE"], big["TGT_RPE"]])}
    else:
        a, l, B, seed = (int(v) for v in shape.split("-"))
        pb = predictor_batch(a, l, B, seed=seed)
    pb["RPE"] = [op.rpe(torch.from_numpy(c), torch.from_numpy(v)).numpy() for c, v in zip(pb["CTRS"], pb["VECS"])]
    return pb


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _hashes(hp, form, shape, use_rpe):
    prec, tile = FORMS[form]
    pb = _batch(shape)
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        hp.set_tuning("pair_tile", tile)
        out = hp.predict_numpy_batch(pb, use_rpe=use_rpe)
        h = {k: _sha(out[k].cpu().numpy()) for k in ("cls", "reg", "vel")}
        hp.debug_set_layers(5)
        hp.predict_numpy_batch(pb, use_rpe=use_rpe)
        h["edge"] = _sha(hp.debug_read("edge"))
    finally:
        hp.debug_set_layers(6)
        hp.set_tuning("pair_tile", 1)
        hp.set_pair_precision(before)
    return h


def _key(form, shape, use_rpe):
    return f"{form}/{shape}/{'rpe_tensor' if use_rpe else 'rpe_in_kernel'}"


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _fresh_predictor():
    """a context of its own with the formula weights and every knob at its default: the state the hashes were recorded in, whatever the
    tests before this module left in the shared one"""
    from mind_amd.predictor import HipPredictor
    from mind_amd.weights import formula_state_dict
    hp = HipPredictor(0)
    hp.load_state_dict(formula_state_dict(as_torch=True))
    return hp


@pytest.fixture(scope="module")
def pin_predictor():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    hp = _fresh_predictor()
    yield hp
    hp.close()


@pytest.mark.parametrize("use_rpe", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_pair_kernel_bits_equal_the_recorded_ones(form, shape, use_rpe, pin_predictor):
    assert _hashes(pin_predictor, form, shape, use_rpe) == _golden()[_key(form, shape, use_rpe)]


def record(path=GOLDEN):
    """Recompute every hash with the library as built and write the golden file (run on the GPU, from the commit whose bits are the pin)."""
    hp = _fresh_predictor()
    rec = {_key(f, s, r): _hashes(hp, f, s, r) for f in FORMS for s in SHAPES for r in (False, True)}
    hp.close()
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(rec)} cases -> {path}")


if __name__ == "__main__":
    record(*sys.argv[1:2])
