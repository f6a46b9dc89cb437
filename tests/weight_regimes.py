"""Weight regimes for the predictor parity tests (a plain helper module: tests/test_oracle_regimes.py and
tests/test_gpu_predictor_regimes.py import it).

The formula weights (mind_amd/weights.py) are one corner of the weight space: norm gains 1 +- 0.1, biases +- 0.05, attention logits that
span 2 to 4 (near-uniform softmax), pre-norm variances far above the normalisation epsilon.  Each regime here is a pure numpy function
from the formula state_dict to a new one that leaves that corner in one named direction, so that a kernel whose epsilon, running maximum,
rescale, mean subtraction or gain handling is subtly wrong costs more than the parity bar:

  plain      formula weights, seed 20240121 (the operating point of every other parity test)
  seed7      formula weights, seed 7
  peaked     q and k rows of every attention in_proj times 4: logits grow 16 times, the softmax is peaked (running maxima and the
             rescale / recombine factors of the split columns matter)
  saturated  the same rows times 8: the float32 reference itself is no witness any more (properties only)
  small      pre-norm variance comparable to the epsilon: the epsilon of every LayerNorm / GroupNorm site moves the outputs
  offset     +30 on the bias of every Linear that feeds a LayerNorm: rows dominated by their mean (one-pass variances cancel)
  gains      norm gains negative, zero and large; biases times 10

tests/test_oracle_regimes.py pins what each regime claims (reference error, attention peak, epsilon sensitivity) on the CPU."""
from collections import OrderedDict

import numpy as np

from mind_amd.weights import formula_state_dict

PLAIN_SEED = 20240121
# seed of the synthetic batches (mind_amd.synth.predictor_batch) the regime tests run: chosen by the reference side alone -- of seeds 1..7 one
# of the two at which max |float32 oracle - float64 oracle| stays below REF_ERR_BAR under every asserted regime at every shape the tests use
# (peaked attention at seed 4: 6.3e-5 at a = 16, l = 112)
BATCH_SEED = 3
REF_ERR_BAR = 3e-5
GAIN_PATTERN = np.array([-1.5, 0.0, 0.25, 3.0, 1.0, -0.5, 2.0, 1.0], np.float32)
SMALL = np.float32(3e-3)
SMALL_FIRST_LAYERS = ("actor_net.groups.0.0.conv1.weight", "actor_net.groups.0.0.downsample.0.weight", "lane_net.proj.0.weight",
                      "fusion_net.proj_rpe_scene.0.weight", "pred_scene.proj_rpe.0.weight")
LAST_LAYERS = ("pred_scene.cls.6", "pred_scene.reg.6")


def _is_gain(name, v):
    return name.endswith(".weight") and v.ndim == 1


def _copy(sd):
    return OrderedDict((k, np.array(v, np.float32)) for k, v in sd.items())


def norm_sites(sd):
    """prefixes of the LayerNorm / GroupNorm sites (every 1-D ``*.weight`` is a norm gain)"""
    return [k[:-len(".weight")] for k, v in sd.items() if _is_gain(k, np.asarray(v))]


def plain(sd):
    return _copy(sd)


def _qk_scaled(sd, f):
    out = _copy(sd)
    for k in out:
        if k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            out[k][:256] *= np.float32(f)
    return out


def peaked(sd):
    return _qk_scaled(sd, 4.0)


def saturated(sd):
    return _qk_scaled(sd, 8.0)


def small(sd):
    out = _copy(sd)
    for k, v in out.items():
        if k.endswith("bias"):
            if k[:-len(".bias")] not in LAST_LAYERS:
                v *= SMALL
        elif _is_gain(k, v) or k in SMALL_FIRST_LAYERS:
            v *= SMALL
        elif k[:-len(".weight")] in LAST_LAYERS:
            v *= np.float32(1.0) / SMALL
    return out


def offset(sd):
    out = _copy(sd)
    for k, v in out.items():
        if (k.endswith(".0.bias") or k.endswith(".3.bias")) and out[k[:-len("bias")] + "weight"].ndim == 2:
            v += np.float32(30.0)
    return out


def gains(sd):
    out = _copy(sd)
    for k, v in out.items():
        if _is_gain(k, v):
            v *= np.resize(GAIN_PATTERN, v.shape)
        elif k.endswith("bias") and not k.endswith("in_proj_bias") and not k.endswith(".6.bias"):
            v *= np.float32(10.0)
    return out


_TRANSFORMS = {"plain": plain, "seed7": plain, "peaked": peaked, "saturated": saturated, "small": small, "offset": offset, "gains": gains}
REGIMES = tuple(_TRANSFORMS)
ASSERTED = tuple(r for r in REGIMES if r != "saturated")      # `saturated`: the reference's own float32 is 2e-4 .. 5e-4 from float64
_cache = {}


def regime_state_dict(name, as_torch=True):
    """the regime's state_dict (float32; torch tensors by default, as HipPredictor.load_state_dict and the oracle take them)"""
    if name not in _cache:
        _cache[name] = _TRANSFORMS[name](formula_state_dict(seed=7 if name == "seed7" else PLAIN_SEED))
    sd = _cache[name]
    if not as_torch:
        return _copy(sd)
    import torch
    return OrderedDict((k, torch.from_numpy(v.copy())) for k, v in sd.items())
