"""GPU: the decoder scene part's launch chain (k_dec_chain1..4, G workgroups per scene, no barrier) against the one-launch kernels.

mind_debug_dec_scene runs the scene part alone on given cls token rows in a given form: Cout and cls of the chain with G = 8 / 16 / 32 must be
the bits of the one-workgroup kernel (form 0) for 1, 2, 5 and 9 scenes, under the formula weights and under random weights (the seed7
regime of tests/weight_regimes.py: formula weights can hide a wrong row), on ordinary rows, on rows scaled by 1e3 and with an all-zero
row.  Through the predictor the default (chain by rule) must equal "dec_mw" 1 and "dec_cls_side" 1 on cls / reg / vel, and twelve cycles of
the native loop on recorded demo_1 across an episode restart must give the same plans with the chain as with "dec_mw" 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

FORMS = (8, 16, 32)
KINDS = ("ordinary", "scaled_1e3", "zero_row")


def _rows(B, kind):
    rows = np.random.default_rng(1000 + B).standard_normal((B, 128)).astype(np.float32)
    if kind == "scaled_1e3":
        rows *= np.float32(1e3)
    elif kind == "zero_row":
        rows[B - 1] = 0.0
    return rows


@pytest.fixture(scope="module")
def predictors(hip_predictor):
    import weight_regimes as wr
    from mind_amd.predictor import HipPredictor
    hp7 = HipPredictor(0)
    hp7.load_state_dict(wr.regime_state_dict("seed7"))
    yield {"formula": hip_predictor, "seed7": hp7}
    hp7.close()


_reference = {}


def _form0(hp, weights, B, kind):
    """the one-workgroup kernel's result, computed once per case and kept read-only"""
    from mind_amd import _lib
    key = (weights, B, kind)
    if key not in _reference:
        cout, cls = _lib.dec_scene(hp.lib, hp.ctx, _rows(B, kind), 0)
        cout.setflags(write=False)
        cls.setflags(write=False)
        _reference[key] = (cout, cls)
    return _reference[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 2, 5, 9])
@pytest.mark.parametrize("weights", ["formula", "seed7"])
def test_chain_forms_give_the_bits_of_the_one_workgroup_kernel(predictors, weights, B, kind):
    from mind_amd import _lib
    hp = predictors[weights]
    cout0, cls0 = _form0(hp, weights, B, kind)
    assert np.isfinite(cout0).all() and np.isfinite(cls0).all()
    assert np.allclose(cls0.sum(axis=1), 1.0, atol=1e-5)
    if kind == "ordinary":
        assert np.unique(cout0.reshape(B * 6, 128), axis=0).shape[0] == B * 6      # every mode token of every scene differs
    for G in FORMS:
        cout, cls = _lib.dec_scene(hp.lib, hp.ctx, _rows(B, kind), G)
        assert np.array_equal(cout.view(np.uint32), cout0.view(np.uint32)), (G, "Cout", int((cout.view(np.uint32) != cout0.view(np.uint32)).sum()))
        assert np.array_equal(cls.view(np.uint32), cls0.view(np.uint32)), (G, "cls")


def test_debug_entry_rejects_other_forms(hip_predictor):
    from mind_amd import _lib
    import ctypes as C
    hp = hip_predictor
    rows = _rows(1, "ordinary")
    fp = C.POINTER(C.c_float)
    cout, cls = np.zeros((1, 6, 128), np.float32), np.zeros((1, 6), np.float32)
    args = lambda form, n=1, reps=1: (hp.ctx, rows.ctypes.data_as(fp), n, form, cout.ctypes.data_as(fp), cls.ctypes.data_as(fp), reps, None)  # noqa: E731
    for form in (1, 4, 24, 64, -8):
        assert hp.lib.mind_debug_dec_scene(*args(form)) == _lib.MIND_EINVAL
    assert hp.lib.mind_debug_dec_scene(*args(8, n=0)) == _lib.MIND_EINVAL
    assert hp.lib.mind_debug_dec_scene(*args(8, reps=0)) == _lib.MIND_EINVAL
    assert hp.lib.mind_debug_dec_scene(None, *args(8)[1:]) == _lib.MIND_EINVAL


def _expected_g(n_scenes, n_cu):
    return next((g for g in (32, 16, 8) if n_scenes * g <= n_cu), 0)


BATCHES = [(40, 55, 1, 1), (7, 12, 5, 3), (1, 3, 2, 5), (3, 5, 32, 7), (2, 4, 40, 9)]


@pytest.mark.parametrize("a,l,B,seed", BATCHES)
def test_default_equals_the_one_launch_forms_through_the_predictor(hip_predictor, a, l, B, seed):
    import torch
    from mind_amd import _lib
    from mind_amd.synth import predictor_batch
    hp = hip_predictor
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    pb = predictor_batch(a, l, B, seed=seed)
    d = _lib.predict_choice({}, hp.pair_precision(), [(a, l)] * B, n_cu=n_cu)
    assert d["dec_chain_g"] == _expected_g(B, n_cu) and (d["dec_chain_g"] > 0) == (B * 8 <= n_cu)
    assert d["want_mw"] == 0 and d["cls_on_side"] == 0
    if n_cu == 256:
        assert d["dec_chain_g"] == {1: 32, 5: 32, 2: 32, 32: 8, 40: 0}[B]
    chain = {k: v.clone() for k, v in hp.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
    for knob in ("dec_mw", "dec_cls_side"):
        assert _lib.predict_choice({knob: 1}, hp.pair_precision(), [(a, l)] * B, n_cu=n_cu)["dec_chain_g"] == 0
        try:
            hp.set_tuning(knob, 1)
            ref = {k: v.clone() for k, v in hp.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        finally:
            hp.set_tuning(knob, 0)
        for k in ("cls", "reg", "vel"):
            assert torch.equal(chain[k], ref[k]), (knob, k)


def test_native_loop_plans_are_the_same_with_the_chain_and_with_dec_mw():
    """twelve cycles of the native loop on demo_1 across an episode restart: run A the default throughout, run B "dec_mw" 1 throughout"""
    from test_gpu_native_loop import _make, _same, _snapshot
    from mind_amd import _lib
    cycles, episode = 12, 7
    created = int(os.environ.get("MIND_DEC_MW", 0))

    def run(dec_mw):
        pl, sim = _make("demo_1", None, episode_plans=episode)
        rt = pl.network.rt
        assert sim._native is not None
        snaps = []
        try:
            rt.set_tuning("dec_mw", dec_mw)
            for _ in range(cycles):
                sim.run_plans(1)
                snaps.append(_snapshot(pl, sim))
        finally:
            rt.set_tuning("dec_mw", created)
        assert sim.n_episodes == 1
        return snaps

    a, b = run(0), run(1)
    assert _lib.predict_choice({}, "bf16x6", [(3, 4)])["dec_chain_g"] == 32 and _lib.predict_choice({"dec_mw": 1}, "bf16x6", [(3, 4)])["dec_chain_g"] == 0
    assert len(a) == len(b) == cycles
    assert sum(len(s["costs"]) > 1 for s in a) >= 4          # the plans really branch: rounds beyond the root run
    for cycle, (x, y) in enumerate(zip(a, b)):
        _same(x, y, cycle)
