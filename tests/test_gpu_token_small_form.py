"""GPU: the small-launch form of the token kernel (k_token_s, mind_amd/csrc/fusion_kernels.hip) gives the bits of k_token_m and of the plain
k_token<4>.  It requests the column partials' statistics and head values in one round trip behind meta, a stage's weights ahead of the stage
in front, and takes two tokens per workgroup on launches that still get a CU per workgroup -- loads and ownership move, no sum changes its
order.

cls, reg and vel of predictor calls must be torch.equal between k_token_m (form 1), k_token_s on four (2) and on two (3) tokens per
workgroup, the rule (0) and "tok_merge" 0, under the formula weights, a second seed and peaked attention (combine weights far from uniform),
in bf16x6 (the folded query as three bf16 parts: mode bits 16 | 32) and f32 (plain fp32 query), at
  (1, 3, 2)     N = 5: one slot per column, odd token counts, a last workgroup with one token
  (7, 12, 5)    a ragged batch, N = 20
  (40, 55, 1)   six slots per column
  (40, 80, 1)   N = 121: eight slots, the cap of the single-round-trip loads
  (36, 55, 5)   460 tokens: the two-token form on 230 workgroups
  (60, 120, 3)  543 tokens: the rule's other side (four tokens per workgroup)
and twelve cycles of the native loop on recorded demo_1, across an episode restart, must plan bit for bit the same under k_token_m and
under the rule."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weight_regimes as wr  # noqa: E402
from mind_amd import _lib  # noqa: E402
from mind_amd.synth import predictor_batch  # noqa: E402
from test_gpu_native_loop import _make, _same, _snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

# (a, l, B) -> (tokens, slots per column, the rule's form on the device's CUs: checked below)
SHAPES = [(1, 3, 2), (7, 12, 5), (40, 55, 1), (40, 80, 1), (36, 55, 5), (60, 120, 3)]
SLOTS = {(1, 3, 2): 1, (40, 55, 1): 6, (40, 80, 1): 8}
WEIGHTS = ("formula", "seed7", "peaked")
CYCLES, EPISODE = 12, 7


def column_splits(N):
    """pair_column_splits (mind_amd/csrc/pair_jobs.h) below 256 tokens: partial slots per column"""
    assert N < 256
    return max(1, min(8, -(-1024 // N), (N + 15) // 16))


def _state_dict(name):
    if name == "formula":
        from mind_amd.weights import formula_state_dict
        return formula_state_dict(as_torch=True)
    return wr.regime_state_dict(name)


@pytest.fixture(scope="module", params=WEIGHTS)
def predictor(request):
    from mind_amd.predictor import HipPredictor
    hp = HipPredictor(0)
    hp.load_state_dict(_state_dict(request.param))
    prec = hp.pair_precision()
    yield hp
    _lib.token_form(0, ctx=hp.ctx)
    hp.set_tuning("tok_merge", 1)
    hp.set_pair_precision(prec)
    hp.close()


def _outputs(hp, pb):
    out = hp.predict_numpy_batch(pb)
    return {k: out[k].clone() for k in ("cls", "reg", "vel")}


@pytest.mark.parametrize("prec", ["bf16x6", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_small_form_gives_the_bits_of_the_other_forms(predictor, shape, prec):
    hp = predictor
    a, l, B = shape
    pb = predictor_batch(a, l, B, seed=3)
    n_tok = (a + l + 1) * B
    if shape in SLOTS:
        assert column_splits(a + l + 1) == SLOTS[shape]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    # the shapes lie on the sides of the rule they are named for (on any device of 232 to 271 CUs)
    assert _lib.token_form(0, n_tok, n_cu) == (2 if n_tok == 543 else 3), (n_tok, n_cu)
    hp.set_pair_precision(prec)
    outs = {}
    try:
        for form in (1, 2, 3, 0):
            assert _lib.token_form(form, ctx=hp.ctx) == form
            outs[form] = _outputs(hp, pb)
        hp.set_tuning("tok_merge", 0)
        outs["plain"] = _outputs(hp, pb)
    finally:
        hp.set_tuning("tok_merge", 1)
        _lib.token_form(0, ctx=hp.ctx)
    ref = outs[1]
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert ref["reg"].numel() == a * B * 6 * 60 * 5
    for name, out in outs.items():
        for k in ("cls", "reg", "vel"):
            assert torch.equal(out[k], ref[k]), (name, k, (out[k] - ref[k]).abs().max().item())


def _loop_cycles(form):
    pl, sim = _make("demo_1", None, episode_plans=EPISODE)
    rt = pl.network.rt
    assert sim._native is not None
    snaps = []
    try:
        assert _lib.token_form(form, ctx=rt.ctx) == form
        for _ in range(CYCLES):
            sim.run_plans(1)
            snaps.append(_snapshot(pl, sim))
    finally:
        _lib.token_form(0, ctx=rt.ctx)
    assert sim.n_episodes == 1
    return snaps


def test_native_loop_plans_the_same_under_k_token_m_and_the_rule():
    old, new = _loop_cycles(1), _loop_cycles(0)
    assert len(old) == len(new) == CYCLES
    assert sum(len(s["costs"]) > 1 for s in old) >= 4          # the plans really branch: rounds beyond the root run
    for cycle, (a, b) in enumerate(zip(old, new)):
        _same(a, b, cycle)
