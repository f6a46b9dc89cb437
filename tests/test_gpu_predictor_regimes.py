"""GPU parity of every predictor kernel variant AWAY from the formula weights: each variant under each weight regime of
tests/weight_regimes.py (peaked attention, pre-norm variance at the epsilon, mean-dominated rows, negative / zero / large gains, a second
seed), at the smallest shapes at which each mechanism of the pair / token kernels exists.

Truth is the float64 oracle.  e_ref = max |float32 oracle - float64 oracle| and e_hip = max |kernel - float64 oracle|, both over reg, vel
and cls of the same case.  The bar of the float32-class variants is

    e_hip <= 4 * e_ref + 5e-6   and   e_hip <= 2e-4

The factor 4: two independent float32 evaluations with different summation orders differ from the truth by up to 2 x the other's error at
the worst of ~1e4 outputs, times 2 for the kernels' longer re-associated sums (folded queries, split operands); 5e-6 is the project's
outright bound for bf16x6 (tests/test_gpu_predictor.py).  The bar never comes from the kernel's own output; tests/test_oracle_regimes.py
pins e_ref <= 3e-5 for every asserted regime on the CPU.  bf16x3 (opt-in, two-way split) gets 1e-3 m; plain bf16 is printed and checked for
finiteness; `saturated` (where the reference's own float32 is no witness) is checked for properties only.

Every case prints one line `regime shape variant e_ref e_hip bar`; profiles/predictor_regimes.txt is that table from a run on the MI355X.
A failing case names the first tap (ActorNet, LaneNet, tokens and edge tensor per fusion layer, mode tokens, target embedding) whose error
exceeds 4 x the float32 oracle's own error at that tap."""
import functools

import numpy as np
import pytest
import torch

import weight_regimes as wr
from mind_amd.synth import predictor_batch
from oracle import predictor as op

pytestmark = pytest.mark.gpu
NEVER = 1 << 30
OUTRIGHT = 2e-4
BAR_BF16X3 = 1e-3

# (a, l, B): N = 8 -- one tile, no split; N = 48 -- three tiles, three one-tile partials per column; N = 129 -- nine tiles in eight partials
# per column, one of which spans two tiles (the in-job running-maximum rescale and the cross-job combine both run)
SHAPES = [(3, 4, 1), (17, 30, 2), (16, 112, 1)]
SEED = wr.BATCH_SEED

# the knobs' defaults (mind_amd/csrc/pred_choice.h), restored after every case
DEFAULTS = {"pair_tile": 1, "actor_f32": 1, "actor_f32_min": NEVER, "actor_f32_pair_min": NEVER, "actor_lw_min": NEVER, "actor_split": 6,
            "tok_merge": 1, "tok_small_max": 2048, "tok_mfma": 0, "tok_bf_min_n": 0, "tok_lw_min_n": NEVER, "tok_lw_min": NEVER,
            "dec_mfma_min": NEVER, "dec_mw": 0, "dec_cls_side": 0, "dec_overlap": 1, "enc_mfma": 1}

# name -> (pair precision or None for the library default, knobs).  Float32 class: every entry of F32_CLASS.
F32_CLASS = {
    # pair arithmetic
    "bf16x6": ("bf16x6", {}),
    "f32": ("f32", {}),
    "bf16x6-pair_tile0": ("bf16x6", {"pair_tile": 0}),
    "f32-pair_tile0": ("f32", {"pair_tile": 0}),
    # ActorNet
    "default": (None, {}),
    "actor_f32=0": (None, {"actor_f32": 0}),
    "f32-actor_f32=0": ("f32", {"actor_f32": 0}),                 # (the fp32 VALU ActorNet: only the exact-fp32 setting reads the knob)
    "actor_f32_min=0": (None, {"actor_f32_min": 0}),
    "actor_f32_pair_min=0": (None, {"actor_f32_pair_min": 0}),
    "f32-actor_f32_pair_min=0": ("f32", {"actor_f32_pair_min": 0}),
    "actor_lw_min=0": (None, {"actor_lw_min": 0}),
    "actor_split=3": (None, {"actor_split": 3}),
    # token stage
    "tok_merge=0": (None, {"tok_merge": 0}),
    "tok_small_max=0": (None, {"tok_small_max": 0}),
    "tok_mfma=1": (None, {"tok_mfma": 1}),
    "tok_bf_min_n=0": (None, {"tok_bf_min_n": 0}),
    "tok_lw_min_n=0": (None, {"tok_lw_min_n": 0}),
    "tok_lw_min_n=0-tok_lw_min=0": (None, {"tok_lw_min_n": 0, "tok_lw_min": 0}),      # ... and the layer-wise kernels themselves
    # decoder
    "dec_mfma_min=0": (None, {"dec_mfma_min": 0}),
    "dec_mw=1": (None, {"dec_mw": 1}),
    "dec_cls_side=1": (None, {"dec_cls_side": 1}),
    "dec_overlap=0": (None, {"dec_overlap": 0}),
    "enc_mfma=0": (None, {"enc_mfma": 0}),
    "enc_mfma=0-dec_mfma_min=0": (None, {"enc_mfma": 0, "dec_mfma_min": 0}),
}
# the two-way split and the kernels only it reaches (k_pair_bf, k_actor_mfma<3>, k_token_mfma<1>)
BF16X3_CLASS = {
    "bf16x3": ("bf16x3", {}),
    "bf16x3-pair_tile0": ("bf16x3", {"pair_tile": 0}),
    "bf16x3-actor_split=3": ("bf16x3", {"actor_split": 3}),
    "bf16x3-tok_bf_min_n=1": ("bf16x3", {"tok_bf_min_n": 1}),
}


def to_t(pb):
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else [torch.from_numpy(x) for x in v])
            for k, v in pb.items()}


def _flat(xs):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])


def _max_err(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def oracle_case(regime, shape):
    """the batch, the float64 oracle's (reg, vel, cls) and e_ref of one (regime, shape): computed once per module run"""
    a, l, B = shape
    pb = predictor_batch(a, l, B, seed=SEED)
    sd = wr.regime_state_dict(regime)
    res = {}
    for dt in (torch.float64, torch.float32):
        cls, reg, vel = op.forward(sd, to_t(pb), dtype=dt)
        res[dt] = tuple(_flat([x.numpy() for x in xs]) for xs in (reg, vel, cls))
    return pb, res[torch.float64], _max_err(res[torch.float32], res[torch.float64])


@pytest.fixture(scope="module")
def regime_predictor(request):
    """(regime, its own HipPredictor(0) with the regime's weights loaded); one alive at a time, closed afterwards"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mind_amd.predictor import HipPredictor
    hp = HipPredictor(0)
    hp.load_state_dict(wr.regime_state_dict(request.param))
    yield request.param, hp
    hp.close()


def _hip_outputs(hp, pb, **kw):
    out = hp.predict_numpy_batch(pb, **kw)
    return out, tuple(out[k].double().cpu().numpy().reshape(-1) for k in ("reg", "vel", "cls"))


def _tap_table(hp, regime, shape):
    """[(tap name, e_ref at the tap, e_hip at the tap)] with the knobs as they are: ActorNet and LaneNet outputs, tokens and edge tensor
    after each fusion layer (mind_debug_set_layers), mode tokens, target embedding -- against the float64 oracle's taps"""
    a, l, B = shape
    n = a + l + 1
    pb = predictor_batch(a, l, B, seed=SEED)
    sd = wr.regime_state_dict(regime)
    t64, t32 = {}, {}
    op.forward(sd, to_t(pb), dtype=torch.float64, taps=t64)
    op.forward(sd, to_t(pb), dtype=torch.float32, taps=t32)
    rows = []

    def add(name, pick, got):
        w64, w32 = (np.asarray(pick(t), np.float64) for t in (t64, t32))
        rows.append((name, float(np.abs(w32 - w64).max()), float(np.abs(np.asarray(got, np.float64).reshape(w64.shape) - w64).max())))
    try:
        out = hp.predict_numpy_batch(pb, want_lane_feat=True)
        add("actor_feat", lambda t: t["actor_net"].numpy(), hp.debug_read("actor_feat"))
        add("lane_feat", lambda t: t["lane_net"].numpy(), out["lane_feat"].cpu().numpy())
        cmode, tgt_emb = hp.debug_read("cmode").copy(), hp.debug_read("tgt_emb").copy()
        used = list(range(a)) + [n - 1]          # the last layer computes the consumed tokens only (actors and cls)
        for k in range(1, 7):
            hp.debug_set_layers(k)
            hp.predict_numpy_batch(pb)
            x = hp.debug_read("x").reshape(B, n, 128)
            xs = lambda t: np.stack([t["fusion"][b][k - 1][0].numpy() for b in range(B)])
            if k == 6:
                add("x after layer 6", lambda t: xs(t)[:, used], x[:, used])
            else:
                add(f"x after layer {k}", xs, x)
            if k < 6:
                e = hp.debug_read("edge").reshape(B, n, n, 128).transpose(0, 2, 1, 3)      # -> the reference's [i][j]
                es = lambda t: np.stack([t["fusion"][b][k - 1][1].numpy() for b in range(B)])
                if k == 5:                       # layer 4 updates the consumed columns only
                    add("edge after layer 5", lambda t: es(t)[:, :, used], e[:, :, used])
                else:
                    add(f"edge after layer {k}", es, e)
        add("cmode", lambda t: np.stack([t["dec"][b]["cmode"].numpy().reshape(6, 128) for b in range(B)]), cmode)
        add("tgt_emb", lambda t: np.stack([t["dec"][b]["tgt_emb"].numpy().reshape(128) for b in range(B)]), tgt_emb)
    finally:
        hp.debug_set_layers(6)
    return rows


def first_bad_tap(hp, regime, shape):
    rows = _tap_table(hp, regime, shape)
    bad = [f"{name}: e_hip {eh:.2e} > 4 x e_ref {er:.2e}" for name, er, eh in rows if eh > 4 * er]
    return bad[0] if bad else "no tap exceeds 4 x the float32 oracle's own error: " + ", ".join(f"{nm} {eh:.1e}/{er:.1e}" for nm, er, eh in rows)


def run_case(regime_predictor, variant, spec, shape, bar_of):
    """one predictor call of `variant` on the case; returns (e_ref, e_hip, bar, where) -- `where` names the first bad tap when the bar is
    missed (computed with the variant's knobs still set)"""
    regime, hp = regime_predictor
    prec, knobs = spec
    pb, want, e_ref = oracle_case(regime, shape)
    assert e_ref <= wr.REF_ERR_BAR, (regime, shape, e_ref)      # a condition on the inputs: beyond it the float32 reference is no witness
    bar = bar_of(e_ref)
    before = hp.pair_precision()
    where = None
    try:
        if prec is not None:
            hp.set_pair_precision(prec)
        for k, v in knobs.items():
            hp.set_tuning(k, v)
        _, got = _hip_outputs(hp, pb)
        finite = all(np.isfinite(g).all() for g in got)
        e_hip = _max_err(got, want) if finite else float("inf")
        if bar is not None and not e_hip <= bar:
            where = first_bad_tap(hp, regime, shape)
    finally:
        for k in knobs:
            hp.set_tuning(k, DEFAULTS[k])
        hp.set_pair_precision(before)
    a, l, B = shape
    print(f"regime={regime} a={a} l={l} B={B} variant={variant} e_ref={e_ref:.2e} e_hip={e_hip:.2e} bar={'-' if bar is None else format(bar, '.2e')}")
    return e_ref, e_hip, bar, where


def _ids(shape):
    return "a%d_l%d_b%d" % shape


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("variant", list(F32_CLASS))
@pytest.mark.parametrize("regime_predictor", wr.ASSERTED, indirect=True)
def test_float32_class_variant_meets_the_reference_derived_bar(regime_predictor, variant, shape):
    e_ref, e_hip, bar, where = run_case(regime_predictor, variant, F32_CLASS[variant], shape, lambda e_ref: min(4 * e_ref + 5e-6, OUTRIGHT))
    assert e_hip <= bar, (regime_predictor[0], variant, shape, f"e_hip {e_hip:.3e} > min(4 x e_ref {e_ref:.3e} + 5e-6, 2e-4)", where)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("variant", list(BF16X3_CLASS))
@pytest.mark.parametrize("regime_predictor", wr.ASSERTED, indirect=True)
def test_two_way_split_variant_meets_its_own_bar(regime_predictor, variant, shape):
    """bf16x3 is opt-in and narrower than float32: 1e-3 m (the accuracy the planner needs), under every asserted regime.  Measured on the
    MI355X: <= 1.7e-4 everywhere but under `peaked`, where the two-way split's 2^-16 operand error is multiplied by logits 16 times larger:
    1.3e-4 .. 2.0e-4 (5.3e-4 with the two-way split ActorNet, 9.7e-4 at N = 8 with the two-way split token kernel as well)."""
    e_ref, e_hip, bar, where = run_case(regime_predictor, variant, BF16X3_CLASS[variant], shape, lambda e_ref: BAR_BF16X3)
    assert e_hip <= bar, (regime_predictor[0], variant, shape, f"e_hip {e_hip:.3e} > 1e-3", where)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("regime_predictor", wr.ASSERTED, indirect=True)
def test_plain_bf16_stays_finite(regime_predictor, shape):
    _, e_hip, _, _ = run_case(regime_predictor, "bf16", ("bf16", {}), shape, lambda e_ref: None)
    assert np.isfinite(e_hip)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("regime_predictor", ["saturated"], indirect=True)
def test_saturated_attention_keeps_the_output_properties(regime_predictor, shape):
    """q, k rows times 8 (logits 64 times the formula weights'): the float32 oracle itself is 2e-4 .. 5e-4 from float64 here, so the
    error is printed, not bounded; the outputs stay finite, cls sums to 1 and sigma is positive."""
    regime, hp = regime_predictor
    pb, want, e_ref = oracle_case(regime, shape)
    out, got = _hip_outputs(hp, pb)
    a, l, B = shape
    print(f"regime={regime} a={a} l={l} B={B} variant=default e_ref={e_ref:.2e} e_hip={_max_err(got, want):.2e} bar=-")
    assert all(torch.isfinite(out[k]).all() for k in ("cls", "reg", "vel"))
    assert (out["cls"].sum(dim=1) - 1).abs().max().item() < 1e-5
    assert (out["reg"][..., 2:] > 0).all()
