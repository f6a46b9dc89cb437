"""GPU parity: the HIP predictor (through the C-ABI) against the oracle and the golden vectors.
Tolerance: 2e-4 absolute on O(1..10 m) trajectory outputs (north_star asks 1e-3 m), in the default arithmetic of the pair
kernel (bf16x6: operands split exactly into bf16 hi + mid + lo, six products, fp32 accumulate: the reference's fp32 class), in its fp32-MFMA
mode AND in the opt-in two-way split (bf16x3); observed ~3e-6 (bf16x6, f32), ~1e-5 (bf16x3).
The plain-bf16 mode (BASELINE config 5) is measured and reported, against a bar it can meet."""
import numpy as np
import pytest
import torch

from mind_amd.synth import predictor_batch
from oracle import predictor as op

pytestmark = pytest.mark.gpu
TOL = 2e-4


def to_t(pb):
    return {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else [torch.from_numpy(x) for x in v])
            for k, v in pb.items()}


@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (8, 20, 2, 1), (40, 55, 1, 1), (2, 2, 1, 3)])
def test_hip_matches_golden(a, l, B, seed, hip_predictor, golden_predictor):
    g = golden_predictor
    key = f"a{a}_l{l}_b{B}_s{seed}"
    pb = predictor_batch(a, l, B, seed=seed)
    out = hip_predictor.predict_numpy_batch(pb, want_lane_feat=True)
    af = hip_predictor.debug_read("actor_feat").reshape(-1, 128)
    assert np.abs(af - g[key + "_actor_net"]).max() < 5e-5
    assert np.abs(out["lane_feat"].cpu().numpy() - g[key + "_lane_net"]).max() < 5e-5
    assert np.abs(out["cls"].cpu().numpy() - g[key + "_cls"]).max() < 1e-5
    reg, vel = out["reg"].cpu().numpy(), out["vel"].cpu().numpy()
    if key + "_tidx" in g:
        reg, vel = reg[:, :, g[key + "_tidx"]], vel[:, :, g[key + "_tidx"]]
    assert np.abs(reg - g[key + "_reg"]).max() < TOL
    assert np.abs(vel - g[key + "_vel"]).max() < TOL


@pytest.mark.parametrize("prec,tol", [("f32", 5e-5), ("bf16x3", 5e-5), ("bf16x6", 5e-5)])
@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (8, 20, 2, 1), (40, 55, 1, 1)])
def test_actor_net_tap_by_arithmetic(prec, tol, a, l, B, seed, hip_predictor, golden_predictor):
    """ActorNet output against the reference's golden tap, 5e-5 absolute on values up to ~4: the fp32 MFMA kernel (k_actor_f32, "f32")
    and the MFMA kernel with both operands split into three bf16 parts (k_actor_mfma<6>, the default)."""
    g = golden_predictor
    pb = predictor_batch(a, l, B, seed=seed)
    before = hip_predictor.pair_precision()
    try:
        hip_predictor.set_pair_precision(prec)
        hip_predictor.predict_numpy_batch(pb)
        af = hip_predictor.debug_read("actor_feat").reshape(-1, 128)
    finally:
        hip_predictor.set_pair_precision(before)
    assert np.abs(af - g[f"a{a}_l{l}_b{B}_s{seed}_actor_net"]).max() < tol


@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (8, 20, 2, 1), (40, 55, 1, 1)])
def test_actor_net_on_the_fp32_mfma_one_and_two_actors_per_workgroup(a, l, B, seed, hip_predictor, golden_predictor):
    """k_actor_f32 (actor_f32_kernels.hip: plain fp32 operands on v_mfma_f32_16x16x4_f32): the ActorNet of the exact-fp32 setting with one
    actor per workgroup, and -- two actors per workgroup, the 6-step layers' weight fragments shared -- of every setting on full-tree rounds.
    Both against the reference's golden tap at the fp32 tolerance (odd actor counts leave the last workgroup half empty), against each other,
    and against the fp32 VALU kernel they replace ("actor_f32" 0)."""
    g = golden_predictor
    pb = predictor_batch(a, l, B, seed=seed)
    before = hip_predictor.pair_precision()
    outs = {}
    try:
        for name, prec, tun in (("f32 x1", "f32", {}), ("f32 x2", "f32", {"actor_f32_pair_min": 0}), ("valu", "f32", {"actor_f32": 0}),
                                ("default x2", "bf16x3", {"actor_f32_min": 0})):
            hip_predictor.set_pair_precision(prec)
            for k, v in tun.items():
                hip_predictor.set_tuning(k, v)
            hip_predictor.predict_numpy_batch(pb)
            outs[name] = hip_predictor.debug_read("actor_feat").reshape(-1, 128).copy()
            hip_predictor.set_tuning("actor_f32", 1); hip_predictor.set_tuning("actor_f32_pair_min", 1 << 30); hip_predictor.set_tuning("actor_f32_min", 1 << 30)
    finally:
        hip_predictor.set_tuning("actor_f32", 1); hip_predictor.set_tuning("actor_f32_pair_min", 1 << 30); hip_predictor.set_tuning("actor_f32_min", 1 << 30)
        hip_predictor.set_pair_precision(before)
    want = g[f"a{a}_l{l}_b{B}_s{seed}_actor_net"]
    for name, af in outs.items():
        assert af.shape == want.shape and np.abs(af - want).max() < 5e-5, (name, float(np.abs(af - want).max()))
    assert np.abs(outs["f32 x1"] - outs["f32 x2"]).max() < 1e-5 and np.array_equal(outs["f32 x2"], outs["default x2"])
    assert np.abs(outs["f32 x1"] - outs["valu"]).max() < 2e-5


@pytest.mark.parametrize("a,l,B,seed", [(1, 1, 1, 5), (5, 1, 2, 5), (16, 15, 3, 2), (17, 30, 3, 4), (33, 64, 2, 6)])
def test_hip_matches_oracle_ragged_tiles(a, l, B, seed, hip_predictor, formula_sd):
    """N = a+l+1 around the 16-row tile boundary (N=3, 7, 32, 48, 98), multi-scene batches, l=1
    (which the reference itself cannot run, Q7)."""
    pb = predictor_batch(a, l, B, seed=seed)
    oc, orr, ov = op.forward(formula_sd, to_t(pb))
    out = hip_predictor.predict_numpy_batch(pb)
    cls, reg, vel = out["cls"].cpu().numpy(), out["reg"].cpu().numpy(), out["vel"].cpu().numpy()
    for b in range(B):
        assert np.abs(cls[b] - oc[b].numpy()[0]).max() < 1e-5
        assert np.abs(reg[b * a:(b + 1) * a] - orr[b].numpy()).max() < TOL
        assert np.abs(vel[b * a:(b + 1) * a] - ov[b].numpy()).max() < TOL


def test_mixed_scene_sizes_in_one_batch(hip_predictor, formula_sd):
    """Scenes of different (a, l) collated into one call, as AIME batches are after pruning."""
    p1, p2 = predictor_batch(5, 9, 1, seed=11), predictor_batch(12, 20, 1, seed=12)
    pb = {"ACTORS": np.concatenate([p1["ACTORS"], p2["ACTORS"]]), "LANES": np.concatenate([p1["LANES"], p2["LANES"]]),
          "ACTOR_IDCS": [np.arange(5), np.arange(5, 17)], "LANE_IDCS": [np.arange(9), np.arange(9, 29)],
          "CTRS": p1["CTRS"] + p2["CTRS"], "VECS": p1["VECS"] + p2["VECS"],
          "TGT_NODES": np.concatenate([p1["TGT_NODES"], p2["TGT_NODES"]]),
          "TGT_RPE": np.concatenate([p1["TGT_RPE"], p2["TGT_RPE"]])}
    out = hip_predictor.predict_numpy_batch(pb)
    reg = out["reg"].cpu().numpy()
    for p, sl in ((p1, slice(0, 5)), (p2, slice(5, 17))):
        _, orr, _ = op.forward(formula_sd, to_t(p))
        assert np.abs(reg[sl] - orr[0].numpy()).max() < TOL


def test_rpe_tensor_input_equals_in_kernel_rpe(hip_predictor):
    pb = predictor_batch(8, 20, 2, seed=1)
    o1 = hip_predictor.predict_numpy_batch(pb)
    pb["RPE"] = [op.rpe(torch.from_numpy(c), torch.from_numpy(v)).numpy() for c, v in zip(pb["CTRS"], pb["VECS"])]
    o2 = hip_predictor.predict_numpy_batch(pb, use_rpe=True)
    assert (o1["reg"] - o2["reg"]).abs().max().item() < 1e-5


def test_lane_feature_reuse_is_identical(hip_predictor):
    """LaneNet output computed once and fed back (reuse across tree nodes of a plan)."""
    pb = predictor_batch(8, 20, 2, seed=1)
    o1 = hip_predictor.predict_numpy_batch(pb, want_lane_feat=True)
    o2 = hip_predictor.predict_numpy_batch(pb, lane_feat=o1["lane_feat"])
    assert torch.equal(o1["reg"], o2["reg"]) and torch.equal(o1["cls"], o2["cls"])


def test_deterministic_and_batch_invariant(hip_predictor):
    """Scene results do not depend on batch composition (needed for identical AIME node sets on 1..8 GPUs)."""
    pb2 = predictor_batch(8, 20, 2, seed=1)
    o2 = hip_predictor.predict_numpy_batch(pb2)
    o2b = hip_predictor.predict_numpy_batch(pb2)
    assert torch.equal(o2["reg"], o2b["reg"])
    pb1 = {k: (v[:8] if k == "ACTORS" else v[:20] if k == "LANES" else v[:1]) for k, v in pb2.items()}
    o1 = hip_predictor.predict_numpy_batch(pb1)
    # the column-split rule depends on the scene's own size only -> bit-identical for any batch composition
    assert torch.equal(o1["reg"], o2["reg"][:8]) and torch.equal(o1["cls"], o2["cls"][:1])


def test_full_size_properties(hip_predictor):
    """cfg4 size (64 agents x 256 lanes): probabilities sum to 1, sigma > 0, finite outputs,
    Bezier end points: pos(t=0) equals the first control point for every mode (size independent)."""
    pb = predictor_batch(64, 256, 2, seed=3)
    out = hip_predictor.predict_numpy_batch(pb)
    cls, reg = out["cls"], out["reg"]
    assert torch.isfinite(reg).all() and torch.isfinite(out["vel"]).all()
    assert (cls.sum(dim=1) - 1).abs().max().item() < 1e-5
    assert (reg[..., 2:] > 0).all()


@pytest.mark.parametrize("a,l,seed", [(64, 256, 21), (128, 256, 22)])
def test_hip_matches_oracle_at_benchmark_sizes(a, l, seed, hip_predictor, formula_sd):
    """The sizes the pair kernel is measured at (cfg4: N = 321 tokens, stress: N = 385): here every query column is split
    over several workgroup passes and the partial softmax / sum p*mem results are combined by k_token -- the oracle
    (which materialises the [N,N,128] memory tensor as the reference does) needs a few seconds per scene."""
    pb = predictor_batch(a, l, 1, seed=seed)
    oc, orr, ov = op.forward(formula_sd, to_t(pb))
    out = hip_predictor.predict_numpy_batch(pb)
    assert np.abs(out["cls"].cpu().numpy()[0] - oc[0].numpy()[0]).max() < 1e-5
    assert np.abs(out["reg"].cpu().numpy() - orr[0].numpy()).max() < TOL
    assert np.abs(out["vel"].cpu().numpy() - ov[0].numpy()).max() < TOL


@pytest.mark.parametrize("prec,bar", [("f32", 2e-4), ("bf16x3", 2e-4), ("bf16x6", 2e-4)])
@pytest.mark.parametrize("a,l,B,seed", [(8, 20, 2, 1), (40, 55, 1, 1), (33, 64, 2, 6), (64, 256, 1, 21)])
def test_pair_kernel_arithmetics_meet_the_parity_bar(prec, bar, a, l, B, seed, hip_predictor, formula_sd):
    """Both fp32-class arithmetics of the pair kernel against the oracle at small, demo and cfg4 sizes (the default mode is
    whatever MIND_PAIR_PREC / the library default says; this test pins each explicitly)."""
    pb = predictor_batch(a, l, B, seed=seed)
    oc, orr, ov = op.forward(formula_sd, to_t(pb))
    before = hip_predictor.pair_precision()
    try:
        hip_predictor.set_pair_precision(prec)
        assert hip_predictor.pair_precision() == prec
        out = hip_predictor.predict_numpy_batch(pb)
    finally:
        hip_predictor.set_pair_precision(before)
    cls, reg, vel = out["cls"].cpu().numpy(), out["reg"].cpu().numpy(), out["vel"].cpu().numpy()
    for b in range(B):
        assert np.abs(cls[b] - oc[b].numpy()[0]).max() < 1e-5
        assert np.abs(reg[b * a:(b + 1) * a] - orr[b].numpy()).max() < bar
        assert np.abs(vel[b * a:(b + 1) * a] - ov[b].numpy()).max() < bar


def test_three_way_split_pair_kernel_is_as_accurate_as_the_fp32_mfma_one(hip_predictor, formula_sd):
    """k_pair_t6 ("bf16x6": both operands of every contraction split EXACTLY into bf16 hi + mid + lo, the six partial products >= 2^-24 on the
    bf16 MFMA, fp32 accumulate) is an fp32-class arithmetic: at demo size, N = 321 (cfg4) and N = 385 (stress) its error against the oracle is
    no larger than that of k_pair (plain fp32 operands on the fp32 MFMA) on the same inputs -- up to the noise of two different fp32
    summation orders -- and below 5e-6 m outright, where the two-way split (bf16x3) sits near 1e-5.  Ragged small scenes ride along."""
    rows = []
    for a, l, B, seed in ((40, 55, 1, 1), (64, 256, 1, 21), (128, 256, 1, 22), (5, 9, 3, 2), (17, 30, 2, 4)):
        pb = predictor_batch(a, l, B, seed=seed)
        oc, orr, ov = op.forward(formula_sd, to_t(pb))
        err = {}
        before = hip_predictor.pair_precision()
        try:
            for prec in ("f32", "bf16x6", "bf16x3"):
                hip_predictor.set_pair_precision(prec)
                out = hip_predictor.predict_numpy_batch(pb)
                reg, vel, cls = out["reg"].cpu().numpy(), out["vel"].cpu().numpy(), out["cls"].cpu().numpy()
                err[prec] = (max(float(np.abs(reg[b * a:(b + 1) * a] - orr[b].numpy()).max()) for b in range(B)),
                             max(float(np.abs(vel[b * a:(b + 1) * a] - ov[b].numpy()).max()) for b in range(B)),
                             max(float(np.abs(cls[b] - oc[b].numpy()[0]).max()) for b in range(B)))
        finally:
            hip_predictor.set_pair_precision(before)
        rows.append((a, l, B, err))
        print(f"a={a} l={l} B={B}: max |reg - oracle| f32 {err['f32'][0]:.2e}  bf16x6 {err['bf16x6'][0]:.2e}  bf16x3 {err['bf16x3'][0]:.2e} m; "
              f"vel {err['f32'][1]:.2e} / {err['bf16x6'][1]:.2e} / {err['bf16x3'][1]:.2e}; cls {err['f32'][2]:.2e} / {err['bf16x6'][2]:.2e} / {err['bf16x3'][2]:.2e}")
    for a, l, B, err in rows:
        assert err["bf16x6"][0] < 5e-6 and err["bf16x6"][1] < 5e-6 and err["bf16x6"][2] < 2e-6, (a, l, err)
        # no larger than the fp32 MFMA kernel's, with a margin for two different summation orders of the same fp32 terms
        assert err["bf16x6"][0] <= 1.5 * err["f32"][0] + 5e-7 and err["bf16x6"][1] <= 1.5 * err["f32"][1] + 5e-7, (a, l, err)
    # ... and over all cases together it is not the worse of the two
    assert sum(e["bf16x6"][0] for *_, e in rows) <= 1.25 * sum(e["f32"][0] for *_, e in rows)


def test_default_pair_arithmetic_is_the_fp32_class_split(hip_predictor):
    """the library computes in the reference's arithmetic class unless asked otherwise (bf16x3 / bf16 are opt-in)"""
    import os
    if "MIND_PAIR_PREC" not in os.environ:
        assert hip_predictor.pair_precision() == "bf16x6"


def test_plain_bf16_mode_error_is_reported(hip_predictor, formula_sd):
    """BASELINE config 5's 'bf16 MFMA attention': plain bf16 operands in the pair contractions.  It cannot meet the 1e-3 m
    bar (CPU emulation tests/diag/bf16_split_emulation.py: 2e-3 .. 4e-3 m); the test records what it does reach at the
    demo and stress scene sizes and bounds it, so that a regression of the mode is still caught."""
    worst = 0.0
    for a, l, seed in ((40, 55, 1), (128, 256, 22)):
        pb = predictor_batch(a, l, 1, seed=seed)
        oc, orr, ov = op.forward(formula_sd, to_t(pb))
        before = hip_predictor.pair_precision()
        try:
            hip_predictor.set_pair_precision("bf16")
            out = hip_predictor.predict_numpy_batch(pb)
        finally:
            hip_predictor.set_pair_precision(before)
        err = float(np.abs(out["reg"].cpu().numpy() - orr[0].numpy()).max())
        print(f"plain bf16 pair kernel, a={a} l={l}: max |reg - oracle| = {err:.3e} m")
        assert np.isfinite(err) and err < 5e-2
        assert np.abs(out["cls"].cpu().numpy()[0] - oc[0].numpy()[0]).max() < 5e-3
        worst = max(worst, err)
    assert worst > 1e-5          # it really ran in reduced precision


@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (17, 30, 3, 4), (40, 55, 1, 1), (64, 256, 1, 21)])
def test_decoder_actor_part_on_the_mfma_kernel(a, l, B, seed, hip_predictor, formula_sd):
    """k_dec_actor_mfma (actor_proj / reg head GEMMs on the bf16 MFMA with three-way split operands; opt-in:
    mind_set_tuning) switched on at small and ragged sizes (3, 51, 40, 64 agents: partial 16-agent workgroups) against the oracle, and
    against the fp32 VALU kernel it replaces."""
    pb = predictor_batch(a, l, B, seed=seed)
    oc, orr, ov = op.forward(formula_sd, to_t(pb))
    ref = hip_predictor.predict_numpy_batch(pb)
    try:
        hip_predictor.set_tuning("dec_mfma_min", 0)
        out = hip_predictor.predict_numpy_batch(pb)
    finally:
        hip_predictor.set_tuning("dec_mfma_min", 1 << 30)
    reg, vel = out["reg"].cpu().numpy(), out["vel"].cpu().numpy()
    for b in range(B):
        assert np.abs(reg[b * a:(b + 1) * a] - orr[b].numpy()).max() < TOL
        assert np.abs(vel[b * a:(b + 1) * a] - ov[b].numpy()).max() < TOL
    assert (out["reg"] - ref["reg"]).abs().max().item() < 5e-5
    assert not torch.equal(out["reg"], ref["reg"])          # it really was the other kernel


@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (17, 30, 3, 4), (40, 55, 2, 1)])
def test_decoder_halves_on_two_streams_are_bit_identical(a, l, B, seed, hip_predictor):
    """The decoder's actor part as two launches (actor_proj on the side stream beside k_dec_scene, then the head on the context
    stream: the default) against the one-kernel form: same code per element, identical bits, also when called back to back."""
    pb = predictor_batch(a, l, B, seed=seed)
    two = [hip_predictor.predict_numpy_batch(pb) for _ in range(2)]
    try:
        hip_predictor.set_tuning("dec_overlap", 0)
        one = hip_predictor.predict_numpy_batch(pb)
    finally:
        hip_predictor.set_tuning("dec_overlap", 1)
    for k in ("cls", "reg", "vel"):
        assert torch.equal(two[0][k], one[k]) and torch.equal(two[1][k], one[k]), k


@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (17, 30, 3, 4), (40, 55, 1, 1)])
def test_token_kernel_on_the_fp32_mfma(a, l, B, seed, hip_predictor, formula_sd):
    """k_token_mfma (opt-in, mind_set_tuning("tok_mfma")): every projection of the per-token epilogue / prologue of the fusion layers on
    v_mfma_f32_16x16x4_f32, 16 tokens per workgroup (ragged last tile at these sizes), against the oracle and against the fp32 VALU
    kernel it replaces (network.py:177-179, 205-232)."""
    pb = predictor_batch(a, l, B, seed=seed)
    oc, orr, ov = op.forward(formula_sd, to_t(pb))
    ref = hip_predictor.predict_numpy_batch(pb)
    try:
        hip_predictor.set_tuning("tok_mfma", 1)
        out = hip_predictor.predict_numpy_batch(pb)
    finally:
        hip_predictor.set_tuning("tok_mfma", 0)
    reg, vel = out["reg"].cpu().numpy(), out["vel"].cpu().numpy()
    for b in range(B):
        assert np.abs(reg[b * a:(b + 1) * a] - orr[b].numpy()).max() < TOL
        assert np.abs(vel[b * a:(b + 1) * a] - ov[b].numpy()).max() < TOL
    assert (out["reg"] - ref["reg"]).abs().max().item() < 5e-5
    assert not torch.equal(out["reg"], ref["reg"])          # it really was the other kernel


@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (17, 30, 3, 4), (40, 55, 1, 1), (9, 21, 5, 2)])
def test_token_kernel_tokens_per_workgroup_do_not_change_results(a, l, B, seed, hip_predictor):
    """k_token has two instantiations -- eight tokens per workgroup for big batches, four for small ones (mind_set_tuning
    "tok_small_max") -- with the same k split and summation order: a scene's result is the same bits whichever one its batch gets
    (the property the sharded / fused paths rely on)."""
    pb = predictor_batch(a, l, B, seed=seed)
    try:
        hip_predictor.set_tuning("tok_small_max", 0)          # everything on the eight-token kernel
        big = hip_predictor.predict_numpy_batch(pb)
        big = {k: v.clone() for k, v in big.items() if torch.is_tensor(v)}
        hip_predictor.set_tuning("tok_small_max", 1 << 30)    # everything on the four-token kernel
        small = hip_predictor.predict_numpy_batch(pb)
    finally:
        hip_predictor.set_tuning("tok_small_max", 2048)
    for k in ("cls", "reg", "vel"):
        assert torch.equal(big[k], small[k]), k


def test_token_kernel_with_merged_projections_equals_the_plain_one(hip_predictor):
    """Small launches run k_token_m: the projections that do not depend on each other (the two halves of the feed-forward layer's first
    matrix; S / T / q of the next layer's prologue) load their weights together and meet behind one pair of barriers -- three of ten
    dependent stages fewer (mind_set_tuning("tok_merge", 0): the plain kernel).  Same loads, same multiply-adds, same summation order:
    every output the same bits, on a lone scene and on ragged batches."""
    for pb in (predictor_batch(40, 55, 1, seed=1), predictor_batch(7, 12, 5, seed=3), predictor_batch(1, 3, 2, seed=5)):
        merged = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        try:
            hip_predictor.set_tuning("tok_merge", 0)
            plain = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        finally:
            hip_predictor.set_tuning("tok_merge", 1)
        for k in ("cls", "reg", "vel"):
            assert torch.equal(merged[k], plain[k]), k


def test_decoder_cls_head_on_the_side_stream_equals_the_one_launch_form(hip_predictor):
    """mind_set_tuning("dec_cls_side", 1): the scene part of the decoder as two launches -- the mode tokens (k_dec_scene_c) and, on the side stream
    beside the actor part's head, the mode probabilities (k_dec_cls).  The same code on the same values: every output the same bits
    (opt-in: measured slower than the one-launch kernel)."""
    for pb in (predictor_batch(40, 55, 1, seed=1), predictor_batch(7, 12, 5, seed=3), predictor_batch(1, 3, 2, seed=5)):
        one = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        try:
            hip_predictor.set_tuning("dec_cls_side", 1)
            two = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        finally:
            hip_predictor.set_tuning("dec_cls_side", 0)
        for k in ("cls", "reg", "vel"):
            assert torch.equal(two[k], one[k]), k


def test_decoder_scene_part_on_eight_workgroups_equals_the_one_workgroup_kernel(hip_predictor):
    """With mind_set_tuning("dec_mw", 1) calls of at most n_cu / 8 scenes run k_dec_scene_mw: eight workgroups per scene share the decoder's
    five big stages with the K split and per-item arithmetic of the one-workgroup kernel (opt-in: 6 us of a 95 us launch).  Every output
    must be the same bits: lone scenes, ragged batches, and a batch too big for the resident form (which then takes the one-workgroup
    kernel by itself)."""
    for pb in (predictor_batch(40, 55, 1, seed=1), predictor_batch(7, 12, 5, seed=3), predictor_batch(1, 3, 2, seed=5), predictor_batch(3, 5, 32, seed=7),
               predictor_batch(2, 4, 40, seed=9)):
        one = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        try:
            hip_predictor.set_tuning("dec_mw", 1)
            mw = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        finally:
            hip_predictor.set_tuning("dec_mw", 0)
        for k in ("cls", "reg", "vel"):
            assert torch.equal(mw[k], one[k]), k


def test_token_kernel_of_big_scenes_on_the_bf16_split_mfma(hip_predictor, formula_sd):
    """With mind_set_tuning("tok_bf_min_n", 256) scenes of >= 256 tokens run their per-token epilogue / prologue on k_token_mfma<1> (bf16
    hi + lo split operands, the pair kernel's arithmetic): against the oracle at the cfg4 scene size, against the VALU kernel it
    replaces there, and -- the kernel is chosen scene by scene -- a big scene's result is the same bits whether it is predicted alone
    or in a batch with a small scene (which keeps the VALU kernel)."""
    big = predictor_batch(64, 256, 1, seed=21)
    small = predictor_batch(9, 21, 1, seed=2)
    oc, orr, ov = op.forward(formula_sd, to_t(big))
    before = hip_predictor.pair_precision()
    hip_predictor.set_pair_precision("bf16x3")                 # (the two-way split token kernel belongs to the two-way split arithmetic: never chosen under bf16x6 / f32)
    valu = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(big).items() if torch.is_tensor(v)}
    try:
        hip_predictor.set_tuning("tok_bf_min_n", 256)          # (opt-in: measured no faster than the VALU kernel at this size)
        out = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(big).items() if torch.is_tensor(v)}
        alone_small = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(small).items() if torch.is_tensor(v)}
        _mixed_check(hip_predictor, small, big, alone_small, out)
    finally:
        hip_predictor.set_tuning("tok_bf_min_n", 0)
        hip_predictor.set_pair_precision(before)
    assert np.abs(out["reg"].cpu().numpy() - orr[0].numpy()).max() < TOL and np.abs(out["vel"].cpu().numpy() - ov[0].numpy()).max() < TOL
    assert (out["reg"] - valu["reg"]).abs().max().item() < 1e-4           # (both are within TOL of the oracle; observed 3e-5 .. 5e-5)
    assert not torch.equal(out["reg"], valu["reg"])                      # it really was the other kernel


def _mixed_check(hip_predictor, small, big, alone_small, out):
    # mixed batch: [small scene, big scene] -> two token launches per layer, the big scene's bits unchanged
    mixed = {"ACTORS": np.concatenate([small["ACTORS"], big["ACTORS"]]), "LANES": np.concatenate([small["LANES"], big["LANES"]]),
             "ACTOR_IDCS": [np.arange(9), np.arange(9, 73)], "LANE_IDCS": [np.arange(21), np.arange(21, 277)],
             "CTRS": small["CTRS"] + big["CTRS"], "VECS": small["VECS"] + big["VECS"],
             "TGT_NODES": np.concatenate([small["TGT_NODES"], big["TGT_NODES"]]), "TGT_RPE": np.concatenate([small["TGT_RPE"], big["TGT_RPE"]])}
    both = hip_predictor.predict_numpy_batch(mixed)
    assert torch.equal(both["reg"][:9], alone_small["reg"]) and torch.equal(both["reg"][9:], out["reg"])
    assert torch.equal(both["cls"][0], alone_small["cls"][0]) and torch.equal(both["cls"][1], out["cls"][0])


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("a,l,B,seed", [(1, 1, 1, 5), (16, 15, 3, 2), (17, 30, 3, 4), (40, 55, 2, 1), (64, 256, 1, 21), (64, 256, 9, 22), (40, 1000, 1, 23),
                                        (15, 239, 1, 24), (16, 239, 2, 25), (17, 239, 1, 26)])
def test_tile_native_pair_kernel_equals_the_row_major_one(prec, a, l, B, seed, hip_predictor):
    """k_pair_t (edge tensor in 8 KB tile chunks of the MFMA C/D layout, next tile and its T rows requested across job boundaries, folded
    query in registers: the default under the bf16 arithmetics) against k_pair_bf (row-major tensor through LDS staging: rounds 2-3,
    mind_set_tuning("pair_tile", 0)).  bf16x3: the same contractions, the same summation orders -- the same bits (N = 3, 32, 48, 96, 321:
    one-tile columns, whole tiles, ragged last tiles, split columns).  Plain bf16: k_pair_t keeps the edge tensor in bf16 too, so the two
    differ by that rounding (both are 6e-3 .. 3e-2 away from the oracle).  Nine scenes of N = 321: more jobs than wave slots, dealt over XCD lanes
    whose cuts fall inside scenes (pair_jobs.h); N = 1041: eight partials per column, 66 tiles; N = 255, 256, 257: either side of the size from
    which a column is cut into jobs of about seven tiles."""
    pb = predictor_batch(a, l, B, seed=seed)
    before = hip_predictor.pair_precision()
    try:
        hip_predictor.set_pair_precision(prec)
        hip_predictor.set_tuning("pair_tile", 0)
        ref = {k: v.clone() for k, v in hip_predictor.predict_numpy_batch(pb).items() if torch.is_tensor(v)}
        hip_predictor.set_tuning("pair_tile", 1)
        out = hip_predictor.predict_numpy_batch(pb)
    finally:
        hip_predictor.set_tuning("pair_tile", 1)
        hip_predictor.set_pair_precision(before)
    for k in ("cls", "reg", "vel"):
        assert torch.isfinite(out[k]).all()
        if prec == "bf16x3":
            assert torch.equal(out[k], ref[k]), k
        else:
            assert (out[k] - ref[k]).abs().max().item() < 3e-2, k
    if prec == "bf16":
        assert not torch.equal(out["reg"], ref["reg"])          # it really was the other kernel


@pytest.mark.parametrize("a,l,B,seed", [(5, 1, 2, 5), (17, 30, 2, 4)])
def test_tile_native_edge_tensor_equals_the_oracles(a, l, B, seed, hip_predictor, formula_sd):
    """The edge tensor after every updating fusion layer, read back through mind_debug_read (which un-permutes the tile-native
    layout to [scene][j][i][128]), against the oracle's (network.py:201-202) -- pins the layout algebra of k_pair_t's loads and stores
    on ragged scenes (N = 7, 48)."""
    pb = predictor_batch(a, l, B, seed=seed)
    taps = {}
    op.forward(formula_sd, to_t(pb), taps=taps)
    n = a + l + 1
    try:
        for k in (1, 3, 5):
            hip_predictor.debug_set_layers(k)
            hip_predictor.predict_numpy_batch(pb)
            e = hip_predictor.debug_read("edge").reshape(B, n, n, 128).transpose(0, 2, 1, 3)      # -> the reference's [i][j]
            for b in range(B):
                d = np.abs(e[b] - taps["fusion"][b][k - 1][1].numpy())
                if k == 5:
                    d = d[:, list(range(a)) + [n - 1]]      # layer 4 updates the consumed columns only
                assert d.max() < 2e-4, (k, b, d.max())
    finally:
        hip_predictor.debug_set_layers(6)


@pytest.mark.parametrize("knobs,restore", [({}, {}), ({"tok_mfma": 1}, {"tok_mfma": 0}), ({"actor_f32_min": 0}, {"actor_f32_min": 1 << 30})])
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "bf16x6"])
@pytest.mark.parametrize("a,l,B", [(3, 4, 1), (17, 30, 3)])
def test_launches_are_the_ones_pred_choose_records(a, l, B, prec, knobs, restore, hip_predictor):
    """What a call launched (mind_last_actor_stats, mind_last_token_stats, mind_last_fusion_stats) against the record of pred_choose for the
    same knobs, arithmetic and scene sizes on this device's CU count (mind_debug_predict_choice: the function mind_predict_batch decides with)."""
    from mind_amd._lib import predict_choice
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    d = predict_choice(knobs, prec, [(a, l)] * B, n_cu=n_cu)
    before = hip_predictor.pair_precision()
    try:
        hip_predictor.set_pair_precision(prec)
        for k, v in knobs.items():
            hip_predictor.set_tuning(k, v)
        out = hip_predictor.predict_numpy_batch(predictor_batch(a, l, B, seed=4))
        actor, tok, fusion = hip_predictor.last_actor_stats(), hip_predictor.last_token_stats(), hip_predictor.fusion_stats()
    finally:
        for k, v in restore.items():
            hip_predictor.set_tuning(k, v)
        hip_predictor.set_pair_precision(before)
    assert torch.isfinite(out["reg"]).all()
    assert (actor["layerwise"], actor["launches"], actor["chunks"]) == (int(d["actor_form"] == 3), d["actor_launches"], d["actor_chunks"]) == (0, 1, 1)
    assert d["actor_form"] == (1 if prec == "f32" or "actor_f32_min" in knobs else 2)
    assert (tok["layerwise"], tok["launches"], tok["chunks"]) == (d["tok_lw"], 7 * d["n_runs"], d["tok_chunks"]) == (0, 7, 0)
    assert d["runs"] == [(0, B * (a + l + 1), int("tok_mfma" in knobs), 0, int("tok_mfma" not in knobs), int("tok_mfma" not in knobs))]
    assert fusion[0] == 6
