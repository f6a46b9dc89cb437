"""Which kernels a mind_predict_batch call runs, checked on the host -- no GPU needed.

mind_predict_batch decides once per call, in pred_choose (mind_amd/csrc/pred_choice.h), and its stages switch on that record;
mind_debug_predict_choice returns the record for a set of knobs, an arithmetic and a batch of scene sizes.  Most forms are bit-identical
to each other by design, so a wrong selection changes no result, only speed: these are the selection rules themselves, as the ladders of
the one-function mind_predict_batch had them.  n_cu is 256 and the side stream present unless a case says otherwise; a scene (a, l) has
N = a + l + 1 tokens."""
import pytest

from mind_amd._lib import predict_choice

VALU, F32, MFMA, LW = 0, 1, 2, 3                     # ActorNet form
K_PAIR, K_PAIR_BF, K_PAIR_T, K_PAIR_T6 = 0, 1, 2, 3  # pair-kernel family
DEC_ONE, DEC_SPLIT, DEC_MFMA = 0, 1, 2               # decoder actor part
ONE = [(3, 4)]
PRECS = ("f32", "bf16x3", "bf16", "bf16x6")


def scenes_of(*tokens):
    return [(1, n - 2) for n in tokens]


@pytest.mark.parametrize("prec,knobs,want", [
    ("bf16x6", {}, (MFMA, 6, 3)), ("bf16", {}, (MFMA, 1, 3)), ("bf16x3", {}, (MFMA, 6, 3)), ("bf16x3", {"actor_split": 3}, (MFMA, 3, 3)),
    ("f32", {}, (F32, 1, 3)), ("f32", {"actor_f32": 0}, (VALU, 0, 3)), ("f32", {"enc_mfma": 0}, (VALU, 0, 3)), ("bf16x3", {"enc_mfma": 0}, (VALU, 0, 3)),
    ("bf16x6", {"actor_f32_min": 2}, (F32, 2, 2)), ("f32", {"actor_f32_min": 2}, (F32, 1, 3)), ("f32", {"actor_f32_pair_min": 2}, (F32, 2, 2)),
    ("bf16x6", {"actor_lw_min": 2, "actor_f32_min": 2}, (F32, 2, 2)), ("f32", {"actor_lw_min": 2}, (F32, 1, 3))])
def test_actor_net_form(prec, knobs, want):
    d = predict_choice(knobs, prec, ONE)
    assert (d["actor_form"], d["actor_arg"], d["actor_grid"]) == want
    assert (d["actor_launches"], d["actor_chunks"]) == (1, 1)


@pytest.mark.parametrize("prec,np_", [("bf16x6", 6), ("bf16x3", 6), ("bf16", 1)])
def test_actor_net_layerwise(prec, np_):
    d = predict_choice({"actor_lw_min": 2}, prec, ONE)
    assert (d["actor_form"], d["actor_arg"], d["np"], d["actor_chunk"], d["actor_chunks"]) == (LW, np_, np_, 1024, 1)
    d = predict_choice({"actor_lw_min": 2, "actor_lw_chunk": 2}, prec, [(3, 4), (2, 0)])
    assert (d["actor_form"], d["actor_chunk"], d["actor_chunks"]) == (LW, 2, 3)                 # ceil(5 / 2)
    assert d["actor_launches"] == 3 * (1 + 2 * 26)                                              # per chunk the split, conv + GroupNorm of 26 stages
    assert predict_choice({"actor_lw_min": 4}, prec, ONE)["actor_form"] == MFMA                 # 3 actors: below the threshold
    assert predict_choice({"actor_lw_min": 2, "actor_split": 3}, "bf16x3", ONE)["actor_arg"] == 3


def test_token_runs_defaults_and_valu_forms():
    for prec in PRECS:
        assert predict_choice({}, prec, ONE)["runs"] == [(0, 8, 0, 0, 1, 1)]
        assert predict_choice({"tok_merge": 0}, prec, ONE)["runs"] == [(0, 8, 0, 0, 1, 0)]
    # the test against tok_small_max is on the RUN, <=
    assert predict_choice({}, "bf16x6", scenes_of(1024, 1024))["runs"] == [(0, 2048, 0, 0, 1, 1)]
    assert predict_choice({}, "bf16x6", scenes_of(1024, 1025))["runs"] == [(0, 2049, 0, 0, 0, 0)]
    assert predict_choice({"tok_small_max": 7}, "bf16x6", ONE)["runs"] == [(0, 8, 0, 0, 0, 0)]
    assert predict_choice({"tok_small_max": 8}, "bf16x6", ONE)["runs"] == [(0, 8, 0, 0, 1, 1)]


def test_token_classes_by_scene():
    two = scenes_of(8, 48)
    for prec in PRECS:
        for other in ({}, {"tok_bf_min_n": 40}, {"tok_lw_min_n": 40, "tok_lw_min": 0}):
            assert predict_choice({"tok_mfma": 1, **other}, prec, two)["runs"] == [(0, 56, 1, int(other.get("tok_lw_min", 1) == 0), 0, 0)]
    for prec in ("bf16x3", "bf16"):
        assert predict_choice({"tok_bf_min_n": 40}, prec, two)["runs"] == [(0, 8, 0, 0, 1, 1), (8, 48, 2, 0, 0, 0)]
        assert predict_choice({"tok_bf_min_n": 40, "tok_lw_min_n": 40}, prec, two)["runs"][1][2] == 2       # kind 2 wins
    for prec in ("bf16x6", "f32"):
        assert predict_choice({"tok_bf_min_n": 40}, prec, two)["runs"] == [(0, 56, 0, 0, 1, 1)]
    assert predict_choice({"tok_bf_min_n": 0}, "bf16x3", two)["runs"] == [(0, 56, 0, 0, 1, 1)]               # 0 = never


def test_token_layerwise_runs():
    four = scenes_of(8, 48, 48, 8)
    d = predict_choice({"tok_lw_min_n": 40}, "bf16x6", four)
    assert d["runs"] == [(0, 8, 0, 0, 1, 1), (8, 96, 1, 0, 0, 0), (104, 8, 0, 0, 1, 1)]
    assert (d["tok_lw"], d["tok_chunks"]) == (0, 0)
    d = predict_choice({"tok_lw_min_n": 40, "tok_lw_min": 96, "tok_lw_chunk": 48}, "bf16x6", four)
    assert [r[3] for r in d["runs"]] == [0, 1, 0] and (d["tok_lw"], d["tok_chunks"], d["tok_chunk"]) == (1, 2, 48)
    d = predict_choice({"tok_lw_min_n": 40, "tok_lw_min": 96, "tok_lw_chunk": 50}, "bf16x6", four)
    assert d["tok_chunks"] == 2                                                                            # ceil(96 / 50)
    d = predict_choice({"tok_lw_min_n": 40, "tok_lw_min": 96}, "bf16x6", four)
    assert (d["tok_chunks"], d["tok_chunk"]) == (1, 32768)
    d = predict_choice({"tok_lw_min_n": 40, "tok_lw_min": 97}, "bf16x6", four)
    assert [r[3] for r in d["runs"]] == [0, 0, 0] and (d["tok_lw"], d["tok_chunks"]) == (0, 0)
    # two layer-wise runs: the chunks of both
    d = predict_choice({"tok_lw_min_n": 40, "tok_lw_min": 48, "tok_lw_chunk": 32}, "f32", scenes_of(48, 8, 48, 48))
    assert [r[:4] for r in d["runs"]] == [(0, 48, 1, 1), (48, 8, 0, 0), (56, 96, 1, 1)] and d["tok_chunks"] == 2 + 3


@pytest.mark.parametrize("prec,qsplit,qk_stride", [("bf16x6", 48, 1536), ("bf16x3", 16, 1024), ("bf16", 16, 1024), ("f32", 0, 1024)])
def test_query_format(prec, qsplit, qk_stride):
    d = predict_choice({}, prec, ONE)
    assert (d["qsplit"], d["qk_stride"]) == (qsplit, qk_stride)


@pytest.mark.parametrize("prec,knobs,want", [
    # family, parts, tiled, bf16 edge tensor, bytes per pair, layer 5 on jobs5
    ("f32", {}, (K_PAIR, 0, 0, 0, 512, 0)), ("f32", {"pair_tile": 0}, (K_PAIR, 0, 0, 0, 512, 0)),
    ("bf16x6", {}, (K_PAIR_T6, 0, 1, 0, 512, 1)), ("bf16x6", {"pair_tile": 0}, (K_PAIR_T6, 0, 1, 0, 512, 1)),
    ("bf16x3", {}, (K_PAIR_T, 3, 1, 0, 512, 1)), ("bf16", {}, (K_PAIR_T, 1, 1, 1, 256, 1)),
    ("bf16x3", {"pair_tile": 0}, (K_PAIR_BF, 3, 0, 0, 512, 0)), ("bf16", {"pair_tile": 0}, (K_PAIR_BF, 1, 0, 0, 512, 0))])
def test_pair_kernel(prec, knobs, want):
    d = predict_choice(knobs, prec, ONE)
    assert (d["pair_family"], d["pair_np"], d["tiled"], d["edge_bf16"], d["edge_pair_bytes"], d["l5_jobs5"]) == want


def test_xcd_grouping_factor():
    big = [(64, 256)] * 8                                   # N = 321: three jobs per column, far more jobs than compute units
    assert predict_choice({}, "bf16x6", big)["xcd_lanes"] == 8 and predict_choice({}, "bf16x6", big)["xcd_lanes5"] == 8
    assert predict_choice({"xcd_order": 0}, "bf16x6", big)["xcd_lanes"] == 1
    assert predict_choice({}, "bf16x6", big[:7])["xcd_lanes"] == 1                       # fewer than eight scenes
    assert predict_choice({}, "bf16x6", big, n_cu=252)["xcd_lanes"] == 1                 # a grid that is no multiple of 8
    # eight scenes of 3 tokens (one tile: one job a column): 24 jobs = the grid, divisible by 8, and 16 jobs on the consumed columns; 9 scenes: 27 jobs
    tiny = [(1, 1)] * 8
    assert (predict_choice({}, "bf16x6", tiny)["xcd_lanes"], predict_choice({}, "bf16x6", tiny)["xcd_lanes5"]) == (8, 8)
    assert predict_choice({}, "bf16x6", [(1, 1)] * 9)["xcd_lanes"] == 1


def test_decoder_actor_part():
    for prec in PRECS:
        d = predict_choice({}, prec, ONE)
        assert (d["dec_actor"], d["split_dec"], d["fp32_dec"], d["dec_np"]) == (DEC_SPLIT, 1, 1, 0)
        assert predict_choice({"dec_overlap": 0}, prec, ONE)["dec_actor"] == DEC_ONE
        assert predict_choice({}, prec, ONE, have_side=False)["dec_actor"] == DEC_ONE
    for prec, knobs, np_ in (("bf16x6", {}, 6), ("bf16x3", {}, 6), ("bf16", {}, 1), ("bf16x3", {"actor_split": 3}, 3)):
        d = predict_choice({"dec_mfma_min": 0, **knobs}, prec, ONE)
        assert (d["dec_actor"], d["dec_np"], d["split_dec"], d["fp32_dec"]) == (DEC_MFMA, np_, 0, 0)
    assert predict_choice({"dec_mfma_min": 3}, "bf16x6", ONE)["dec_actor"] == DEC_MFMA       # 3 agents: at the threshold
    assert predict_choice({"dec_mfma_min": 4}, "bf16x6", ONE)["dec_actor"] == DEC_SPLIT
    assert predict_choice({"dec_mfma_min": 0}, "f32", ONE)["dec_actor"] == DEC_SPLIT
    assert predict_choice({"dec_mfma_min": 0, "enc_mfma": 0}, "bf16x6", ONE)["dec_actor"] == DEC_SPLIT


def test_decoder_scene_part():
    d = predict_choice({}, "bf16x6", ONE)
    assert (d["want_mw"], d["cls_on_side"]) == (0, 0)
    for n, blocks, want in ((1, 64, 1), (32, 256, 1), (33, 320, 0)):
        d = predict_choice({"dec_mw": 1}, "bf16x6", ONE * n)
        assert (d["mw_blocks"], d["want_mw"]) == (blocks, want)
    assert predict_choice({"dec_mw": 1}, "bf16x6", ONE, n_cu=32)["want_mw"] == 0
    assert predict_choice({"dec_cls_side": 1}, "bf16x6", ONE)["cls_on_side"] == 1
    assert predict_choice({"dec_cls_side": 1, "dec_overlap": 0}, "bf16x6", ONE)["cls_on_side"] == 0
    assert predict_choice({"dec_cls_side": 1}, "bf16x6", ONE, have_side=False)["cls_on_side"] == 0
    assert predict_choice({"dec_cls_side": 1, "dec_mfma_min": 0}, "bf16x6", ONE)["cls_on_side"] == 0        # (no split form under the MFMA actor part)
    d = predict_choice({"dec_cls_side": 1, "dec_mw": 1}, "bf16x6", ONE)
    assert (d["want_mw"], d["cls_on_side"]) == (1, 0)
    assert predict_choice({"dec_cls_side": 1, "dec_mw": 1}, "bf16x6", ONE * 33)["cls_on_side"] == 1         # mw not possible: the two-launch form


def test_target_embedding_fence():
    assert predict_choice({}, "bf16x6", ONE)["tgt_wait_first"] == 0
    assert predict_choice({"tgt_side": 0}, "bf16x6", ONE)["tgt_wait_first"] == 1
    assert predict_choice({"tgt_side": 0}, "bf16x6", ONE, have_side=False)["tgt_wait_first"] == 0


def test_rejects_and_truncation():
    assert predict_choice({"no_such_knob": 1}, "bf16x6", ONE) is None
    assert predict_choice({"ilqr_wgs": 8}, "bf16x6", ONE) is None            # a knob of the context, not of the predictor
    assert predict_choice({}, 4, ONE) is None and predict_choice({}, -1, ONE) is None
    assert predict_choice({}, "bf16x6", [(3, 4), (0, 4)]) is None
    assert predict_choice({}, "bf16x6", [(3, -1)]) is None
    import ctypes as C
    from mind_amd import _lib
    lib = _lib.load()
    sa, sl, out = (C.c_int * 1)(3), (C.c_int * 1)(4), (C.c_longlong * 4)(-7, -7, -7, -7)
    assert lib.mind_debug_predict_choice(None, None, 0, 3, 256, 1, sa, sl, 1, out, 3) == 38     # the full record's length
    assert list(out) == [32, 1, 6, -7]                                                          # ... of which cap were written
    assert lib.mind_debug_predict_choice(None, None, 0, 3, 256, 1, None, sl, 1, out, 3) == _lib.MIND_EINVAL
    assert lib.mind_debug_predict_choice(None, None, 0, 3, 256, 1, sa, sl, 1, None, 3) == _lib.MIND_EINVAL
