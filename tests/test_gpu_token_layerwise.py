"""GPU: the layer-wise token stage (mind_amd/csrc/token_lw_kernels.hip; mind_set_tuning "tok_lw_min_n" / "tok_lw_min" / "tok_lw_chunk")
against the kernel whose arithmetic it repeats, k_token_mfma<0> ("tok_mfma" 1).  The path restates nothing -- every projection is
tm_mma<0>'s MFMA sequence per output element, the LayerNorms are tm_layernorm itself, the merge and the QK packing are the same
expressions -- so the requirement is BIT-identity: every output and the x / ST / QK taps, in the three QK formats, for ragged tiles,
several chunks, every position in a batch, mixed batches and a whole plan."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from mind_amd import _lib
from mind_amd.synth import predictor_batch
from oracle import predictor as op
from test_gpu_predictor import TOL, to_t          # the file-level parity bar of tests/test_gpu_predictor.py (no new constant)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 1 << 30
OUTS = ("cls", "reg", "vel")
TAPS = ("x", "ST", "QK")
QBITS = {"bf16x6": 48, "bf16x3": 16, "bf16": 16, "f32": 0}

# the smallest batch in which a token has nsplit > 1: mind_debug_pair_schedule gives the columns of a scene of N <= 16 tokens one partial
# slot and those of N = 17 two (N = 31: 2, 48: 3, 96: 6, 321: 3 -- so the batches above it split too); checked on the CPU by
# test_the_split_batch_really_has_split_columns below.  (64, 256, 1, 21) is the cfg4 scene size.
SPLIT_BATCH = (1, 15, 1, 5)
BATCHES = [(3, 4, 1, 1), (9, 21, 5, 2), (17, 30, 3, 4), (40, 55, 1, 1), SPLIT_BATCH, (64, 256, 1, 21)]


def _restore(hp, prec):
    hp.set_tuning("tok_mfma", 0)
    hp.set_tuning("tok_lw_min_n", NEVER)
    hp.set_tuning("tok_lw_min", NEVER)
    hp.set_tuning("tok_lw_chunk", 0)
    hp.set_pair_precision(prec)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(hp, pb, tok_mfma=0, min_n=NEVER, lw_min=NEVER, chunk=0, taps=True):
    hp.set_tuning("tok_mfma", tok_mfma)
    hp.set_tuning("tok_lw_min_n", min_n)
    hp.set_tuning("tok_lw_min", lw_min)
    hp.set_tuning("tok_lw_chunk", chunk)
    o = hp.predict_numpy_batch(pb)
    r = {k: o[k].cpu().numpy().copy() for k in OUTS}
    if taps:
        for k in TAPS:
            r[k] = hp.debug_read(k).copy()
    return r, hp.last_token_stats()


def _same(a, b, keys=OUTS + TAPS):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (k, int((_bits(a[k]) != _bits(b[k])).sum()))


def _planned_launches(n_tokens, prec, chunk=0):
    """what the host plan predicts for the seven token steps of one predictor call whose scenes form one layer-wise run"""
    lib = _lib.load()
    info = np.zeros(4, np.int64)
    q = QBITS[prec]
    n = [lib.mind_debug_token_lw_plan(n_tokens, m | q, chunk, None, 0, info.ctypes.data_as(C.POINTER(C.c_longlong))) for m in [1 | 4] + [2 | 4] * 5 + [2 | 8]]
    assert min(n) > 0
    return sum(n)


def _cat(scenes):
    """single-scene predictor_batch dicts -> one batch"""
    na = np.cumsum([0] + [len(s["ACTORS"]) for s in scenes])
    nl = np.cumsum([0] + [len(s["LANES"]) for s in scenes])
    return {"ACTORS": np.concatenate([s["ACTORS"] for s in scenes]), "LANES": np.concatenate([s["LANES"] for s in scenes]),
            "ACTOR_IDCS": [np.arange(na[i], na[i + 1]) for i in range(len(scenes))], "LANE_IDCS": [np.arange(nl[i], nl[i + 1]) for i in range(len(scenes))],
            "CTRS": [s["CTRS"][0] for s in scenes], "VECS": [s["VECS"][0] for s in scenes],
            "TGT_NODES": np.concatenate([s["TGT_NODES"] for s in scenes]), "TGT_RPE": np.concatenate([s["TGT_RPE"] for s in scenes])}


def _scene_rows(r, a0, a1, b):
    return {"cls": r["cls"][b], "reg": r["reg"][a0:a1], "vel": r["vel"][a0:a1]}


def test_the_split_batch_really_has_split_columns():
    """(host part of the bit-identity test's batches) N = 17 is the smallest scene whose columns get more than one partial slot."""
    lib = _lib.load()

    def jobs_per_column(N):
        out, info = np.zeros((N * 8, 6), np.int32), np.zeros(4, np.int32)
        n = lib.mind_debug_pair_schedule(np.array([N], np.int32).ctypes.data_as(C.POINTER(C.c_int)), np.array([1], np.int32).ctypes.data_as(C.POINTER(C.c_int)),
                                         1, 256, 0, out.ctypes.data_as(C.POINTER(C.c_int)), N * 8, info.ctypes.data_as(C.POINTER(C.c_int)))
        assert n > 0
        return int(info[0])
    a, l, B, _ = SPLIT_BATCH
    assert B == 1 and jobs_per_column(a + l + 1) > 1
    assert all(jobs_per_column(N) == 1 for N in range(2, a + l + 1))
    assert [jobs_per_column(N) for N in (31, 48, 96, 321)] == [2, 3, 6, 3]


@pytest.fixture(scope="module")
def default_before(hip_predictor):
    """the default path before this module touches any of its knobs (test_defaults_... compares against it at the end)"""
    pbs = {b: predictor_batch(*b[:3], seed=b[3]) for b in ((9, 21, 5, 2), (40, 55, 1, 1))}
    return {b: _run(hip_predictor, pb, taps=False)[0] for b, pb in pbs.items()}, pbs


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x3", "f32"])
@pytest.mark.parametrize("a,l,B,seed", BATCHES)
def test_bit_identical_to_the_fp32_mfma_token_kernel(prec, a, l, B, seed, hip_predictor, default_before):
    hp = hip_predictor
    pb = predictor_batch(a, l, B, seed=seed)
    ntok = (a + l + 1) * B
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        valu, st_v = _run(hp, pb)
        want, st0 = _run(hp, pb, tok_mfma=1)
        got, st1 = _run(hp, pb, min_n=0, lw_min=0)
    finally:
        _restore(hp, before)
    assert st_v["layerwise"] == 0 and st0["layerwise"] == 0 and st0["launches"] == 7 and st0["chunks"] == 0
    assert st1["layerwise"] == 1 and st1["chunks"] == 1 and st1["launches"] == _planned_launches(ntok, prec) == 3 + 5 * 6 + 4
    assert np.isfinite(want["reg"]).all() and np.abs(want["reg"]).max() > 0.1
    _same(got, want)
    assert not (np.array_equal(got["reg"], valu["reg"]) and np.array_equal(got["x"], valu["x"]))      # it really was another kernel than the default


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x3", "f32"])
def test_bit_identical_over_several_chunks_with_a_ragged_last_one(prec, hip_predictor, default_before):
    """155 tokens in chunks of 48: three whole chunks and one of 11 through the same arena; scenes of 31 tokens straddle tiles and chunks."""
    hp = hip_predictor
    pb = predictor_batch(9, 21, 5, seed=2)
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        want, _ = _run(hp, pb, tok_mfma=1)
        one, s1 = _run(hp, pb, min_n=0, lw_min=0)
        got, s4 = _run(hp, pb, min_n=0, lw_min=0, chunk=48)
        odd, s7 = _run(hp, pb, min_n=0, lw_min=0, chunk=7)          # ... and chunks that are no multiple of a tile
        neg, sn = _run(hp, pb, min_n=0, lw_min=0, chunk=-5)         # a negative chunk means the default
    finally:
        _restore(hp, before)
    assert s1["chunks"] == 1 and s4["chunks"] == 4 and s7["chunks"] == 23 and sn["chunks"] == 1
    assert s4["launches"] == _planned_launches(155, prec, 48) == 4 * 37
    _same(got, want)
    _same(one, want)
    _same(odd, want)
    _same(neg, want)


def test_a_scene_is_the_same_bits_alone_first_and_last_in_a_batch(hip_predictor, default_before):
    hp = hip_predictor
    s = predictor_batch(9, 21, 1, seed=7)
    others = [predictor_batch(9, 21, 1, seed=30 + k) for k in range(4)]
    before = hp.pair_precision()
    try:
        alone, _ = _run(hp, s, min_n=0, lw_min=0, taps=False)
        first, _ = _run(hp, _cat([s] + others), min_n=0, lw_min=0, taps=False)
        last, st = _run(hp, _cat(others + [s]), min_n=0, lw_min=0, taps=False)
    finally:
        _restore(hp, before)
    assert st["layerwise"] == 1
    _same(_scene_rows(alone, 0, 9, 0), _scene_rows(first, 0, 9, 0), OUTS)
    _same(_scene_rows(alone, 0, 9, 0), _scene_rows(last, 36, 45, 4), OUTS)
    _same(_scene_rows(first, 9, 45, slice(1, 5)), _scene_rows(last, 0, 36, slice(0, 4)), OUTS)      # ... and so are the others


def test_scenes_below_and_above_the_scene_threshold_in_one_batch(hip_predictor, default_before):
    """tok_lw_min_n = 32: the scene of 8 tokens keeps the VALU kernel, the scene of 48 takes the fp32-MFMA class and runs layer-wise -- two
    kinds of runs in one call (three runs here), and every scene gets the bits it gets alone."""
    hp = hip_predictor
    small, big = predictor_batch(3, 4, 1, seed=1), predictor_batch(17, 30, 1, seed=4)
    before = hp.pair_precision()
    try:
        s_def, _ = _run(hp, small, taps=False)
        s_alone, st_s = _run(hp, small, min_n=32, lw_min=0, taps=False)
        b_alone, st_b = _run(hp, big, min_n=32, lw_min=0, taps=False)
        b_mfma, _ = _run(hp, big, tok_mfma=1, taps=False)
        mixed, st_m = _run(hp, _cat([small, big, small]), min_n=32, lw_min=0, taps=False)
    finally:
        _restore(hp, before)
    assert st_s["layerwise"] == 0 and st_b["layerwise"] == 1 and st_m["layerwise"] == 1
    assert st_m["launches"] == 7 * 2 + 37 and st_m["chunks"] == 1
    _same(s_alone, s_def, OUTS)
    _same(b_alone, b_mfma, OUTS)
    _same(_scene_rows(mixed, 0, 3, 0), _scene_rows(s_alone, 0, 3, 0), OUTS)
    _same(_scene_rows(mixed, 3, 20, 1), _scene_rows(b_alone, 0, 17, 0), OUTS)
    _same(_scene_rows(mixed, 20, 23, 2), _scene_rows(s_alone, 0, 3, 0), OUTS)


def test_short_runs_keep_the_one_kernel_form(hip_predictor, default_before):
    """tok_lw_min_n = 0 puts every scene in the fp32-MFMA class; with tok_lw_min above the batch's token count the run stays on
    k_token_mfma<0> -- and the bits do not move."""
    hp = hip_predictor
    pb = predictor_batch(17, 30, 3, seed=4)
    before = hp.pair_precision()
    try:
        want, _ = _run(hp, pb, tok_mfma=1)
        got, st = _run(hp, pb, min_n=0, lw_min=3 * 48 + 1)
        lw, st_lw = _run(hp, pb, min_n=0, lw_min=3 * 48)
    finally:
        _restore(hp, before)
    assert st["layerwise"] == 0 and st["launches"] == 7 and st["chunks"] == 0 and st_lw["layerwise"] == 1
    _same(got, want)
    _same(lw, want)


@pytest.mark.parametrize("a,l,B,seed", [(9, 21, 5, 2), (40, 55, 1, 1)])
def test_wired_to_the_right_weights(a, l, B, seed, hip_predictor, formula_sd, default_before):
    """k_token_mfma<0> meets the parity bar of tests/test_gpu_predictor.py already; this guards the wiring of the seven steps."""
    hp = hip_predictor
    pb = predictor_batch(a, l, B, seed=seed)
    _, orr, ov = op.forward(formula_sd, to_t(pb))
    before = hp.pair_precision()
    try:
        got, st = _run(hp, pb, min_n=0, lw_min=0, taps=False)
    finally:
        _restore(hp, before)
    assert st["layerwise"] == 1
    for b in range(B):
        er, ev = np.abs(got["reg"][b * a:(b + 1) * a] - orr[b].numpy()).max(), np.abs(got["vel"][b * a:(b + 1) * a] - ov[b].numpy()).max()
        print(f"layer-wise token stage a{a}_l{l}_b{B}_s{seed} scene {b}: max|reg - oracle| = {er:.3e}, max|vel - oracle| = {ev:.3e}")
        assert er < TOL and ev < TOL


def test_the_knobs_and_the_profiled_times(hip_predictor, default_before):
    """mind_set_tuning takes the three names (it needs a context, so this lives here); with profiling on the stats carry the summed launch
    times, by stage for the layer-wise form."""
    hp = hip_predictor
    pb = predictor_batch(17, 30, 3, seed=4)
    before = hp.pair_precision()
    with pytest.raises(_lib.MindError):
        hp.set_tuning("tok_lw_no_such_knob", 1)
    try:
        hp.set_profiling(True)
        _, st0 = _run(hp, pb, taps=False)
        _, st1 = _run(hp, pb, min_n=0, lw_min=0, taps=False)
    finally:
        hp.set_profiling(False)
        _restore(hp, before)
    assert st0["layerwise"] == 0 and st0["ms"] > 0 and st0["stage_ms"][7] == pytest.approx(st0["ms"], rel=1e-3) and sum(st0["stage_ms"][:7]) == 0
    assert st1["layerwise"] == 1 and st1["ms"] > 0 and all(v > 0 for v in st1["stage_ms"][:7]) and st1["stage_ms"][7] == 0
    assert sum(st1["stage_ms"]) == pytest.approx(st1["ms"], rel=1e-3)


def _plan_tables(pl):
    gen = pl.scen_tree_gen
    nodes = [(k, n.parent_key, int(n.data.data["CUR_T"]) if n.data.data is not None else -1, int(n.data.data["END_T"]) if n.data.data is not None else -1,
              bool(n.data.branch_flag), bool(n.data.end_flag), bool(n.data.terminate_flag)) for k, n in gen.tree.nodes.items()]
    rows = [(k, n.parent_key) + tuple(np.asarray(n.data[i]).copy() for i in range(4)) for t in gen.get_scenario_tree() for k, n in t.nodes.items()]
    flats = [{k: np.asarray(t._flat[k]).copy() for k in ("parent", "prob", "mean", "cov")} for t in gen.last_trees]
    return nodes, rows, flats


def test_a_whole_plan_is_the_same_with_either_form():
    """One cycle of the recorded demo_1 scene through mind_aime_plan on one rank: with k_token_mfma<0> and with the layer-wise kernels
    the node table, the returned rows and the flattened cost trees are the same bits."""
    sys.path.insert(0, ROOT)
    from bench import BRANCHING_WEIGHTS, WORKLOADS, make_closed_loop
    res = []
    for knobs in (dict(tok_mfma=1, tok_lw_min_n=NEVER, tok_lw_min=NEVER), dict(tok_mfma=0, tok_lw_min_n=0, tok_lw_min=0)):
        pl, sim, _ = make_closed_loop(dict(WORKLOADS["demo_1"]), ckpt=BRANCHING_WEIGHTS, speculative=False)
        pl.scen_tree_gen.native_aime = True
        rt = pl.network.rt
        try:
            for k, v in knobs.items():
                rt.set_tuning(k, v)
            sim.run_plans(1)
            st = rt.last_token_stats()
        finally:
            for k, v in dict(tok_mfma=0, tok_lw_min_n=NEVER, tok_lw_min=NEVER).items():
                rt.set_tuning(k, v)
        assert pl.scen_tree_gen.n_native_plans == 1 and st["layerwise"] == (1 if knobs["tok_lw_min"] == 0 else 0)
        res.append(_plan_tables(pl) + (np.array(sim.ctrl),))
    (na, ra, fa, ca), (nb, rb, fb, cb) = res
    assert na == nb and len(na) >= 1 and len(ra) == len(rb) > 0 and len(fa) == len(fb) > 0
    for x, y in zip(ra, rb):
        assert x[:2] == y[:2]
        for u, v in zip(x[2:], y[2:]):
            assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v), x[0]
    for x, y in zip(fa, fb):
        assert all(x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]) for k in x)
    assert np.array_equal(ca, cb)


def test_defaults_leave_the_default_path_where_it_was(hip_predictor, default_before):
    """With every knob back at its default (never) the outputs are the bits of the run made before this module touched a knob -- the
    arena, the plan and the events the new path left behind change nothing."""
    hp = hip_predictor
    want, pbs = default_before
    before = hp.pair_precision()
    try:
        _run(hp, pbs[(9, 21, 5, 2)], min_n=0, lw_min=0, chunk=48, taps=False)
        _restore(hp, before)
        for b, pb in pbs.items():
            got, st = _run(hp, pb, taps=False)
            assert st["layerwise"] == 0 and st["launches"] == 7 and st["chunks"] == 0
            _same(got, want[b], OUTS)
    finally:
        _restore(hp, before)
