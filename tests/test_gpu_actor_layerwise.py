"""GPU: the layer-wise batched ActorNet (mind_amd/csrc/actor_lw_kernels.hip; mind_set_tuning "actor_lw_min") against the per-actor kernel
it can replace, k_actor_mfma<NP>.  The path restates nothing: its convolutions run am_conv's MFMA sequence per output element, its
GroupNorm stages call am_gn itself -- so the requirement is BIT-identity in every arithmetic, for every batch, chunk size and position in
the batch, and through a whole plan in which rounds (and ranks) differ in which of the two kernels they take."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from mind_amd.synth import predictor_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dist_gpu_worker.py")
NEVER = 1 << 30


def _restore(hp, prec):
    hp.set_tuning("actor_lw_min", NEVER)
    hp.set_tuning("actor_lw_chunk", 0)
    hp.set_pair_precision(prec)


def _actor_feat(hp, pb, lw_min, chunk=0):
    hp.set_tuning("actor_lw_min", lw_min)
    hp.set_tuning("actor_lw_chunk", chunk)
    hp.predict_numpy_batch(pb)
    return hp.debug_read("actor_feat").reshape(-1, 128).copy(), hp.last_actor_stats()


BATCHES = [(3, 4, 1, 1), (8, 20, 2, 1), (40, 55, 1, 1), (17, 30, 3, 4), (64, 256, 1, 21),
           (1, 1, 1, 5), (5, 1, 2, 5), (33, 64, 2, 6)]      # ... and the odd actor counts 1, 5, 33 of test_hip_matches_oracle_ragged_tiles


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x3", "bf16"])
@pytest.mark.parametrize("a,l,B,seed", BATCHES)
def test_bit_identical_to_the_per_actor_kernel(prec, a, l, B, seed, hip_predictor):
    hp = hip_predictor
    pb = predictor_batch(a, l, B, seed=seed)
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        want, st0 = _actor_feat(hp, pb, NEVER)
        got, st1 = _actor_feat(hp, pb, 0)
    finally:
        _restore(hp, before)
    assert st0["layerwise"] == 0 and st0["launches"] == 1
    assert st1["layerwise"] == 1 and st1["chunks"] == 1 and st1["launches"] == 53
    assert want.shape == (a * B, 128) and np.isfinite(want).all() and np.abs(want).max() > 0.1
    assert np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x3", "bf16"])
def test_bit_identical_over_several_chunks_with_a_ragged_last_one(prec, hip_predictor):
    """300 actors in chunks of 96: three whole chunks and one of 12, every chunk through the same arena."""
    hp = hip_predictor
    pb = predictor_batch(60, 4, 5, seed=3)
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        want, st0 = _actor_feat(hp, pb, NEVER)
        got, st1 = _actor_feat(hp, pb, 0, chunk=96)
    finally:
        _restore(hp, before)
    assert st0["layerwise"] == 0 and st1["layerwise"] == 1 and st1["chunks"] == 4 and st1["launches"] == 4 * 53
    assert want.shape == (300, 128) and np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("prec", ["bf16x6", "bf16x3"])
@pytest.mark.parametrize("a,l,B,seed", [(3, 4, 1, 1), (8, 20, 2, 1), (40, 55, 1, 1)])
def test_golden_tap(prec, a, l, B, seed, hip_predictor, golden_predictor):
    """The bar of test_actor_net_tap_by_arithmetic: 5e-5 absolute against the reference's ActorNet tap."""
    hp = hip_predictor
    pb = predictor_batch(a, l, B, seed=seed)
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        af, st = _actor_feat(hp, pb, 0)
    finally:
        _restore(hp, before)
    err = float(np.abs(af - golden_predictor[f"a{a}_l{l}_b{B}_s{seed}_actor_net"]).max())
    print(f"layer-wise ActorNet {prec} a{a}_l{l}_b{B}_s{seed}: max|actor_feat - reference tap| = {err:.3e}")
    assert st["layerwise"] == 1
    assert err < 5e-5


def test_batch_and_chunk_invariance(hip_predictor):
    """An actor's row does not depend on the batch around it, on its place in the batch (column tiles at T = 12 and T = 6 hold several
    actors: no padding row may come from a neighbour) or on the chunking."""
    hp = hip_predictor
    big = predictor_batch(60, 4, 5, seed=3)
    row = predictor_batch(7, 3, 1, seed=9)["ACTORS"][4].copy()
    solo = predictor_batch(1, 1, 1, seed=5)
    solo["ACTORS"] = row[None].copy()
    front = dict(big, ACTORS=big["ACTORS"].copy())
    front["ACTORS"][0] = row
    back = dict(big, ACTORS=big["ACTORS"].copy())
    back["ACTORS"][299] = row
    before = hp.pair_precision()
    try:
        alone, _ = _actor_feat(hp, solo, 0)
        f1, _ = _actor_feat(hp, front, 0)
        b1, s1 = _actor_feat(hp, back, 0)
        f2, _ = _actor_feat(hp, front, 0, chunk=96)
        b2, s2 = _actor_feat(hp, back, 0, chunk=7)
        ref, s0 = _actor_feat(hp, back, NEVER)
    finally:
        _restore(hp, before)
    assert s1["chunks"] == 1 and s2["chunks"] == 43 and s0["layerwise"] == 0
    assert np.array_equal(alone[0], f1[0]) and np.array_equal(alone[0], b1[299])
    assert np.array_equal(f1, f2) and np.array_equal(b1, b2) and np.array_equal(b1, ref)
    assert np.array_equal(f1[1:299], b1[1:299])              # ... and the rows between do not see the changed neighbours


def test_threshold_selects_the_kernel_and_leaves_the_prediction(hip_predictor):
    """actor_lw_min = 100: a call of 64 actors stays on k_actor_mfma, a call of 128 takes the layer-wise kernels; cls / reg / vel are the
    same bits as with the knob at its default (never), where no call takes the new path."""
    hp = hip_predictor
    before = hp.pair_precision()
    outs = {}
    try:
        for A, pb in ((64, predictor_batch(64, 8, 1, seed=2)), (128, predictor_batch(64, 8, 2, seed=2))):
            for knob in (NEVER, 100):
                hp.set_tuning("actor_lw_min", knob)
                o = hp.predict_numpy_batch(pb)
                outs[A, knob] = ({k: o[k].cpu().numpy().copy() for k in ("cls", "reg", "vel")}, hp.last_actor_stats())
    finally:
        _restore(hp, before)
    assert outs[64, NEVER][1]["layerwise"] == 0 and outs[128, NEVER][1]["layerwise"] == 0
    assert outs[64, 100][1]["layerwise"] == 0 and outs[128, 100][1]["layerwise"] == 1
    for A in (64, 128):
        for k in ("cls", "reg", "vel"):
            assert np.array_equal(outs[A, NEVER][0][k], outs[A, 100][0][k]), (A, k)


def test_negative_chunk_means_the_default_and_the_arena_is_reused(hip_predictor):
    """A second call with a smaller chunk reuses the arena; a negative chunk means the default."""
    hp = hip_predictor
    pb = predictor_batch(17, 30, 3, seed=4)
    before = hp.pair_precision()
    try:
        a, s1 = _actor_feat(hp, pb, 0, chunk=16)
        b, s2 = _actor_feat(hp, pb, 0, chunk=-5)
    finally:
        _restore(hp, before)
    assert s1["chunks"] == 4 and s2["chunks"] == 1 and np.array_equal(a, b)


# ---- through the plan: tests/dist_gpu_worker.py as it is, started the way tests/test_gpu_sharded.py::_run starts it
def _run(world, tmp_path, tag, port, extra_env):
    procs, outs = [], []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
        out = os.path.join(tmp_path, f"{tag}_w{world}_r{r}.pkl")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, WORKER, out, "1"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    failed = None
    for p in procs:
        try:
            log, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        if p.returncode != 0 and failed is None:
            failed = (p.returncode, log.decode()[-2000:])
    assert failed is None, failed            # (a failed rank ends the test: nothing else is started)
    return [pickle.load(open(o, "rb")) for o in outs]


def _same_plan(a, b):
    for pa, pb in zip(a["res"], b["res"]):
        assert pa["keys"] == pb["keys"] and pa["best"] == pb["best"] and pa["n_trees"] == pb["n_trees"] == 6
        assert np.array_equal(pa["pos0"], pb["pos0"]) and np.array_equal(pa["xs"], pb["xs"]) and np.array_equal(pa["ctrl"], pb["ctrl"])


def test_the_full_tree_plans_the_same_with_either_kernel(tmp_path):
    """The full cfg4 tree (rounds of 64 / 384 / 2 304 / 13 824 actors) in one process with the knob at never, at 0 (every round layer-wise)
    and at 1 000 (the first two rounds on k_actor_mfma, the last two layer-wise): the same plan, bit for bit.  Then three gloo ranks with
    the knob at 5 000 -- a rank's block of the widest round is 4 608 actors (per-actor kernel) where the single process's 13 824 ran
    layer-wise at 1 000 -- return that plan too: no rule has to agree across ranks."""
    tmp = str(tmp_path)
    base = {"MIND_TEST_WORKLOAD": "cfg4tree"}
    never = _run(1, tmp, "never", 29711, dict(base, MIND_ACTOR_LW_MIN=str(NEVER)))[0]
    assert never["expanded"] == 259 and never["native_plans"] == 1
    every = _run(1, tmp, "zero", 29712, dict(base, MIND_ACTOR_LW_MIN="0"))[0]
    _same_plan(never, every)
    mixed = _run(1, tmp, "mixed", 29713, dict(base, MIND_ACTOR_LW_MIN="1000"))[0]
    _same_plan(never, mixed)
    ranks = _run(3, tmp, "ranks", 29714, dict(base, MIND_ACTOR_LW_MIN="5000"))
    assert sum(r["expanded"] for r in ranks) == 259
    for r in ranks:
        assert r["native_plans"] == 1
        _same_plan(mixed, r)
