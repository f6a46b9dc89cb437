"""GPU: the knobs that close idle gaps of the planning cycle move host work and HIP calls, never an arithmetic operation, so every plan must
stay bit-identical with each of them on or off:
  "dec_poll"    the round's last glue kernel marks the mirrored decisions complete (a generation word behind them) and the host polls the
                word instead of draining the stream, sizing the next round's buffers while it waits;
  "root_head"   the root round's lane graph, world-frame histories, lane-distance field and frame read-back are launched by the predictor
                call behind ActorNet instead of in front of the call;
  "round_head"  the same for a later round's repeated lane features and frame read-back.
  "dec_head_ra" the split decoder's head (k_dec_actor<2, .>) with 1 or 2 agents per workgroup instead of 4: its two 128 -> 128 stages take the
                K split of the four-agent form explicitly, everything else is per row.
The native loop on recorded demo_1 (tables of mind_loop_last_plan, 12 cycles across an episode restart) with all on, all off and each alone;
and the polled decisions on plans of particular shapes: one round where nothing branches, a scripted tree that branches in every round the
depth allows, and a round of AIME_SMALL + 1 = 9 scenes (the first size whose scene tables no longer travel in the kernel arguments); and the
head's three forms on predictor calls of 1, 3, 4, 5 and 9 agents per scene (the ego alone, both sides of the 2- and 4-agent workgroup
boundaries) in 1 and 3 scenes, under random weights (tests/weight_regimes.py: formula weights can hide a wrong row)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_native_loop import _make, _same, _snapshot  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("dec_poll", "root_head", "round_head", "dec_head_ra")
OFF = {"dec_head_ra": 4}         # (the head's agents per workgroup: 0 = by the call's agents, 4 = the head as it was)
CYCLES, EPISODE = 12, 7          # (the episode restarts behind the seventh plan)


def _created_with():
    """what the context was created with: the library's defaults (on) or their MIND_* overrides"""
    return {k: int(os.environ.get("MIND_" + k.upper(), 0 if k in OFF else 1)) for k in KNOBS}


def _arm(on):
    """knob values with the knobs of `on` on and the others off"""
    return {k: (0 if k in OFF else 1) if k in on else OFF.get(k, 0) for k in KNOBS}


def _loop_cycles(values):
    pl, sim = _make("demo_1", None, episode_plans=EPISODE)
    rt = pl.network.rt
    assert sim._native is not None
    snaps = []
    try:
        for k, v in values.items():
            rt.set_tuning(k, v)
        for _ in range(CYCLES):
            sim.run_plans(1)
            snaps.append(_snapshot(pl, sim))
    finally:
        for k, v in _created_with().items():
            rt.set_tuning(k, v)
    assert sim.n_episodes == 1
    return snaps


@pytest.fixture(scope="module")
def all_on():
    snaps = _loop_cycles(_arm(KNOBS))
    # consecutive plans decide differently (a generation word left over from the plan before would hand the host that plan's decisions)
    for a, b in zip(snaps, snaps[1:]):
        assert len(a["scen"]) != len(b["scen"]) or any(not np.array_equal(u, v) for x, y in zip(a["scen"], b["scen"]) for u, v in zip(x[2:], y[2:]))
    assert sum(len(s["costs"]) > 1 for s in snaps) >= 4          # the plans really branch: rounds beyond the root run
    return snaps


@pytest.mark.parametrize("arm", ("all_off",) + KNOBS)
def test_cycle_gap_knobs_leave_every_cycle_bit_identical(all_on, arm):
    """all knobs off, and each alone, against all on"""
    snaps = _loop_cycles(_arm((arm,)))
    assert len(snaps) == len(all_on) == CYCLES
    for cycle, (a, b) in enumerate(zip(all_on, snaps)):
        _same(a, b, cycle)


def _plan_once(make, dec_poll):
    pl, sim = make()
    rt = pl.network.rt
    plans, plan = [], rt.aime_plan
    rt.aime_plan = lambda *a, **k: plans.append(plan(*a, **k)) or plans[-1]
    try:
        rt.set_tuning("dec_poll", dec_poll)
        sim.run_plans(2)          # two plans back to back: the second one's words follow the first one's in the same staging
    finally:
        del rt.aime_plan
        rt.set_tuning("dec_poll", _created_with()["dec_poll"])
    assert len(plans) == 2 and pl.scen_tree_gen.n_native_plans == 2
    out = []
    for nodes, rows, info in plans:
        out.append(dict(rounds=[n for n in info["round_scenes"] if n > 0], nodes=nodes.tobytes(), rows=rows.copy(), flats=info["flats"]))
    scen, traj = sim.last_result
    return out, dict(best=pl.timing["best_traj_idx"], costs=np.array(pl.timing["tree_costs"]), ctrl=np.array(sim.ctrl),
                     xs=[np.array([n.data[0] for k, n in t.nodes.items() if k != -1]) for t in traj])


def _recorded_plain():
    from bench import PLAIN_WEIGHTS, WORKLOADS, make_closed_loop
    pl, sim, _ = make_closed_loop(dict(WORKLOADS["demo_1"]), ckpt=PLAIN_WEIGHTS, speculative=False)
    return pl, sim


def _scripted(speeds=None):
    from bench import make_closed_loop
    pl, sim, _ = make_closed_loop(dict(n_agents=16, n_lanes=4, n_segs=8, seed=4), full_tree=True, speculative=False)
    if speeds is not None:
        pl.scen_tree_gen.network.speeds = speeds          # (equal ego speeds give equal topology signatures: those modes merge)
    return pl, sim


# the rounds each shape must show (checked on the plans themselves): one round and no branch; every round the tree's depth of 4 allows, the
# last one of more than 200 scenes; three surviving modes per scene, hence a round of nine scenes
SHAPES = {
    "nothing_branches": (_recorded_plain, lambda r: r == [1]),
    "every_round_branches": (_scripted, lambda r: r[:3] == [1, 6, 36] and len(r) == 4 and r[3] > 200),
    "nine_scenes": (lambda: _scripted((1.0, 1.0, 4.6, 4.6, 10.0, 10.0)), lambda r: r[:3] == [1, 3, 9]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_polled_decisions_equal_the_drained_stream(shape):
    sys.path.insert(0, ROOT)
    make, rounds_ok = SHAPES[shape]
    (polled, end_p), (drained, end_d) = _plan_once(make, 1), _plan_once(make, 0)
    for p, d in zip(polled, drained):
        print(shape, "rounds", p["rounds"])
        assert rounds_ok(p["rounds"]), p["rounds"]
        assert p["rounds"] == d["rounds"] and p["nodes"] == d["nodes"] and np.array_equal(p["rows"], d["rows"])
        assert len(p["flats"]) == len(d["flats"])
        for (ta, fa), (tb, fb) in zip(p["flats"], d["flats"]):
            assert ta == tb and all(np.array_equal(fa[k], fb[k]) and fa[k].dtype == fb[k].dtype for k in ("parent", "prob", "mean", "cov"))
    assert end_p["best"] == end_d["best"] and np.array_equal(end_p["costs"], end_d["costs"]) and np.array_equal(end_p["ctrl"], end_d["ctrl"])
    assert len(end_p["xs"]) == len(end_d["xs"]) > 0 and all(np.array_equal(x, y) for x, y in zip(end_p["xs"], end_d["xs"]))


@pytest.fixture(scope="module")
def seed7_predictor():
    import weight_regimes as wr
    from mind_amd.predictor import HipPredictor
    hp = HipPredictor(0)
    hp.load_state_dict(wr.regime_state_dict("seed7"))
    yield hp
    hp.set_tuning("dec_head_ra", _created_with()["dec_head_ra"])
    hp.close()


@pytest.mark.parametrize("scenes", [1, 3])
@pytest.mark.parametrize("agents", [1, 3, 4, 5, 9])
def test_decoder_head_forms_give_the_same_bits(seed7_predictor, agents, scenes):
    from mind_amd.synth import predictor_batch
    hp = seed7_predictor
    pb = predictor_batch(agents, 4, scenes, seed=3)
    outs = {}
    for ra in (4, 1, 2, 0):
        hp.set_tuning("dec_head_ra", ra)
        out = hp.predict_numpy_batch(pb)
        outs[ra] = (out["reg"].cpu().numpy().copy(), out["vel"].cpu().numpy().copy())
    reg4, vel4 = outs[4]
    assert reg4.size == agents * scenes * 6 * 60 * 5 and vel4.size == agents * scenes * 6 * 60 * 2
    assert np.isfinite(reg4).all() and np.isfinite(vel4).all()
    assert np.unique(reg4.reshape(agents * scenes * 6, -1)[:agents * 6], axis=0).shape[0] == agents * 6          # a scene's (agent, mode) rows all differ
    for ra in (1, 2, 0):
        assert np.array_equal(outs[ra][0].view(np.uint32), reg4.view(np.uint32)), (ra, "reg")
        assert np.array_equal(outs[ra][1].view(np.uint32), vel4.view(np.uint32)), (ra, "vel")
