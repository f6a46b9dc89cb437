"""The five synchronous "upload, launch, read back" entries (mind_audit_plan, mind_audit_episode, mind_audit_road_plan,
mind_audit_road_episode, mind_forecast_score) share ONE scratch buffer of the context: run interleaved on one context, every call behind a
larger call of another entry, each must return what the same call returns on a fresh context, bit for bit -- in particular the three calls
that skip an upload (no ``scored``, no track beside the ego's row, a tree without exo agents) right behind a call that left other bytes
where the skipped input would lie.  Shapes: the smallest that cross each staging edge (AU_CH = 16 agents, AU_TCH = 64 tracks, RD_TV = 256
vertices inside a ring)."""
import numpy as np
import pytest
import torch

import road_cases as rc

pytestmark = pytest.mark.gpu
BOX = (4.5, 2.0, 1.2)


def _calls(device):
    """name -> function of a HipPredictor, and the order to run them in on the shared context"""
    rng = np.random.default_rng(20251)
    flats = []
    for M, a in ((5, 1), (9, 18)):                                        # an agent-free tree, a tree of more than AU_CH agents
        flats.append(dict(parent=np.arange(-1, M - 1, dtype=np.int32), prob=rng.uniform(0.1, 1.0, M).astype(np.float32),
                          mean=rng.uniform(-25.0, 25.0, (M, a, 2)).astype(np.float32), cov=rng.uniform(0.0, 2.0, (M, a)).astype(np.float32)))
    xs = rng.uniform(-25.0, 25.0, (3, 14, 6))
    road = rc.synth_road(5, (4, 257))                                     # the second ring straddles a turn of RD_TV vertices
    ego = np.concatenate([rng.uniform(-25.0, 25.0, (2, 3, 2)), rng.uniform(0.0, 9.0, (2, 3, 1)), rng.uniform(-3.0, 3.0, (2, 3, 1))], 2)
    exo, valid, boxes = rng.uniform(-25.0, 25.0, (3, 66, 5)), (rng.uniform(size=(3, 66)) < 0.7).astype(np.uint8), rng.uniform(0.5, 6.0, (66, 2))
    gen = torch.Generator().manual_seed(3)
    reg, cls = torch.randn(3, 2, 8, 5, generator=gen).to(device), torch.softmax(torch.randn(2, 2, generator=gen), 1).to(device)
    gt, gv, scored = rng.normal(size=(3, 8, 2)), (rng.uniform(size=(3, 8)) < 0.8).astype(np.uint8), np.array([1, 0, 1], np.uint8)
    score = lambda hp, sc: hp.forecast_score(reg, cls, [0, 1, 3], gt, gv, sc, horizons=(4, 8))
    calls = dict(plan=lambda hp: hp.audit_plan(flats, xs, BOX, 2.5),
                 episode=lambda hp: hp.audit_episode(ego, exo, valid, boxes, BOX),
                 episode_alone=lambda hp: hp.audit_episode(ego, exo[:, :1], valid[:, :1], boxes[:1], BOX),
                 road_plan=lambda hp: hp.audit_road_plan(flats, xs, road.verts, road.poly_off, BOX),
                 road_episode=lambda hp: hp.audit_road_episode(ego, road.verts, road.poly_off, BOX),
                 forecast=lambda hp: score(hp, scored), forecast_all=lambda hp: score(hp, None))
    # arena bytes, about: episode 9.6 K > road_plan 7.5 K > plan 5.0 K > road_episode 4.6 K > forecast 2 K > episode_alone 0.6 K
    order = ("episode", "road_plan", "plan", "road_episode", "forecast", "episode", "forecast_all", "road_plan", "episode_alone")
    return calls, order


def _bytes(res):
    """every array of a result dict (per-tree lists flattened) as raw bytes"""
    out = {}
    for k, v in res.items():
        for i, a in enumerate(v if isinstance(v, list) else [v]):
            out[k, i] = (a.dtype.str, a.shape, a.tobytes())
    return out


def test_interleaved_calls_equal_fresh_contexts(hip_predictor):
    from mind_amd.predictor import HipPredictor
    calls, order = _calls(hip_predictor.device)
    want = {}
    for name, fn in calls.items():
        fresh = HipPredictor(0)
        try:
            want[name] = _bytes(fn(fresh))
        finally:
            fresh.close()
    assert all(len(w) > 0 for w in want.values())
    assert want["forecast"] != want["forecast_all"] and want["episode"] != want["episode_alone"]      # (the skipped inputs matter)
    for step, name in enumerate(order):
        got = _bytes(calls[name](hip_predictor))
        assert got.keys() == want[name].keys(), (step, name)
        for k in got:
            assert got[k] == want[name][k], (step, name, k)
