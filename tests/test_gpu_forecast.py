"""GPU: forecast scoring on the device (mind_forecast_score / k_forecast_modes, k_forecast_scenes, mind_amd/forecast.py) against the library's
HOST evaluation of the same header (mind_debug_forecast_score): every output bit for bit, over every shape, horizon set and validity
pattern of the CPU suite's seeded batches (tests/forecast_cases.py: tests/test_forecast_host.py asserts that none of their decisions sits
within 1e-7 of an edge), agent counts about the staging block, launch shapes, hand and NaN cases, the predictor's own outputs, and a
closed loop scored beside the planner in both drivers."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import forecast_cases as fc
import forecast_restate as rs
from mind_amd import _lib, forecast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

NB = 5                    # agents per workgroup of k_forecast_modes at K = 6, T = 60 (FC_NB_6_60)
CFG = dict(miss_radius=2.0, disc_scale=1.0, disc_offset=0.5)


def _dev(hp, b, scored=None, horizons=(60,), lo=0, hi=None, off=None, **kw):
    """the device call on agents lo..hi of a host batch (one scene unless ``off`` says otherwise)"""
    hi = len(b["reg"]) if hi is None else hi
    off = b["actor_off"] if off is None and (lo, hi) == (0, len(b["reg"])) else ([0, hi - lo] if off is None else off)
    reg, cls = torch.from_numpy(np.array(b["reg"][lo:hi])).to(hp.device), torch.from_numpy(np.array(b["cls"])).to(hp.device)
    if len(off) - 1 != cls.shape[0]:
        cls = cls[:len(off) - 1].contiguous()
    return hp.forecast_score(reg, cls, off, b["gt"][lo:hi], b["valid"][lo:hi], None if scored is None else scored[lo:hi], horizons, **dict(CFG, **kw))


def _host(b, scored=None, horizons=(60,), lo=0, hi=None, off=None, **kw):
    hi = len(b["reg"]) if hi is None else hi
    off = b["actor_off"] if off is None and (lo, hi) == (0, len(b["reg"])) else ([0, hi - lo] if off is None else off)
    return _lib.forecast_score_host(b["reg"][lo:hi], b["cls"][:len(off) - 1], off, b["gt"][lo:hi], b["valid"][lo:hi],
                                    None if scored is None else scored[lo:hi], horizons, **dict(CFG, **kw))


@pytest.mark.parametrize("K,T", fc.SHAPES)
def test_device_is_the_host_text(hip_predictor, K, T):
    b = fc.batch(K, T)
    for hz in fc.horizons_for(T):
        for scored in (None, b["scored"]):
            fc.same(_dev(hip_predictor, b, scored, hz), _host(b, scored, hz), where=(K, T, hz, scored is None))
    # only some outputs asked for: the others are not touched, these are the same
    r = hip_predictor.forecast_score(torch.from_numpy(b["reg"].copy()).to(hip_predictor.device), torch.from_numpy(b["cls"].copy()).to(hip_predictor.device),
                                     b["actor_off"], b["gt"], b["valid"], horizons=(T,), want=("fde", "s_miss_rate"), **CFG)
    assert sorted(r) == ["fde", "s_miss_rate"]
    fc.same(r, _host(b, None, (T,)), names=("fde", "s_miss_rate"))


def test_agent_counts_about_the_staging_block(hip_predictor):
    b = fc.batch()
    assert NB > 2
    for n in (1, NB - 1, NB, NB + 1, 2 * NB + 1):
        for lo in (0, 14):                   # (agent 14 on: another mix of validity patterns at the block's edge)
            fc.same(_dev(hip_predictor, b, b["scored"], (10, 30, 60), lo, lo + n), _host(b, b["scored"], (10, 30, 60), lo, lo + n), where=(n, lo))
    # an unaligned view of reg (the 4-byte staging path) gives the same bits
    hp = hip_predictor
    flat = torch.zeros(b["reg"].size + 1, device=hp.device)
    flat[1:] = torch.from_numpy(b["reg"].copy()).to(hp.device).reshape(-1)
    view = flat[1:].view(b["reg"].shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    r = hp.forecast_score(view, torch.from_numpy(b["cls"].copy()).to(hp.device), b["actor_off"], b["gt"], b["valid"], b["scored"], (10, 30, 60), **CFG)
    fc.same(r, _host(b, b["scored"], (10, 30, 60)))


def test_launch_shapes(hip_predictor):
    """the 323-agent batch in one call == the same agents one scene per call == one agent per call, every per-agent output"""
    b = fc.batch()
    hz = (10, 30, 60)
    off = b["actor_off"]
    whole = _dev(hip_predictor, b, None, hz)
    names = rs.NAMES_A3 + rs.NAMES_A2
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        if hi == lo:                         # (a call without an agent is a no-op: it writes nothing)
            continue
        b1 = dict(b, cls=b["cls"][s:s + 1])
        one = _dev(hip_predictor, b1, None, hz, lo, hi)
        fc.same(one, fc.agent_rows(whole, lo, hi), names=names, where=("scene", s))
        fc.same({k: one[k][0] for k in rs.NAMES_S}, {k: whole[k][s] for k in rs.NAMES_S}, names=rs.NAMES_S, where=("scene row", s))
    for a in range(323):
        s = int(np.searchsorted(off, a, side="right") - 1)
        one = _dev(hip_predictor, dict(b, cls=b["cls"][s:s + 1]), None, hz, a, a + 1)
        fc.same(one, fc.agent_rows(whole, a, a + 1), names=names, where=("agent", a))


def _one(hp, xy, gt, sig=(1.0, 1.0), cls=None, K=6, T=1, horizons=None, **kw):
    gt = np.asarray(gt, np.float64).reshape(-1, T, 2)
    A = gt.shape[0]
    reg = np.zeros((A, K, T, 5), np.float32)
    reg[..., :2] = np.asarray(xy, np.float32).reshape(A, -1, T, 2)
    reg[..., 2], reg[..., 3], reg[..., 4] = sig[0], sig[1], 1.0
    cls = np.full((1, K), 1.0 / K, np.float32) if cls is None else np.asarray(cls, np.float32).reshape(1, K)
    b = dict(reg=reg, cls=cls, actor_off=np.array([0, A], np.int32), gt=gt, valid=np.ones((A, T), np.uint8))
    hz = (T,) if horizons is None else horizons
    got = _dev(hp, b, None, hz, **kw)
    fc.same(got, _host(b, None, hz, **kw))
    return got


def test_hand_and_nan_cases_on_the_device(hip_predictor):
    hp = hip_predictor
    r = _one(hp, [[0.0, 0.0]], [[3.0, 4.0]], sig=(2.5, 1.0), disc_offset=2.5, miss_radius=5.0)
    assert np.all(r["ade"] == 5.0) and np.all(r["fde"] == 5.0) and np.all(r["cover"] == 1) and np.all(r["first_out"] == -1)
    assert r["s_miss_rate"][0, 0] == 0.0 and np.all(r["k_ade"] == 0) and np.all(r["s_k_fde"] == 0)
    r = _one(hp, [[0.0, 0.0]], [[3.0, 4.0]], sig=(1.0, 2.5), disc_offset=2.5 - 2.0 ** -50, miss_radius=np.nextafter(5.0, 0.0))
    assert np.all(r["cover"] == 0) and np.all(r["first_out"] == 0) and r["s_miss_rate"][0, 0] == 1.0 and r["s_miss_top"][0, 0] == 1.0
    r = _one(hp, [[0.0, 0.0]], [[3.0, 4.0]], cls=[0.1, 0.3, 0.05, 0.3, 0.2, 0.05])
    assert r["s_k_top"][0, 0] == 1
    T, hz = 8, (2, 4, 8)
    g = np.random.default_rng(3)
    gt = np.cumsum(g.uniform(0.5, 1.0, (2, T, 2)), axis=1)
    xy = gt[:, None] + g.normal(scale=0.3, size=(2, 6, T, 2))
    xy[0, 2, 3, 0] = np.nan
    r = _one(hp, xy, gt, T=T, horizons=hz, disc_offset=50.0)
    assert np.isfinite(r["ade"][0, 0, 2]) and np.isnan(r["ade"][0, 1:, 2]).all() and np.all(r["k_ade"][0, 1:] != 2) and np.all(r["s_k_ade"][0, 1:] != 2)
    assert r["first_out"][0, :, 2].tolist() == [-1, 3, 3] and r["cover"][0, :, 2].tolist() == [2, 3, 7]
    xy[0, :, :, 0] = np.inf
    r = _one(hp, xy, gt, T=T, horizons=hz)
    assert np.all(r["k_ade"][0] == -1) and np.all(r["k_fde"][0] == -1) and np.isnan(r["brier_fde"][0]).all() and np.all(r["s_k_fde"][0] == -1)
    xy[0, :, :, 0] = np.nan
    r = _one(hp, xy, gt, T=T, horizons=hz)
    assert np.all(r["k_ade"][0] == -1) and np.isnan(r["min_fde"][0]).all() and np.isnan(r["s_miss_rate"]).all()


@pytest.fixture(scope="module")
def predicted(hip_predictor):
    """hip_predictor.predict on synthetic scenes (formula weights): (agents per scene, scenes) -> (device outputs, actor_off)"""
    from mind_amd.synth import predictor_batch
    out = {}
    for a in (1, 3, 36):
        for B in (1, 3):
            pb = predictor_batch(a, 10, B, seed=11 + a + B)
            o = hip_predictor.predict_numpy_batch(pb)
            out[(a, B)] = (o, [a * i for i in range(B + 1)])
    return out


@pytest.mark.parametrize("a,B", [(1, 1), (1, 3), (3, 1), (3, 3), (36, 1), (36, 3)])
def test_end_to_end_on_the_predictors_outputs(hip_predictor, predicted, a, B):
    o, off = predicted[(a, B)]
    reg, cls = o["reg"], o["cls"]
    assert reg.shape == (a * B, 6, 60, 5) and cls.shape == (B, 6) and reg.device == hip_predictor.device
    g = np.random.default_rng(a * 10 + B)
    rh = reg.cpu().numpy()
    # a truth near one of the modes, drifting away from it; a few holes
    gt = rh[np.arange(a * B), g.integers(0, 6, a * B), :, :2].astype(np.float64) + np.cumsum(g.normal(scale=0.05, size=(a * B, 60, 2)), axis=1)
    valid = (g.uniform(size=(a * B, 60)) < 0.9).astype(np.uint8)
    got = hip_predictor.forecast_score(reg, cls, off, gt, valid, horizons=(10, 30, 60), **CFG)
    want = _lib.forecast_score_host(rh, cls.cpu().numpy(), off, gt, valid, None, (10, 30, 60), **CFG)
    fc.same(got, want)
    assert np.isfinite(got["s_min_ade"]).all() and np.all(got["s_n_scored"][:, -1] == a)


def _make(scene, native):
    sys.path.insert(0, ROOT)
    from bench import BRANCHING_WEIGHTS, WORKLOADS
    from mind_amd.closed_loop import ClosedLoopSim
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.scene_io import ReplayWorld, scene_fixture_path
    cfg = os.path.join(ROOT, "mind_amd", "planners", "mind", "configs", "synthetic.json")
    wkw = dict(WORKLOADS[scene])
    w = ReplayWorld.from_scene_file(scene_fixture_path(wkw["scene"]))
    cfg = dict(json.load(open(cfg)), planning_config="planners.mind.configs.planning." + wkw["scene"], ckpt_path=BRANCHING_WEIGHTS)
    pl = MINDPlanner(cfg)
    pl.traj_tree_opt.speculative = False
    return pl, ClosedLoopSim(w, pl, native=native)


def _trace(sim, stepper, n_plans):
    """drive until n_plans plans were made: per step the ego state in force and the control, per plan the first trajectory tree's states"""
    from mind_amd import audit
    states, ctrls, plans = [], [], []
    while sim.n_plans < n_plans:
        planned = stepper()
        states.append(np.array(sim.state, np.float64))
        ctrls.append(np.array(sim.ctrl, np.float64))
        if planned:
            scen, traj = sim.last_result
            plans.append(audit._states_of(traj[0], len(audit._flat_of(scen[0])["parent"])).copy())
    return np.stack(states), np.stack(ctrls), plans


EVERY = 5
SCORING = dict(horizons=(10, 30, 60), disc_offset=forecast.DEFAULT_DISC_OFFSET)


@pytest.mark.parametrize("native", [None, False])
def test_episode_scorer_beside_the_planner(native):
    """12 planning cycles of recorded demo_1: wrapped and unwrapped runs make the same plans, controls and ego states bit for bit; the
    scorer's per-cycle rows are score_scene called by hand at the same instants, from a window and a generator of this test's own"""
    N = 12
    pl0, sim0 = _make("demo_1", native)
    assert (sim0._native is not None) == (native is None)
    s0, c0, p0 = _trace(sim0, sim0.step, N)
    pl, sim = _make("demo_1", native)
    sc = forecast.EpisodeForecastScorer(sim, every=EVERY, **SCORING)
    gen_before = (pl.scen_tree_gen.lane_graph, pl.scen_tree_gen.lane_feat_in)
    gen = type(pl.scen_tree_gen)(pl.device, pl.network, pl.obs_len, pl.scen_tree_gen.pred_len, pl.scen_tree_gen.config)
    win, hand, w = forecast.ObservationWindow(pl.obs_len), [], sim.world

    def stepper():
        t = sim.sim_time
        if sim.last_trigger is None or (t - sim.last_trigger) >= sim.PLAN_STEP:       # the simulator's trigger: an observation cycle starts
            lcl = forecast.observation(w, t, sim.state if sim.enabled else None)
            win.update(lcl)
            if len(hand) % EVERY == 0:
                gen.set_target_lane(*type(pl)._resample_target_lane(pl, lcl))
                hand.append((t, forecast.score_scene(gen, w, lcl, win.agent_obs, t, **SCORING)))
            else:
                hand.append((t, None))
        return sc.step()
    s1, c1, p1 = _trace(sim, stepper, N)
    assert (sim._native is not None) == (native is None)
    assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and len(p0) == len(p1) == N and all(np.array_equal(x, y) for x, y in zip(p0, p1))
    if native is None:              # (the Python steps' own process_data rewrites them every plan)
        assert pl.scen_tree_gen.lane_graph is gen_before[0] and pl.scen_tree_gen.lane_feat_in is gen_before[1]
    rep = sc.report()
    want = [(t, r) for t, r in hand if r is not None]
    C_ = len(rep["times"])
    assert C_ == len(want) == (sc.n_cycles + EVERY - 1) // EVERY and sc.n_cycles == len(hand) and rep["planned"].sum() >= 2 and (~rep["planned"]).sum() >= 2
    assert rep["before"]["cycles"].tolist() == np.flatnonzero(~rep["planned"]).tolist() and rep["after"]["times"][0] >= sim.enable_time - 1e-9
    assert np.all(rep["s_n_scored"][:, -1] > 1) and np.isfinite(rep["s_min_ade"]).all() and np.isfinite(rep["mean"]["s_min_fde"]).all()
    assert np.all((rep["cover_frac"] >= 0) & (rep["cover_frac"] <= 1))
    for i, (t, r) in enumerate(want):
        row = sc.rows[i]
        assert row["time"] == t == rep["times"][i] and row["tids"] == r["tids"] and np.array_equal(row["gt"], r["gt"]) and np.array_equal(row["valid"], r["valid"])
        fc.same(row, r, where=("cycle", i))
        for k in forecast.EpisodeForecastScorer.SCENE_KEYS:
            assert np.array_equal(rep[k][i], r[k][0], equal_nan=True), (k, i)
    # before the take-over the window is the recording's: the same rows from the world alone
    lcl, obs, t_obs = fc.window_at(w, want[1][0])
    assert t_obs == want[1][0] and not rep["planned"][1]
    gen.set_target_lane(*type(pl)._resample_target_lane(pl, lcl))
    fc.same(sc.rows[1], forecast.score_scene(gen, w, lcl, obs, t_obs, **SCORING))
    print("demo_1", "native" if native is None else "python", "cycles", C_, "min ADE @1/3/6 s before", rep["before"]["mean"]["s_min_ade"], "after",
          rep["after"]["mean"]["s_min_ade"], "miss", rep["mean"]["s_miss_rate"], "cover", rep["mean"]["cover_frac"])


def test_score_scene_is_the_calls_by_hand(hip_predictor):
    pl, sim = _make("demo_2", False)
    w = sim.world
    lcl, obs, t = fc.window_at(w, 4.0)
    gen = type(pl.scen_tree_gen)(pl.device, pl.network, pl.obs_len, pl.scen_tree_gen.pred_len, pl.scen_tree_gen.config)
    gen.set_target_lane(*type(pl)._resample_target_lane(pl, lcl))
    got = forecast.score_scene(gen, w, lcl, obs, t, horizons=(10, 30, 60), **CFG)
    scene = gen.process_data(lcl, obs)
    d, _ = gen.predict_inputs([scene])
    pl.network(d)
    pk = pl.network.last_packed
    gt, valid = forecast.ground_truth(w, scene, t)
    assert np.array_equal(gt, got["gt"]) and np.array_equal(valid, got["valid"]) and got["tids"] == list(scene["TRAJS_TID"])
    a = len(scene["TRAJS_TID"])
    fc.same(got, pk["rt"].forecast_score(pk["reg"], pk["cls"], [0, a], gt, valid, horizons=(10, 30, 60), **CFG))
    fc.same(got, _lib.forecast_score_host(pk["reg"].cpu().numpy(), pk["cls"].cpu().numpy(), [0, a], gt, valid, None, (10, 30, 60), **CFG))
    from mind_amd import runtime
    fc.same(got, runtime.forecast_score(pk["reg"], pk["cls"], [0, a], gt, valid, horizons=(10, 30, 60), **CFG))


def test_error_codes_on_the_device(hip_predictor):
    import ilqr_policy_restate as pr
    from mind_amd.predictor import IlqrCall
    from oracle import ilqr as oi
    hp = hip_predictor
    b = fc.batch()
    reg, cls = torch.from_numpy(b["reg"].copy()).to(hp.device), torch.from_numpy(b["cls"].copy()).to(hp.device)

    def raw(gt=b["gt"], valid=b["valid"], horizons=(60,)):
        cfg, B, off, g, v, sc, out, res, keep = _lib.forecast_args(6, 60, b["actor_off"], gt, valid, None, horizons, **CFG, want=("ade",))
        res["ade"][:] = -7.0
        rc = hp.lib.mind_forecast_score(hp.ctx, C.byref(cfg), B, off, C.c_void_p(reg.data_ptr()), C.c_void_p(cls.data_ptr()), g, v, sc, C.byref(out))
        return rc, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode(), res["ade"]
    rc, _, ade = raw()
    assert rc == _lib.MIND_OK and not np.any(ade == -7.0)
    bad = b["gt"].copy()
    bad[0, 7, 0] = np.nan                                # agent 0: every sample valid
    rc, msg, ade = raw(gt=bad)
    assert rc == _lib.MIND_EINVAL and msg.startswith("mind_forecast_score") and "agent 0 sample 7" in msg and np.all(ade == -7.0)
    bad = b["gt"].copy()
    bad[1, 7, 0] = np.inf                                # agent 1: no sample valid
    rc, _, ade = raw(gt=bad)
    assert rc == _lib.MIND_OK and np.array_equal(ade, raw()[2], equal_nan=True)
    rc, msg, ade = raw(horizons=(61,))
    assert rc == _lib.MIND_EINVAL and "horizon" in msg and np.all(ade == -7.0)
    with pytest.raises(_lib.MindError):
        hp.forecast_score(reg, cls, b["actor_off"], b["gt"], b["valid"], miss_radius=-1.0)
    # while a begun tree-iLQR call is pending: MIND_ESTATE, and that call then finishes with its usual result
    s = pr.scene("lead", 4)
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    ref = hp.ilqr_contingency(cfg_w, cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"])
    call = IlqrCall(hp.lib, cfg_w, [s["flat"]], s["x0"], s["lane"], s["tv"], cfg_full=cfg_f)
    call.begin(hp)
    try:
        rc, msg, ade = raw()
        assert rc == _lib.MIND_ESTATE and "has not been finished" in msg and np.all(ade == -7.0)
    finally:
        xs2, us2, sw, sf = call.wait().finish()
    assert np.array_equal(xs2[0], ref[0][0]) and np.array_equal(us2[0], ref[1][0])
    assert raw()[0] == _lib.MIND_OK
