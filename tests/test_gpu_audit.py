"""GPU: the clearance audit on the device (mind_audit_plan / k_audit_plan, mind_audit_episode / k_audit_episode, mind_amd/audit.py) against the
library's HOST evaluation of the same header (mind_debug_box_clearance with its own sin / cos, pair by pair) reduced by the restatement's rules
(tests/box_geom_restate.py, tests/audit_cases.py): every output bit for bit.  The scripted trees' margins make that meaningful: the smallest
|clearance| over the four fixtures is 1.7e-3 m and the smallest gap between the nearest and the second-nearest agent 1.8e-3 m, so no argmin
and no hit flag sits on a last-bit edge."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import audit_cases as ac
import ilqr_policy_restate as pr
from mind_amd import _lib, audit
from mind_amd.predictor import IlqrCall
from oracle import ilqr as oi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

FIXTURES = [("lead", 4), ("branch3", 12), ("deep", 4), ("straight", 1)]
CB, CH = 256, 16          # candidates per workgroup and agents per LDS staging turn of k_audit_plan (AU_CB, AU_CH)
MARGIN = 2.5


@pytest.fixture(scope="module")
def cases(hip_predictor):
    """per fixture: the flat tree and three candidate state sets [3, M, 6] -- the states of the warm controls, of the full fit, and of the
    full fit's controls plus unit noise (HipPredictor.ilqr_score rolls them out)"""
    hp, out = hip_predictor, {}
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    for kind, a in FIXTURES:
        s = pr.scene(kind, a)
        _, us_w, _ = hp.ilqr_solve(cfg_w, [s["flat"]], s["x0"], s["lane"], s["tv"], 0)
        _, us_f, _, _ = hp.ilqr_contingency(cfg_w, cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"])
        noise = np.random.default_rng(17).normal(size=us_f[0].shape)
        xs = hp.ilqr_score(cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"], 1, np.stack([us_w[0], us_f[0], us_f[0] + noise]), want_L=False)[0][0]
        assert np.all(np.isfinite(xs))
        out[(kind, a)] = dict(flat=s["flat"], xs=xs, M=s["M"])
    return out


def _many(xs, n):
    """n distinct candidates from the three of a case: copy c is shifted rigidly by a few centimetres per copy"""
    out = np.stack([xs[c % 3] for c in range(n)])
    out[:, :, 0] += 0.037 * (np.arange(n) // 3)[:, None]
    out[:, :, 1] -= 0.011 * (np.arange(n) // 3)[:, None]
    return out


def test_plan_audit_is_the_host_text(hip_predictor, cases):
    for key in FIXTURES:
        c = cases[key]
        got = hip_predictor.audit_plan([c["flat"]], [c["xs"]], ac.EGO_BOX, MARGIN)
        ac.same_plan(got, ac.host_plan([c["flat"]], [c["xs"]], ac.EGO_BOX, MARGIN))
        print(key, "fit: nodes hit", int(got["tree_hits"][1, 0]), "of", c["M"], "min", float(got["tree_min"][1, 0]))
    fit = {k: hip_predictor.audit_plan([cases[k]["flat"]], [cases[k]["xs"][1:2]], ac.EGO_BOX, MARGIN) for k in FIXTURES}
    lead, b3, deep, st = (fit[k] for k in FIXTURES)
    assert lead["tree_hits"][0, 0] == 0 and lead["tree_first"][0, 0] == -1 and lead["tree_min"][0, 0] > 0 and lead["tree_mass"][0, 0] == 0.0
    for r in (b3, deep):
        assert r["tree_hits"][0, 0] > 0 and r["tree_min"][0, 0] < 0 and r["tree_first"][0, 0] >= 0 and r["tree_mass"][0, 0] > 0
        assert r["node_clear"][0][0, r["tree_node"][0, 0]] == r["tree_min"][0, 0] and r["tree_agent"][0, 0] >= 1
    assert np.all(st["node_clear"][0] == np.inf) and np.all(st["node_agent"][0] == -1)
    assert st["tree_min"][0, 0] == np.inf and st["tree_agent"][0, 0] == -1 and st["tree_node"][0, 0] == 0 and st["tree_hits"][0, 0] == 0
    assert cases[("branch3", 12)]["M"] > 64 and cases[("branch3", 12)]["flat"]["cov"].shape[1] > 8
    # a box of another size, carried forward of the rear axle: against the host text with the centre moved by hand is not bitwise (the
    # kernel subtracts the offset from the difference), so only the rule: offset 0 and a box grown by 2 x 0.3 lowers every clearance by <= 0.3 * sqrt(2)
    c = cases[("branch3", 12)]
    big = hip_predictor.audit_plan([c["flat"]], [c["xs"]], (5.1, 2.6), MARGIN)
    base = hip_predictor.audit_plan([c["flat"]], [c["xs"]], ac.EGO_BOX, MARGIN)
    ac.same_plan(big, ac.host_plan([c["flat"]], [c["xs"]], (5.1, 2.6), MARGIN))
    d = base["node_clear"][0] - big["node_clear"][0]
    assert np.all(d >= -1e-12) and np.all(d <= 0.3 * np.sqrt(2.0) + 1e-12)


def test_centre_offset_moves_the_box_along_its_heading(hip_predictor, cases):
    """center_offset o at state (x, y, yaw) is the box of offset 0 at (x + o cos yaw, y + o sin yaw): to rounding of the moved centre"""
    c = cases[("deep", 4)]
    xs = c["xs"].copy()
    o = 1.4
    got = hip_predictor.audit_plan([c["flat"]], [xs], ac.EGO_BOX + (o,), MARGIN)
    xs[:, :, 0] += o * np.cos(xs[:, :, 3])
    xs[:, :, 1] += o * np.sin(xs[:, :, 3])
    want = hip_predictor.audit_plan([c["flat"]], [xs], ac.EGO_BOX, MARGIN)
    assert np.abs(got["node_clear"][0] - want["node_clear"][0]).max() < 1e-9 and np.array_equal(got["node_agent"][0], want["node_agent"][0])


def _tiled(flat, a, M=None):
    """the branch3 tree with a agents: its exo agents repeated with shifted means (and a little more sigma per repeat)"""
    M = len(flat["parent"]) if M is None else M
    mean, cov = np.zeros((M, a, 2), np.float32), np.zeros((M, a), np.float32)
    a0 = flat["cov"].shape[1]
    for j in range(1, a):
        src, rep = 1 + (j - 1) % (a0 - 1), (j - 1) // (a0 - 1)
        mean[:, j] = flat["mean"][:M, src] + np.float32(1.3 * rep) * np.array([1.0, -0.6], np.float32)
        cov[:, j] = flat["cov"][:M, src] + np.float32(0.05 * rep)
    par = flat["parent"][:M].copy()
    par[0] = -1
    return dict(parent=par, prob=flat["prob"][:M].copy(), mean=mean, cov=cov)


def test_launch_shapes(hip_predictor, cases):
    hp = hip_predictor
    flats = [cases[k]["flat"] for k in FIXTURES]
    n_max = 300
    xs = [_many(cases[k]["xs"], n_max) for k in FIXTURES]
    # the yardstick: one candidate on one tree per call
    single = [[hp.audit_plan([f], [x[c:c + 1]], ac.EGO_BOX, MARGIN) for c in range(n_max)] for f, x in zip(flats, xs)]
    ac.same_plan(hp.audit_plan([flats[1]], [xs[1][7:8]], ac.EGO_BOX, MARGIN), ac.host_plan([flats[1]], [xs[1][7:8]], ac.EGO_BOX, MARGIN))
    for n in (1, 3, CB + 1, n_max):
        got = hp.audit_plan(flats, [x[:n] for x in xs], ac.EGO_BOX, MARGIN)          # all four trees in ONE call: 4 / 12 / 4 / 1 agents
        for t in range(4):
            for c in range(n):
                s = single[t][c]
                assert np.array_equal(got["node_clear"][t][c], s["node_clear"][0][0]) and np.array_equal(got["node_agent"][t][c], s["node_agent"][0][0]), (n, t, c)
                for k in ("tree_min", "tree_node", "tree_agent", "tree_hits", "tree_first", "tree_mass"):
                    assert got[k][c, t] == s[k][0, 0], (n, t, c, k)
    # one trajectory node; agent counts about the staging turn: within one turn, exactly one, one more, two, two and one more
    b3 = cases[("branch3", 12)]
    synth = [_tiled(b3["flat"], 3, M=1)] + [_tiled(b3["flat"], a) for a in (2, CH + 1, CH + 2, 2 * CH + 1, 2 * CH + 2)]
    sx = [b3["xs"][:, :1]] + [b3["xs"]] * 5
    for t in (3, 5):                                      # the last agent, alone in its staging turn, sits on the fit's node 3
        synth[t]["mean"][3, -1] = b3["xs"][1, 3, :2].astype(np.float32)
    got = hp.audit_plan(synth, sx, ac.EGO_BOX, MARGIN)
    ac.same_plan(got, ac.host_plan(synth, sx, ac.EGO_BOX, MARGIN))
    assert got["node_agent"][3][1, 3] == CH + 1 and got["node_agent"][5][1, 3] == 2 * CH + 1 and got["node_clear"][5][1, 3] < -MARGIN
    for t, (f, x) in enumerate(zip(synth, sx)):
        one = hp.audit_plan([f], [x], ac.EGO_BOX, MARGIN)
        assert np.array_equal(one["node_clear"][0], got["node_clear"][t]) and np.array_equal(one["node_agent"][0], got["node_agent"][t])
        assert all(np.array_equal(one[k][:, 0], got[k][:, t]) for k in one if k.startswith("tree_"))


def test_a_nan_state_is_reported_and_stays_where_it_is(hip_predictor, cases):
    hp = hip_predictor
    flats = [cases[k]["flat"] for k in FIXTURES]
    xs = [cases[k]["xs"].copy() for k in FIXTURES]
    clean = hp.audit_plan(flats, xs, ac.EGO_BOX, MARGIN)
    for bad, col in ((np.nan, 3), (np.inf, 0), (-np.inf, 5)):
        x2 = [x.copy() for x in xs]
        x2[1][1, 5, col] = bad
        got = hp.audit_plan(flats, x2, ac.EGO_BOX, MARGIN)
        assert np.isnan(got["node_clear"][1][1, 5]) and got["node_agent"][1][1, 5] == -1
        assert np.isnan(got["tree_min"][1, 1]) and np.isnan(got["tree_mass"][1, 1])
        assert (got["tree_node"][1, 1], got["tree_agent"][1, 1], got["tree_hits"][1, 1], got["tree_first"][1, 1]) == (5, -1, -1, -1)
        keep = np.ones(cases[FIXTURES[1]]["M"], bool)
        keep[5] = False
        assert np.array_equal(got["node_clear"][1][1, keep], clean["node_clear"][1][1, keep])
        for t in range(4):
            rows = [c for c in range(3) if (c, t) != (1, 1)]
            assert np.array_equal(got["node_clear"][t][rows], clean["node_clear"][t][rows]) and np.array_equal(got["node_agent"][t][rows], clean["node_agent"][t][rows])
            for k in ("tree_min", "tree_node", "tree_agent", "tree_hits", "tree_first", "tree_mass"):
                assert np.array_equal(got[k][rows, t], clean[k][rows, t]), (k, t)
        ac.same_plan(got, ac.host_plan(flats, x2, ac.EGO_BOX, MARGIN))


@pytest.mark.parametrize("name,n", [("demo_1", 40), ("demo_3", 16)])
def test_episode_audit_is_the_host_text(hip_predictor, name, n):
    w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
    assert ego.shape == (546, 4) and exo.shape == (546, n, 5)
    one = hip_predictor.audit_episode(ego, exo, valid, boxes, ac.EGO_BOX)
    want = ac.host_episode(ego[None], exo, valid, boxes)
    ac.same_episode(one, want)
    if name == "demo_1":
        assert one["ego_hits"][0] > 0 and one["ego_min"][0] < 0 and one["step_track"][0, one["ego_step"][0]] == one["ego_track"][0] >= 1
    else:
        assert one["ego_hits"][0] == 0 and one["ego_first"][0] == -1 and one["ego_min"][0] > 0
    egos = np.stack([ego, ego + np.array([1.5, -0.75, 0, 0]), ego + np.array([-3.0, 2.0, 0, 0])])
    three = hip_predictor.audit_episode(egos, exo, valid, boxes, ac.EGO_BOX)
    ac.same_episode(three, ac.host_episode(egos, exo, valid, boxes))
    assert np.array_equal(three["step_clear"][0], one["step_clear"][0])
    # a step on which every track is invalid; and more egos than one workgroup takes
    v2 = valid.copy()
    v2[10] = 0
    many = np.stack([ego[:40] + np.array([0.01 * k, 0, 0, 0]) for k in range(65)])
    got = hip_predictor.audit_episode(many, exo[:40], v2[:40], boxes, ac.EGO_BOX)
    ac.same_episode(got, ac.host_episode(many, exo[:40], v2[:40], boxes))
    assert np.all(got["step_clear"][:, 10] == np.inf) and np.all(got["step_track"][:, 10] == -1)


def test_episode_edges(hip_predictor):
    hp = hip_predictor
    # S = 1, n = 1: the ego alone
    r = hp.audit_episode(np.zeros((1, 4)), np.zeros((1, 1, 5)), np.zeros((1, 1), np.uint8), np.ones((1, 2)), ac.EGO_BOX)
    assert r["step_clear"][0, 0] == np.inf and r["step_track"][0, 0] == -1 and r["ego_min"][0] == np.inf
    assert (r["ego_step"][0], r["ego_track"][0], r["ego_hits"][0], r["ego_first"][0]) == (0, -1, 0, -1)
    # more tracks than one staging turn (64), two of them mirrored in the ego's axis: the lower one is named; touching is no hit
    n, S = 131, 3
    g = np.random.default_rng(2)
    exo = np.zeros((S, n, 5))
    exo[:, :, 0], exo[:, :, 1], exo[:, :, 2] = g.uniform(-60, 60, (S, n)), g.uniform(20, 60, (S, n)), g.uniform(-7, 7, (S, n))
    valid = (g.uniform(size=(S, n)) < 0.8).astype(np.uint8)
    boxes = np.stack([g.uniform(0.5, 7, n), g.uniform(0.5, 2.5, n)], 1)
    exo[1, 70], exo[1, 129], boxes[70], boxes[129] = (0, 6, 0, 0, 0), (0, -6, 0, 0, 0), (4, 2), (4, 2)
    valid[1, 70] = valid[1, 129] = 1
    exo[2, 100], boxes[100], valid[2, 100] = (4.25, 0, 0, 0, 0), (4, 2), 1
    ego = np.zeros((S, 4))
    got = hp.audit_episode(ego, exo, valid, boxes, ac.EGO_BOX)
    ac.same_episode(got, ac.host_episode(ego[None], exo, valid, boxes))
    assert got["step_track"][0, 1] == 70 and got["step_clear"][0, 1] == 4.0
    assert got["step_track"][0, 2] == 100 and got["step_clear"][0, 2] == 0.0 and got["ego_hits"][0] == 0 and got["ego_first"][0] == -1


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


def _drive(au, n_plans):
    while au.sim.n_plans < n_plans:
        au.step()
    return au.report()


def test_closed_loop_auditor():
    pl, sim = _make("demo_2", None)
    assert sim._native is not None
    au = audit.EpisodeAuditor(sim)
    rep = _drive(au, 10)
    S = len(rep["times"])
    assert rep["enabled"].sum() > 0 and not rep["enabled"][0] and S == sim.n_steps
    # before the take-over the ego is the recording: the recorded scene's values, by the host text
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_2")
    nb = int((~rep["enabled"]).sum())
    assert rep["times"].tolist() == times[:S] and rep["before"]["steps"].tolist() == list(range(nb))
    rec = ac.host_episode(ego[None, :nb], exo[:nb], valid[:nb], boxes)
    assert np.array_equal(rep["before"]["step_clear"], rec["step_clear"][0]) and np.array_equal(rep["before"]["step_track"], rec["step_track"][0])
    assert rep["before"]["ego_hits"] == 0 and rep["before"]["ego_min"] == rec["ego_min"][0] > 0 and rep["before"]["ego_step"] == rec["ego_step"][0]
    # the whole report: the recorded arrays through the host text
    states = np.stack(au.states)
    assert np.array_equal(states[:nb], ego[:nb]) and not np.array_equal(states[nb + 5:], ego[nb + 5:S])
    want = ac.host_episode(states[None], exo[:S], valid[:S], boxes)
    assert np.array_equal(rep["step_clear"], want["step_clear"][0]) and np.array_equal(rep["step_track"], want["step_track"][0])
    for k in ("ego_min", "ego_step", "ego_track", "ego_hits", "ego_first"):
        assert rep[k] == want[k][0], k
    after = rep["after"]
    assert after["steps"][0] == nb and after["ego_min"] == rep["step_clear"][nb:].min() and after["ego_hits"] == int((rep["step_clear"][nb:] < 0).sum())
    # the last plan, as the loop hands it out
    scen, traj = sim.last_result
    got = audit.audit_plan(scen, traj, planner=pl)
    flat = scen[0]._flat if getattr(scen[0], "_flat", None) is not None else audit._flat_of(scen[0])
    xs = np.asarray(traj[0]._arrays[0])[1:]
    margin = float(pl.traj_tree_opt.config.opt_cfg["w_exo_cov_offset"])
    want = ac.host_plan([flat], [xs[None]], ac.EGO_BOX, margin)
    assert np.array_equal(got["node_clear"][0], want["node_clear"][0][0]) and np.array_equal(got["node_agent"][0], want["node_agent"][0][0])
    for k in ("tree_min", "tree_node", "tree_agent", "tree_hits", "tree_first", "tree_mass"):
        assert got[k][0] == want[k][0, 0], k
    print(f"demo_2 after the take-over: min clearance {after['ego_min']:+.3f} m at step {after['ego_step']}; last plan: {int(got['tree_hits'][0])} of {len(xs)} nodes "
          f"inside a disc, min {float(got['tree_min'][0]):+.3f} m")
    # the Python steps give the same report over the common steps
    pl2, sim2 = _make("demo_2", False)
    assert sim2._native is None
    rep2 = _drive(audit.EpisodeAuditor(sim2), 3)
    S2 = len(rep2["times"])
    assert nb < S2 < S
    for k in ("times", "enabled", "step_clear", "step_track"):
        assert np.array_equal(rep2[k], rep[k][:S2]), k


def _raw_plan(hp, box, margin, trees, n_trees, n_cand, xs, out):
    rc = hp.lib.mind_audit_plan(hp.ctx, C.byref(box) if box is not None else None, margin, trees, n_trees, n_cand,
                                None if xs is None else xs.ctypes.data_as(C.POINTER(C.c_double)), None if out is None else C.byref(out))
    return rc, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode()


def test_error_codes(hip_predictor, cases):
    hp = hip_predictor
    c = cases[("lead", 4)]
    M, xs = c["M"], np.ascontiguousarray(c["xs"])
    keep = []
    trees, _ = hp._cost_trees([c["flat"]], None, keep)
    clear = np.full((3, M), -7.0)
    out = _lib.AuditPlanOut()
    out.node_clear = clear.ctypes.data_as(C.POINTER(C.c_double))
    box = _lib.AuditBox(4.5, 2.0, 0.0)
    ok = (box, MARGIN, trees, 1, 3, xs, out)

    def with_(**kw):
        names = ("box", "margin", "trees", "n_trees", "n_cand", "xs", "out")
        return [kw.get(n, v) for n, v in zip(names, ok)]
    for bad in (dict(box=None), dict(trees=None), dict(out=None), dict(xs=None), dict(n_trees=-1), dict(n_cand=-1), dict(out=_lib.AuditPlanOut()),
                dict(margin=-0.5), dict(margin=np.nan), dict(margin=np.inf), dict(box=_lib.AuditBox(-1.0, 2.0, 0.0)), dict(box=_lib.AuditBox(4.5, np.nan, 0.0)),
                dict(box=_lib.AuditBox(4.5, 2.0, np.inf)), dict(n_cand=(1 << 20) // M + 1)):
        rc, msg = _raw_plan(hp, *with_(**bad))
        assert rc == _lib.MIND_EINVAL and msg.startswith("mind_audit_plan"), (bad, rc, msg)
    for key, idx, val in (("mean", (3, 1, 0), np.nan), ("mean", (0, 2, 1), np.inf), ("cov", (2, 1), np.nan), ("cov", (2, 3), -0.1)):
        f = dict(c["flat"], **{key: c["flat"][key].copy()})
        f[key][idx] = val
        t2, _ = hp._cost_trees([f], None, keep)
        rc, msg = _raw_plan(hp, *with_(trees=t2))
        assert rc == _lib.MIND_EINVAL and f"node {idx[0]} agent {idx[1]}" in msg, msg
    assert np.all(clear == -7.0)                                   # nothing was written
    assert _raw_plan(hp, *with_(n_cand=0))[0] == _lib.MIND_OK and np.all(clear == -7.0)          # no candidate: a successful no-op
    # the episode entry
    S, n = 4, 3
    eo = _lib.AuditEpisodeOut()
    sc = np.full((1, S), -7.0)
    eo.step_clear = sc.ctypes.data_as(C.POINTER(C.c_double))
    ego, exo, valid, boxes = np.zeros((1, S, 4)), np.ones((S, n, 5)), np.ones((S, n), np.uint8), np.ones((n, 2))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def episode(box=box, n_ego=1, S=S, n=n, ego=ego, exo=exo, valid=valid, boxes=boxes, out=eo):
        rc = hp.lib.mind_audit_episode(hp.ctx, C.byref(box) if box is not None else None, n_ego, S, n, dp(ego), dp(exo),
                                       None if valid is None else valid.ctypes.data_as(C.POINTER(C.c_uint8)), dp(boxes), None if out is None else C.byref(out))
        return rc
    nan_ego, nan_exo, inv = ego.copy(), exo.copy(), valid.copy()
    nan_ego[0, 2, 3], nan_exo[1, 2, 0] = np.nan, np.inf
    for bad in (dict(box=None), dict(out=None), dict(out=_lib.AuditEpisodeOut()), dict(n_ego=-1), dict(S=-1), dict(n=0), dict(ego=None), dict(exo=None),
                dict(valid=None), dict(boxes=None), dict(boxes=-boxes), dict(boxes=boxes * np.nan), dict(ego=nan_ego), dict(exo=nan_exo),
                dict(box=_lib.AuditBox(4.5, -2.0, 0.0)), dict(n_ego=(1 << 22) // S + 1)):
        assert episode(**bad) == _lib.MIND_EINVAL, bad
    assert np.all(sc == -7.0)
    inv[1, 2] = 0                                                   # an invalid row may hold anything
    assert episode(exo=nan_exo, valid=inv) == _lib.MIND_OK and np.all(np.isfinite(sc))
    sc[:] = -7.0
    assert episode(n_ego=0) == _lib.MIND_OK and episode(S=0) == _lib.MIND_OK and np.all(sc == -7.0)
    # while a begun tree-iLQR call is pending: MIND_ESTATE, and that call then finishes with its usual result
    s = pr.scene("lead", 4)
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    ref = hp.ilqr_contingency(cfg_w, cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"])
    call = IlqrCall(hp.lib, cfg_w, [s["flat"]], s["x0"], s["lane"], s["tv"], cfg_full=cfg_f)
    call.begin(hp)
    try:
        rc, msg = _raw_plan(hp, *ok)
        assert rc == _lib.MIND_ESTATE and "has not been finished" in msg and np.all(clear == -7.0)
        assert episode() == _lib.MIND_ESTATE and np.all(sc == -7.0)
        with pytest.raises(_lib.MindError):
            hp.audit_plan([c["flat"]], [c["xs"]], ac.EGO_BOX, MARGIN)
    finally:
        xs2, us2, sw, sf = call.wait().finish()
    assert np.array_equal(xs2[0], ref[0][0]) and np.array_equal(us2[0], ref[1][0]) and sw == ref[2] and sf == ref[3]
    rc, _ = _raw_plan(hp, *ok)
    assert rc == _lib.MIND_OK and np.array_equal(clear, ac.host_plan([c["flat"]], [c["xs"]])["node_clear"][0])
