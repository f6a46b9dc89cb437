"""GPU: the road audit on the device (mind_audit_road_plan / mind_audit_road_episode, k_road_boxes; mind_amd/audit.py) against the
library's HOST evaluation of the same header (mind_debug_road_margin with its own sin / cos) reduced by the restatement's rules
(tests/road_geom_restate.py, tests/road_cases.py): every output bit for bit, at the smallest shapes that can go wrong -- vertex counts about
the staging tile, rings ending on and straddling a tile boundary, box counts about the workgroup and off the wave."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import audit_cases as ac
import ilqr_policy_restate as pr
import road_cases as rc
from mind_amd import _lib, audit
from mind_amd.predictor import IlqrCall
from oracle import ilqr as oi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BB, TV = 256, 256          # boxes per workgroup and vertices per staging turn of k_road_boxes (RD_BB, RD_TV)
FIXTURES = [("lead", 4), ("branch3", 12)]
# ring sizes: V = 3; three rings within a turn; V = exactly one turn in one ring; one turn + 1; a ring ending exactly on the turn's
# boundary with more behind it; a ring straddling it; two boundaries, straddled by one ring each, the middle ring ending on the second
SHAPES = [(3,), (5, 9, 4), (TV,), (TV + 1,), (100, TV - 100, 30), (200, 100), (TV - 3, TV + 3, 7), (2 * TV + 40,)]


def _egos(road, n, seed):
    """n boxes about the road as one ego trace [1, n, 4] = (x, y, v, yaw)"""
    b = rc.boxes_about(road, n, seed)
    return np.stack([b[:, 0], b[:, 1], np.full(n, 3.0), b[:, 2]], 1)[None]


@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_road_shapes(hip_predictor, sizes):
    road = rc.synth_road(11 + len(sizes) + sizes[0], sizes, origin=(6500.0, 900.0))
    assert road.n_rings == len(sizes) and len(road.verts) == sum(sizes)
    egos = _egos(road, 100, 5)                          # (100: no multiple of the wave)
    got = hip_predictor.audit_road_episode(egos, road.verts, road.poly_off, rc.EGO_BOX)
    rc.same_episode(got, rc.host_episode(egos, road))
    hit = got["step_margin"][0] < 0
    assert hit.any() and (~hit).any() and set(np.unique(got["step_ring"])) == set(range(len(sizes)))
    assert got["ego_hits"][0] == hit.sum() and got["ego_first"][0] == np.flatnonzero(hit)[0]
    off = hip_predictor.audit_road_episode(egos, road.verts, road.poly_off, rc.EGO_BOX + (1.4,))
    rc.same_episode(off, rc.host_episode(egos, road, rc.EGO_BOX + (1.4,)))


@pytest.mark.parametrize("n", [1, BB, BB + 1, 2 * BB + 37])
def test_box_counts(hip_predictor, n):
    road = rc.synth_road(21, (200, 100), origin=(-300.0, 1200.0))
    egos = _egos(road, n, 9)
    one = hip_predictor.audit_road_episode(egos, road.verts, road.poly_off, rc.EGO_BOX)          # one ego of n steps
    rc.same_episode(one, rc.host_episode(egos, road))
    many = hip_predictor.audit_road_episode(egos.reshape(n, 1, 4), road.verts, road.poly_off, rc.EGO_BOX)     # n egos of one step
    rc.same_episode(many, rc.host_episode(egos.reshape(n, 1, 4), road))
    assert np.array_equal(many["step_margin"][:, 0], one["step_margin"][0]) and np.array_equal(many["ego_min"], one["step_margin"][0])
    assert np.array_equal(many["ego_hits"], (one["step_margin"][0] < 0).astype(np.int32))


@pytest.fixture(scope="module")
def cases(hip_predictor):
    """per scripted tree: the flat tree, three candidate state sets [3, M, 6] (the states of the warm controls, of the full fit, and of the
    full fit's controls plus unit noise) and a road that holds the first half of every trajectory and not its far end"""
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


def _corridor(xs, n_vert, seed):
    """a ring of n_vert vertices about the nodes nearer to the start than the median: an ellipse through the padded bounding box's corners,
    its vertices at jittered angles"""
    p = xs[..., :2].reshape(-1, 2)
    d = np.linalg.norm(p - xs[0, 0, :2], axis=1)
    near = p[d <= np.median(d)]
    lo, hi = near.min(0) - 3.0, near.max(0) + 3.0
    ang = np.sort(np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, n_vert))
    return np.stack([(lo[0] + hi[0]) / 2 + np.sqrt(0.5) * (hi[0] - lo[0]) * np.cos(ang), (lo[1] + hi[1]) / 2 + np.sqrt(0.5) * (hi[1] - lo[1]) * np.sin(ang)], 1)


def _many(xs, n):
    """n distinct candidates from the three of a case: copy c is shifted rigidly by a few centimetres per copy"""
    out = np.stack([xs[c % 3] for c in range(n)])
    out[:, :, 0] += 0.037 * (np.arange(n) // 3)[:, None]
    out[:, :, 1] -= 0.011 * (np.arange(n) // 3)[:, None]
    return out


def test_plan_audit_is_the_host_text(hip_predictor, cases):
    """1 and 257 candidates on the scripted trees, both trees in ONE call against one call per tree and per candidate"""
    hp = hip_predictor
    flats = [cases[k]["flat"] for k in FIXTURES]
    road = audit.Road.from_polygons([_corridor(cases[FIXTURES[0]]["xs"], TV + 9, 1), _corridor(cases[FIXTURES[1]]["xs"], 41, 2)])
    n_max = BB + 1
    xs = [_many(cases[k]["xs"], n_max) for k in FIXTURES]
    want = rc.host_plan(flats, xs, road)
    got = hp.audit_road_plan(flats, xs, road.verts, road.poly_off, rc.EGO_BOX)
    rc.same_plan(got, want)
    for t, k in enumerate(FIXTURES):
        hit = got["node_margin"][t] < 0
        assert hit.any() and (~hit).any() and cases[k]["M"] == hit.shape[1]
        assert np.array_equal(got["tree_hits"][:, t], hit.sum(1)) and np.all(got["tree_mass"][hit.any(1), t] > 0)
        print(k, "nodes off the corridor", int(hit[1].sum()), "of", hit.shape[1], "min", float(got["tree_min"][1, t]))
    first = hp.audit_road_plan(flats, [x[:1] for x in xs], road.verts, road.poly_off, rc.EGO_BOX)
    rc.same_plan(first, rc.host_plan(flats, [x[:1] for x in xs], road))
    for t in range(2):                                   # one call per tree; one call per candidate (a few of them, first and last included)
        alone = hp.audit_road_plan([flats[t]], [xs[t]], road.verts, road.poly_off, rc.EGO_BOX)
        for k in rc.PLAN_KEYS:
            assert np.array_equal(alone[k][0], got[k][t]), (k, t)
        for k in rc.TREE_KEYS:
            assert np.array_equal(alone[k][:, 0], got[k][:, t]), (k, t)
        for c in (0, 1, 2, 63, 64, 255, 256):
            single = hp.audit_road_plan([flats[t]], [xs[t][c:c + 1]], road.verts, road.poly_off, rc.EGO_BOX)
            for k in rc.PLAN_KEYS:
                assert np.array_equal(single[k][0][0], got[k][t][c]), (k, t, c)
            for k in rc.TREE_KEYS:
                assert single[k][0, 0] == got[k][c, t], (k, t, c)


def test_a_nan_state_is_reported_and_stays_where_it_is(hip_predictor, cases):
    hp = hip_predictor
    flats = [cases[k]["flat"] for k in FIXTURES]
    xs = [cases[k]["xs"].copy() for k in FIXTURES]
    road = audit.Road.from_polygons([_corridor(cases[FIXTURES[1]]["xs"], 41, 2)])
    clean = hp.audit_road_plan(flats, xs, road.verts, road.poly_off, rc.EGO_BOX)
    for bad, col in ((np.nan, 3), (np.inf, 0), (-np.inf, 5), (np.nan, 2)):
        x2 = [x.copy() for x in xs]
        x2[1][1, 5, col] = bad
        got = hp.audit_road_plan(flats, x2, road.verts, road.poly_off, rc.EGO_BOX)
        assert np.isnan(got["node_margin"][1][1, 5]) and all(got[k][1][1, 5] == -1 for k in ("node_corner", "node_ring", "node_edge"))
        assert np.isnan(got["tree_min"][1, 1]) and np.isnan(got["tree_mass"][1, 1])
        assert (got["tree_node"][1, 1], got["tree_corner"][1, 1], got["tree_hits"][1, 1], got["tree_first"][1, 1]) == (5, -1, -1, -1)
        keep = np.ones(cases[FIXTURES[1]]["M"], bool)
        keep[5] = False
        for k in rc.PLAN_KEYS:
            assert np.array_equal(got[k][1][1, keep], clean[k][1][1, keep]), k
        for t in range(2):
            rows = [c for c in range(3) if (c, t) != (1, 1)]
            for k in rc.PLAN_KEYS:
                assert np.array_equal(got[k][t][rows], clean[k][t][rows]), (k, t)
            for k in rc.TREE_KEYS:
                assert np.array_equal(got[k][rows, t], clean[k][rows, t]), (k, t)
        rc.same_plan(got, rc.host_plan(flats, x2, road))
    # an episode: the NaN step is reported, its neighbours and the other ego stay
    egos = np.concatenate([_egos(road, 70, 3), _egos(road, 70, 4)])
    base = hp.audit_road_episode(egos, road.verts, road.poly_off, rc.EGO_BOX)
    egos[1, 33, 1] = np.nan
    got = hp.audit_road_episode(egos, road.verts, road.poly_off, rc.EGO_BOX)
    rc.same_episode(got, rc.host_episode(egos, road))
    assert np.isnan(got["step_margin"][1, 33]) and np.isnan(got["ego_min"][1])
    assert (got["ego_step"][1], got["ego_corner"][1], got["ego_hits"][1], got["ego_first"][1]) == (33, -1, -1, -1)
    keep = np.ones(70, bool)
    keep[33] = False
    assert all(np.array_equal(got[k][0], base[k][0]) for k in base) and all(np.array_equal(got[k][1, keep], base[k][1, keep]) for k in rc.STEP_KEYS)


def test_scripted_plan_through_audit_road_rollouts(hip_predictor, cases):
    """the straight-ahead states of a scripted tree, shifted laterally by known amounts on the 40 x 8 m rectangle road: the closed form and
    the expected tree_hits / tree_first / tree_mass"""
    flat = cases[("branch3", 12)]["flat"]
    M = len(flat["parent"])
    depth = np.zeros(M, int)
    for i in range(M):
        depth[i] = 0 if flat["parent"][i] < 0 else depth[flat["parent"][i]] + 1
    road = audit.Road.from_polygons([rc.RECT])
    shifts = np.array([0.0, 1.0, 2.999, 3.0, 3.25, -3.5, -2.0])
    drift = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.125])          # candidate 6 drifts right by 1/8 m per tree level
    xs = np.zeros((len(shifts), M, 6))
    xs[:, :, 0] = -10.0 + 0.25 * depth[None, :]
    xs[:, :, 1] = shifts[:, None] + drift[:, None] * depth[None, :]
    xs[:, :, 2] = 5.0
    got = audit.audit_road_rollouts(flat, xs, road, runtime=hip_predictor)
    want = 3.0 - np.abs(xs[:, :, 1])
    assert depth.max() * 0.25 < 10.0 and np.abs(got["node_margin"] - want).max() <= 1e-12
    assert np.all(got["node_ring"] == 0) and np.array_equal(got["node_edge"], np.where(xs[:, :, 1] >= 0, 2, 0))
    hit = want < 0.0
    assert got["tree_hits"][:6].tolist() == [0, 0, 0, 0, M, M] and got["tree_first"][:6].tolist() == [-1, -1, -1, -1, 0, 0]
    assert got["node_margin"][3].tolist() == [0.0] * M                 # touching: 0.0 and no hit
    mass = 0.0
    for i in range(M):
        mass = mass + np.float64(np.float32(flat["prob"][i]))
    assert got["tree_mass"][:6].tolist() == [0.0, 0.0, 0.0, 0.0, mass, mass] and np.abs(got["tree_min"][:4] - [3.0, 2.0, 0.001, 0.0]).max() <= 1e-12
    assert hit[6].any() and not hit[6, 0] and got["tree_hits"][6] == hit[6].sum() and got["tree_first"][6] == np.flatnonzero(hit[6])[0]
    m6 = 0.0
    for i in np.flatnonzero(hit[6]):
        m6 = m6 + np.float64(np.float32(flat["prob"][i]))
    assert got["tree_mass"][6] == m6 and got["tree_node"][6] == np.argmin(want[6]) and got["tree_corner"][6] == 1
    one = audit.audit_road_rollouts(flat, xs[6], road, runtime=hip_predictor)
    assert all(np.array_equal(one[k], got[k][6]) for k in got)
    rc.same_plan(hip_predictor.audit_road_plan([flat], xs, road.verts, road.poly_off, rc.EGO_BOX), rc.host_plan([flat], [xs], road))


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
    """drive until n_plans plans were made: per step the ego state in force and the control, per plan every trajectory tree's states"""
    states, ctrls, plans = [], [], []
    while sim.n_plans < n_plans:
        planned = stepper()
        states.append(np.array(sim.state, np.float64))
        ctrls.append(np.array(sim.ctrl, np.float64))
        if planned:
            scen, traj = sim.last_result
            plans.append([audit._states_of(tr, len(audit._flat_of(sc)["parent"])).copy() for sc, tr in zip(scen, traj)])
    return np.stack(states), np.stack(ctrls), plans


def _plan_against_host(sim, road):
    scen, traj = sim.last_result
    got = audit.audit_road_plan(scen, traj, road)
    flats = [audit._flat_of(s) for s in scen]
    xs = [audit._states_of(t, len(f["parent"]))[None] for t, f in zip(traj, flats)]
    want = rc.host_plan(flats, xs, road)
    for k in rc.PLAN_KEYS:
        assert len(got[k]) == len(flats) and all(np.array_equal(g, w[0]) for g, w in zip(got[k], want[k])), k
    for k in rc.TREE_KEYS:
        assert np.array_equal(got[k], want[k][0]), k
    return got


@pytest.mark.parametrize("name,native", [("demo_1", None), ("demo_1", False), ("demo_3", None), ("demo_3", False)])
def test_episode_road_auditor_beside_the_planner(name, native):
    """the wrapped run's plans, controls and ego states equal the unwrapped run's bit for bit; before the take-over nothing leaves the road;
    the report is the host entry on the recorded trace.  Nothing is asserted about the steps after the take-over beyond that parity."""
    N = 10 if native is None else 4
    road = rc.demo_road(name)
    pl0, sim0 = _make(name, native)
    assert (sim0._native is not None) == (native is None)
    s0, c0, p0 = _trace(sim0, sim0.step, N)
    pl, sim = _make(name, native)
    au = audit.EpisodeRoadAuditor(sim, road)
    s1, c1, p1 = _trace(sim, au.step, N)
    assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and len(p0) == len(p1) == N
    assert all(len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)) for a, b in zip(p0, p1))
    rep = au.report()
    S = len(rep["times"])
    en = rep["enabled"]
    nb = int((~en).sum())
    assert S == sim.n_steps and 0 < nb < S and not en[:nb].any() and en[nb:].all()
    states = np.stack(au.states)
    w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
    assert rep["times"].tolist() == times[:S] and np.array_equal(states[:nb], ego[:nb])
    want = rc.host_episode(states[None], road)
    for k in rc.STEP_KEYS:
        assert np.array_equal(rep[k], want[k][0]), k
    for k in rc.EGO_KEYS:
        assert rep[k] == want[k][0], k
    before, after = rep["before"], rep["after"]
    assert before["steps"].tolist() == list(range(nb)) and before["ego_hits"] == 0 and before["ego_first"] == -1 and before["ego_min"] > 0
    rec = rc.host_episode(ego[None, :nb], road)
    assert np.array_equal(before["step_margin"], rec["step_margin"][0]) and before["ego_min"] == rec["ego_min"][0] and before["ego_step"] == rec["ego_step"][0]
    assert after["steps"].tolist() == list(range(nb, S)) and np.array_equal(after["step_margin"], rep["step_margin"][nb:])
    assert after["ego_hits"] == int((rep["step_margin"][nb:] < 0).sum()) and after["ego_min"] == rep["step_margin"][nb:].min()
    plan = _plan_against_host(sim, road)
    print(name, "native" if native is None else "python", "steps", S, "before: min", before["ego_min"], "after: min", after["ego_min"], "hits",
          after["ego_hits"], "| last plan: trees", len(plan["tree_min"]), "min", plan["tree_min"].tolist(), "nodes off the road", plan["tree_hits"].tolist())


def test_a_real_plan_on_the_demo_4_road():
    """the 385-vertex road (two staging turns) with the states of a real plan() result"""
    road = rc.demo_road("demo_4")
    assert len(road.verts) == 385
    pl, sim = _make("demo_4", None)
    _trace(sim, sim.step, 2)
    plan = _plan_against_host(sim, road)
    assert np.all(np.isfinite(plan["tree_min"]))
    print("demo_4 last plan: min", plan["tree_min"].tolist(), "nodes off the road", plan["tree_hits"].tolist())


def test_error_codes(hip_predictor, cases):
    hp = hip_predictor
    c = cases[("lead", 4)]
    M, xs = c["M"], np.ascontiguousarray(c["xs"])
    keep = []
    trees, _ = hp._cost_trees([c["flat"]], None, keep)
    road = audit.Road.from_polygons([rc.RECT, [(30, 0), (40, 0), (35, 5)]])
    margin = np.full((3, M), -7.0)
    out = _lib.AuditRoadPlanOut()
    out.node_margin = margin.ctypes.data_as(C.POINTER(C.c_double))
    box = _lib.AuditBox(4.5, 2.0, 0.0)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    nan_v = road.verts.copy()
    nan_v[6, 0] = np.nan
    bad_road = (dict(verts=None), dict(off=None), dict(P=0), dict(P=-2), dict(off=[1, 4, 7]), dict(off=[0, 2, 7]), dict(off=[0, 5, 7]), dict(off=[0, 7, 4]),
                dict(verts=nan_v), dict(P=(1 << 16) + 1), dict(box=None), dict(box=_lib.AuditBox(-1.0, 2.0, 0.0)), dict(box=_lib.AuditBox(4.5, np.nan, 0.0)),
                dict(box=_lib.AuditBox(4.5, 2.0, np.inf)), dict(out=None))

    def plan(box=box, verts=road.verts, off=road.poly_off, P=2, trees=trees, n_trees=1, n_cand=3, xs=xs, out=out):
        offs = None if off is None else np.ascontiguousarray(off, np.int32)
        rc_ = hp.lib.mind_audit_road_plan(hp.ctx, None if box is None else C.byref(box), dp(verts), ip(offs), P, trees, n_trees, n_cand, dp(xs),
                                          None if out is None else C.byref(out))
        return rc_, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode()
    for bad in bad_road + (dict(trees=None), dict(xs=None), dict(n_trees=-1), dict(n_cand=-1), dict(out=_lib.AuditRoadPlanOut()), dict(n_cand=(1 << 20) // M + 1)):
        r, msg = plan(**bad)
        assert r == _lib.MIND_EINVAL and msg.startswith("mind_audit_road_plan"), (bad, r, msg)
    assert np.all(margin == -7.0)                                  # nothing was written
    assert plan(n_cand=0)[0] == _lib.MIND_OK and np.all(margin == -7.0)          # no candidate: a successful no-op
    # the episode entry
    S = 4
    eo = _lib.AuditRoadEpisodeOut()
    sm = np.full((1, S), -7.0)
    eo.step_margin = sm.ctypes.data_as(C.POINTER(C.c_double))
    ego = np.zeros((1, S, 4))

    def episode(box=box, verts=road.verts, off=road.poly_off, P=2, n_ego=1, S=S, ego=ego, out=eo):
        offs = None if off is None else np.ascontiguousarray(off, np.int32)
        return hp.lib.mind_audit_road_episode(hp.ctx, None if box is None else C.byref(box), dp(verts), ip(offs), P, n_ego, S, dp(ego),
                                              None if out is None else C.byref(out))
    for bad in bad_road + (dict(n_ego=-1), dict(S=-1), dict(ego=None), dict(out=_lib.AuditRoadEpisodeOut()), dict(n_ego=(1 << 22) // S + 1)):
        assert episode(**bad) == _lib.MIND_EINVAL, bad
    assert np.all(sm == -7.0)
    assert episode(n_ego=0) == _lib.MIND_OK and episode(S=0) == _lib.MIND_OK and np.all(sm == -7.0)
    # while a begun tree-iLQR call is pending: MIND_ESTATE, and that call then finishes with its usual result
    s = pr.scene("lead", 4)
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    ref = hp.ilqr_contingency(cfg_w, cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"])
    call = IlqrCall(hp.lib, cfg_w, [s["flat"]], s["x0"], s["lane"], s["tv"], cfg_full=cfg_f)
    call.begin(hp)
    try:
        r, msg = plan()
        assert r == _lib.MIND_ESTATE and "has not been finished" in msg and np.all(margin == -7.0)
        assert episode() == _lib.MIND_ESTATE and np.all(sm == -7.0)
        with pytest.raises(_lib.MindError):
            hp.audit_road_plan([c["flat"]], [c["xs"]], road.verts, road.poly_off, rc.EGO_BOX)
    finally:
        xs2, us2, sw, sf = call.wait().finish()
    assert np.array_equal(xs2[0], ref[0][0]) and np.array_equal(us2[0], ref[1][0]) and sw == ref[2] and sf == ref[3]
    assert plan()[0] == _lib.MIND_OK and np.array_equal(margin, rc.host_plan([c["flat"]], [c["xs"]], road)["node_margin"][0])
    assert episode() == _lib.MIND_OK
    assert sm[0].tolist() == [3.0] * S
