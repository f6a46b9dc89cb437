"""GPU: the lane audit on the device (mind_audit_lane_plan / mind_audit_lane_episode, k_lane_boxes<1>, k_lane_boxes<2>, k_lane_progress;
mind_amd/audit.py) against the library's HOST evaluation of the same header (mind_debug_lane_project with its own sin / cos) reduced by the
restatement's rules (tests/lane_geom_restate.py, tests/lane_cases.py): every output bit for bit (NaN equal to NaN), in both forms, at the
smallest shapes that can go wrong -- vertex counts about the staging tile, lanes ending on and beginning a tile, the pair of vertices that
is no segment lying across a tile boundary, box counts about the wave and the workgroup."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import audit_cases as ac
import ilqr_policy_restate as pr
import lane_cases as lc
from mind_amd import _lib, audit
from mind_amd.predictor import IlqrCall
from oracle import ilqr as oi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BB, TV = 256, 256          # boxes per workgroup of k_lane_boxes<1> and vertices per staging turn (LG_BB, LG_TV)
FORM_RULE_ROWS = 1 << 17   # LG_FORM2_MAX_ROWS: form 0 is form 2 up to here, form 1 above
# lane sizes.  One lane: V = 2, one turn less one, exactly one turn, one turn + 1, two turns and a bit.  Two lanes: the first ending exactly at
# the end of a turn (the next begins the next turn), its last vertex the first of the next turn, the second beginning on a turn's last
# vertex; V = 2 TV + 37 split inside the second turn.  21 lanes: two-vertex lanes, a boundary on each of two turn ends, a long tail.
SHAPES = [(2,), (TV - 1,), (TV,), (TV + 1,), (2 * TV + 37,), (TV, 40), (TV + 1, 40), (TV - 1, 40), (TV + 10, TV + 27), (2, 2),
          (2,) * 6 + (30,) * 8 + (4,) + (100, TV - 100) + (9,) * 3 + (2 * TV + 37 - 27,)]
FIXTURES = [("lead", 4), ("branch3", 12)]


def _egos(lanes, n, seed):
    """n boxes about the lanes as one ego trace [1, n, 4] = (x, y, v, yaw)"""
    b = lc.boxes_about(lanes, n, seed)
    return np.stack([b[:, 0], b[:, 1], np.full(n, 3.0), b[:, 2]], 1)[None]


def _episode(hp, egos, lanes, form, box=lc.EGO_BOX, cos_flow=lc.COS_FLOW, bound=lc.BOUND):
    return hp.audit_lane_episode(egos, lanes.verts, lanes.lane_off, box, cos_flow, bound, form)


@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: f"P{len(s)}V{sum(s)}_{s[0]}")
def test_lane_shapes(hip_predictor, sizes):
    assert len(SHAPES[-1]) == 21 and sum(SHAPES[-1][:15]) == TV and sum(SHAPES[-1][:17]) == 2 * TV
    lanes = lc.synth_lanes(11 + len(sizes) + sizes[0], sizes, origin=(6500.0, 900.0))
    assert lanes.n_lanes == len(sizes) and len(lanes.verts) == sum(sizes)
    egos = _egos(lanes, 100, 5)                         # (100: no multiple of the wave)
    want = lc.host_episode(egos, lanes)
    for form in (1, 2, 0):
        lc.same_episode(_episode(hip_predictor, egos, lanes, form), want)
    hit = want["step_margin"][0] < 0
    assert hit.any() and (~hit).any() and len(np.unique(want["step_lane"][0])) >= min(len(sizes), 2)
    assert want["ego_hits"][0] == hit.sum() and want["ego_first"][0] == np.flatnonzero(hit)[0]
    off = (4.5, 2.0, 1.4)
    for form in (1, 2):
        lc.same_episode(_episode(hip_predictor, egos, lanes, form, off, 0.2, 2.0), lc.host_episode(egos, lanes, off, 0.2, 2.0))


def test_no_segment_across_a_tile_boundary(hip_predictor):
    """lane 0's last vertex is the last of the first staging turn, lane 1's first vertex the first of the second, and the line between them
    passes through the pose: the reported distance is the real segments' (3 m to the end of lane 0), not 0 -- in both forms; then the same
    with the pair inside a turn and with lane 0's end ON the second turn's first vertex"""
    for n0 in (TV, TV - 7, TV + 1):
        x_end = float(n0 - 1)
        lane0 = np.stack([np.arange(n0, dtype=np.float64), np.zeros(n0)], 1)
        lane1 = np.stack([x_end + np.arange(40, dtype=np.float64), np.full(40, 8.0)], 1)
        lanes = audit.Lanes.from_polylines([lane0, lane1])
        egos = np.array([[[x_end, 3.0, 2.0, 0.0], [x_end, 6.0, 2.0, 0.0], [x_end, 4.0, 2.0, 0.0], [x_end - 0.5, 1.0, 2.0, 0.0]]])
        want = lc.host_episode(egos, lanes)
        assert want["step_lat"][0, 0].tolist() == [3.0, -2.0, 4.0, 1.0] and want["step_lane"][0, 0].tolist() == [0, 1, 0, 0]
        assert want["step_s"][0, 0].tolist() == [x_end, 0.0, x_end, x_end - 0.5] and want["step_edge"][0, 0].tolist() == [n0 - 2, 0, n0 - 2, n0 - 2]
        for form in (1, 2, 0):
            lc.same_episode(_episode(hip_predictor, egos, lanes, form), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, BB, BB + 1])
def test_box_counts(hip_predictor, n):
    lanes = lc.synth_lanes(21, (200, 100), origin=(-300.0, 1200.0))
    egos = _egos(lanes, n, 9)
    want_one, want_many = lc.host_episode(egos, lanes), lc.host_episode(egos.reshape(n, 1, 4), lanes)
    for form in (1, 2, 0):
        one = _episode(hip_predictor, egos, lanes, form)                                  # one ego of n steps
        lc.same_episode(one, want_one)
        many = _episode(hip_predictor, egos.reshape(n, 1, 4), lanes, form)                # n egos of one step
        lc.same_episode(many, want_many)
        assert np.array_equal(many["step_margin"][:, 0], one["step_margin"][0], equal_nan=True) and np.all(many["ego_progress"] == 0.0)
    assert np.array_equal(want_many["ego_hits"], (want_one["step_margin"][0] < 0).astype(np.int32))


def test_form_0_above_the_rule(hip_predictor):
    """more rows than the library's rule gives to form 2: form 0 (then form 1) and both forced forms equal the host text; few vertices and
    one step per ego keep it quick"""
    lanes = lc.synth_lanes(5, (9, 7), origin=(3000.0, 1500.0))
    n = FORM_RULE_ROWS + 77
    egos = _egos(lanes, n, 3).reshape(n, 1, 4)
    res = _lib.lane_project(egos.reshape(-1, 4)[:, [0, 1, 3]], lc.EGO_BOX, lanes.verts, lanes.lane_off, lc.COS_FLOW, lc.BOUND)
    for form in (0, 1, 2):
        got = _episode(hip_predictor, egos, lanes, form)
        for k in lc.BOX_KEYS:
            assert np.array_equal(got["step_" + k][:, :, 0], res[k], equal_nan=True), (form, k)
        assert np.array_equal(got["step_margin"][:, 0], res["margin"]) and np.array_equal(got["ego_min"], res["margin"])
        assert np.array_equal(got["ego_lane"], res["lane"][1]) and np.array_equal(got["ego_hits"], (res["margin"] < 0).astype(np.int32))


def test_a_nan_row_is_reported_and_stays_where_it_is(hip_predictor):
    lanes = lc.synth_lanes(21, (200, 100), origin=(-300.0, 1200.0))
    egos = np.concatenate([_egos(lanes, 70, 3), _egos(lanes, 70, 4)])
    base = lc.host_episode(egos, lanes)
    keep = np.ones(70, bool)
    keep[33] = False
    for bad, col in ((np.nan, 1), (np.inf, 0), (-np.inf, 3), (np.nan, 2)):
        e2 = egos.copy()
        e2[1, 33, col] = bad
        want = lc.host_episode(e2, lanes)
        for form in (1, 2):
            got = _episode(hip_predictor, e2, lanes, form)
            lc.same_episode(got, want)
            assert np.isnan(got["step_margin"][1, 33]) and np.isnan(got["ego_min"][1]) and np.all(got["step_lane"][:, 1, 33] == -1)
            assert all(np.isnan(got["step_" + k][:, 1, 33]).all() for k in ("lat", "s", "along", "across"))
            assert (got["ego_step"][1], got["ego_lane"][1], got["ego_hits"][1], got["ego_first"][1]) == (33, -1, -1, -1)
            for k in lc.STEP_KEYS:
                assert np.array_equal(got[k][..., 0, :], base[k][..., 0, :], equal_nan=True) and np.array_equal(got[k][..., 1, keep], base[k][..., 1, keep], equal_nan=True), k
            assert all(got[k][0] == base[k][0] for k in lc.EGO_KEYS)
            assert np.isfinite(got["ego_progress"][1])          # (the NaN step has lane -1: the progress passes over it)


@pytest.fixture(scope="module")
def plan_case():
    """the two scripted trees with two candidate state sets each, made without a solver: node i of depth d sits d x 1.5 m along the tree's
    target lane, candidate 0 on the centreline, candidate 1 drifting left by 0.4 m a level and turned 0.3 rad; the lanes are the two target
    lanes, each once more reversed and 3.6 m to the left (the oncoming lane), and a far cross street"""
    flats, xs, polylines = [], [], []
    for t, (kind, a) in enumerate(FIXTURES):
        s = pr.scene(kind, a)
        flat, lane = s["flat"], np.asarray(s["lane"], np.float64)[:, :2] + np.array([0.0, 40.0 * t])
        M = len(flat["parent"])
        depth = np.zeros(M, int)
        for i in range(M):
            depth[i] = 0 if flat["parent"][i] < 0 else depth[flat["parent"][i]] + 1
        seg = np.diff(lane, axis=0)
        cum = np.concatenate([[0.0], np.cumsum(np.linalg.norm(seg, axis=1))])
        arc = np.minimum(2.0 + 1.5 * depth, cum[-1] - 1.0)
        k = np.clip(np.searchsorted(cum, arc, side="right") - 1, 0, len(seg) - 1)
        e = seg[k] / np.linalg.norm(seg[k], axis=1, keepdims=True)
        on = lane[k] + (arc - cum[k])[:, None] * e
        left = np.stack([-e[:, 1], e[:, 0]], 1)
        yaw = np.arctan2(e[:, 1], e[:, 0])
        x = np.zeros((2, M, 6))
        x[0, :, :2], x[0, :, 3] = on, yaw
        x[1, :, :2], x[1, :, 3] = on + (0.4 * depth)[:, None] * left, yaw + 0.3
        x[:, :, 2] = 5.0
        flats.append(flat)
        xs.append(x)
        polylines += [lane, lane[::-1] + 3.6 * np.array([0.0, 1.0])]
    polylines.append(np.stack([np.full(30, 500.0), np.linspace(-50.0, 50.0, 30)], 1))
    return flats, xs, audit.Lanes.from_polylines(polylines)


def test_plan_audit_is_the_host_text(hip_predictor, plan_case):
    """a two-tree plan with two candidates: node arrays against the host text, tree folds and tree_progress against the numpy restatements
    of their rules; one call for both trees against one call per tree and per candidate, in both forms"""
    hp = hip_predictor
    flats, xs, lanes = plan_case
    want = lc.host_plan(flats, xs, lanes)
    got = hp.audit_lane_plan(flats, xs, lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, lc.BOUND)
    lc.same_plan(got, want)
    for form in (1, 2):
        lc.same_plan(hp.audit_lane_plan(flats, xs, lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, lc.BOUND, form), want)
    for t in range(2):
        M = len(flats[t]["parent"])
        assert np.all(want["node_lane"][t][:, 0] == 2 * t) and np.abs(want["node_lat"][t][1, 0]).max() < 1e-9            # candidate 0: on its lane
        assert want["tree_hits"][0, t] == 0 and 0 < want["tree_hits"][1, t] < M and want["tree_first"][1, t] > 0       # candidate 1 drifts off it
        assert want["tree_progress"][0, t] > 1.0 and want["tree_mass"][1, t] > 0
        # the progress of candidate 0 is the probability-weighted arc length of the tree's edges: 1.5 m a level until the lane's end
        prob = flats[t]["prob"].astype(np.float64)
        s0 = want["node_s"][t][0, 0]
        par = np.asarray(flats[t]["parent"])
        assert abs(want["tree_progress"][0, t] - sum(prob[i] * (s0[i] - s0[par[i]]) for i in range(M) if par[i] >= 0)) < 1e-9
        alone = hp.audit_lane_plan([flats[t]], [xs[t]], lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, lc.BOUND)
        for k in lc.PLAN_KEYS:
            assert np.array_equal(alone[k][0], got[k][t], equal_nan=True), (k, t)
        for k in lc.TREE_KEYS:
            assert np.array_equal(alone[k][:, 0], got[k][:, t], equal_nan=True), (k, t)
    # through mind_amd.audit: C candidates on one tree, and one [M, 6] set
    roll = audit.audit_lane_rollouts(flats[1], xs[1], lanes, runtime=hp)
    for k in lc.PLAN_KEYS:
        assert np.array_equal(roll[k], want[k][1], equal_nan=True), k
    for k in lc.TREE_KEYS:
        assert np.array_equal(roll[k], want[k][:, 1], equal_nan=True), k
    with np.errstate(invalid="ignore"):
        assert np.array_equal(roll["node_heading_err"], np.arctan2(roll["node_across"], roll["node_along"]), equal_nan=True)
    assert np.abs(roll["node_heading_err"][1, 0]).max() < 1e-9 and np.abs(roll["node_heading_err"][1, 1] - 0.3).max() < 1e-9
    one = audit.audit_lane_rollouts(flats[1], xs[1][1], lanes, runtime=hp)
    assert all(np.array_equal(one[k], roll[k][..., 1, :] if k.startswith("node_") else roll[k][1], equal_nan=True) for k in roll)
    # a NaN node: reported, its tree NaN, its neighbours and the other tree untouched
    x2 = [x.copy() for x in xs]
    x2[1][1, 5, 4] = np.nan
    bad = hp.audit_lane_plan(flats, x2, lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, lc.BOUND)
    lc.same_plan(bad, lc.host_plan(flats, x2, lanes))
    assert np.isnan(bad["tree_min"][1, 1]) and (bad["tree_node"][1, 1], bad["tree_lane"][1, 1], bad["tree_hits"][1, 1]) == (5, -1, -1)
    assert np.isfinite(bad["tree_progress"][1, 1]) and np.array_equal(bad["tree_min"][:, 0], got["tree_min"][:, 0])


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


@pytest.mark.parametrize("native", [None, False], ids=["native", "python"])
def test_episode_lane_auditor_beside_the_planner(native):
    """demo_1 until two plans past the take-over, native and Python steps: the report is the host text on the recorded states, `before` /
    `after` partition the steps, and the last plan's audit is the host text too.  Nothing is asserted about how well the planner keeps
    its lane."""
    pl, sim = _make("demo_1", native)
    assert (sim._native is not None) == (native is None)
    lanes = audit.Lanes.from_semantic_map(sim.world.smp)
    au = audit.EpisodeLaneAuditor(sim, lanes, audit.DEFAULT_LANE_ANGLE, audit.DEFAULT_LANE_BOUND)
    while sim.n_plans < 2:
        au.step()
    rep = au.report()
    S = len(rep["times"])
    en = rep["enabled"]
    nb = int((~en).sum())
    assert S == sim.n_steps and 0 < nb < S and not en[:nb].any() and en[nb:].all()
    states = np.stack(au.states)
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_1")
    assert rep["times"].tolist() == times[:S] and np.array_equal(states[:nb], ego[:nb])
    want = lc.host_episode(states[None], lanes)
    for k in lc.BOX_KEYS:
        assert np.array_equal(rep["step_" + k], want["step_" + k][1, 0], equal_nan=True) and np.array_equal(rep["step_" + k + "_any"], want["step_" + k][0, 0]), k
    assert np.array_equal(rep["step_margin"], want["step_margin"][0])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(rep["step_heading_err"], np.arctan2(rep["step_across"], rep["step_along"]), equal_nan=True)
    for k in lc.EGO_KEYS:
        assert rep[k] == want[k][0], k
    before, after = rep["before"], rep["after"]
    assert before["steps"].tolist() == list(range(nb)) and after["steps"].tolist() == list(range(nb, S))
    rec = lc.host_episode(ego[None, :nb], lanes)
    assert before["ego_hits"] == 0 and before["ego_first"] == -1 and before["ego_min"] == rec["ego_min"][0] > 0 and before["ego_step"] == rec["ego_step"][0]
    assert np.array_equal(before["step_lat"], rec["step_lat"][1, 0]) and (before["ego_progress"], before["ego_back"]) == (rec["ego_progress"][0], rec["ego_back"][0])
    tail = lc.host_episode(states[None, nb:], lanes)
    assert np.array_equal(after["step_margin"], rep["step_margin"][nb:]) and after["ego_min"] == tail["ego_min"][0] and after["ego_step"] == nb + tail["ego_step"][0]
    assert after["ego_hits"] == tail["ego_hits"][0] and (after["ego_progress"], after["ego_back"]) == (tail["ego_progress"][0], tail["ego_back"][0])
    # the last plan
    scen, traj = sim.last_result
    got = audit.audit_lane_plan(scen, traj, lanes)
    flats = [audit._flat_of(s) for s in scen]
    xs = [audit._states_of(t, len(f["parent"]))[None] for t, f in zip(traj, flats)]
    plan = lc.host_plan(flats, xs, lanes)
    for k in lc.PLAN_KEYS:
        assert len(got[k]) == len(flats) and all(np.array_equal(g, p[..., 0, :], equal_nan=True) for g, p in zip(got[k], plan[k])), k
    for k in lc.TREE_KEYS:
        assert np.array_equal(got[k], plan[k][0], equal_nan=True), k
    print("demo_1", "native" if native is None else "python", "steps", S, "before: min margin", before["ego_min"], "progress", before["ego_progress"], "| after: min",
          after["ego_min"], "hits", after["ego_hits"], "progress", after["ego_progress"], "| last plan: trees", len(flats), "progress", got["tree_progress"].tolist())


def test_error_codes(hip_predictor, plan_case):
    hp = hip_predictor
    flats, xs_all, _ = plan_case
    flat, xs = flats[0], np.ascontiguousarray(xs_all[0])
    M = len(flat["parent"])
    keep = []
    trees, _ = hp._cost_trees([flat], None, keep)
    lanes = audit.Lanes.from_polylines([[(0.0, 0.0), (8.0, 0.0), (16.0, 0.0)], [(0.0, 0.0), (8.0, 0.0), (8.0, 8.0)], [(0.0, 5.0), (9.0, 5.0)]])
    margin = np.full((2, M), -7.0)
    out = _lib.AuditLanePlanOut()
    out.node_margin = margin.ctypes.data_as(C.POINTER(C.c_double))
    box, good = _lib.AuditBox(4.5, 2.0, 0.0), _lib.AuditLaneCfg(lc.COS_FLOW, 5.0, 0)
    cfg = lambda *a: _lib.AuditLaneCfg(*a)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    nan_v = lanes.verts.copy()
    nan_v[6, 0] = np.nan
    bad_lanes = (dict(verts=None), dict(off=None), dict(P=0), dict(P=-2), dict(P=(1 << 16) + 1), dict(off=[1, 3, 6, 8]), dict(off=[0, 1, 6, 8]), dict(off=[0, 3, 3, 8]),
                 dict(off=[0, 6, 3, 8]), dict(verts=nan_v), dict(box=None), dict(box=_lib.AuditBox(-1.0, 2.0, 0.0)), dict(box=_lib.AuditBox(4.5, np.nan, 0.0)),
                 dict(box=_lib.AuditBox(4.5, 2.0, np.inf)), dict(cfg=None), dict(cfg=cfg(1.5, 5.0, 0)), dict(cfg=cfg(np.nan, 5.0, 0)), dict(cfg=cfg(0.5, 0.0, 0)),
                 dict(cfg=cfg(0.5, np.inf, 0)), dict(cfg=cfg(0.5, np.nan, 0)), dict(cfg=cfg(0.5, 5.0, 3)), dict(cfg=cfg(0.5, 5.0, -1)), dict(out=None))

    def plan(box=box, cfg=good, verts=lanes.verts, off=lanes.lane_off, P=3, trees=trees, n_trees=1, n_cand=2, xs=xs, out=out):
        rc_ = hp.lib.mind_audit_lane_plan(hp.ctx, None if box is None else C.byref(box), None if cfg is None else C.byref(cfg), dp(verts), ip(off), P, trees, n_trees,
                                          n_cand, dp(xs), None if out is None else C.byref(out))
        return rc_, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode()
    for bad in bad_lanes + (dict(trees=None), dict(xs=None), dict(n_trees=-1), dict(n_cand=-1), dict(out=_lib.AuditLanePlanOut()), dict(n_cand=(1 << 20) // M + 1)):
        r, msg = plan(**bad)
        assert r == _lib.MIND_EINVAL and msg.startswith("mind_audit_lane_plan"), (bad, r, msg)
    assert np.all(margin == -7.0)                                  # nothing was written
    assert plan(n_cand=0)[0] == _lib.MIND_OK and np.all(margin == -7.0)          # no candidate: a successful no-op
    # the episode entry
    S = 4
    eo = _lib.AuditLaneEpisodeOut()
    sm = np.full((1, S), -7.0)
    eo.step_margin = sm.ctypes.data_as(C.POINTER(C.c_double))
    ego = np.zeros((1, S, 4))
    ego[0, :, 1] = 2.0

    def episode(box=box, cfg=good, verts=lanes.verts, off=lanes.lane_off, P=3, n_ego=1, S=S, ego=ego, out=eo):
        return hp.lib.mind_audit_lane_episode(hp.ctx, None if box is None else C.byref(box), None if cfg is None else C.byref(cfg), dp(verts), ip(off), P, n_ego, S,
                                              dp(ego), None if out is None else C.byref(out))
    for bad in bad_lanes + (dict(n_ego=-1), dict(S=-1), dict(ego=None), dict(out=_lib.AuditLaneEpisodeOut()), dict(n_ego=(1 << 22) // S + 1)):
        assert episode(**bad) == _lib.MIND_EINVAL, bad
    assert np.all(sm == -7.0)
    assert episode(n_ego=0) == _lib.MIND_OK and episode(S=0) == _lib.MIND_OK and np.all(sm == -7.0)
    # the Python layer raises on the same, before the library is asked
    for bad in (lambda: hp.audit_lane_episode(ego, lanes.verts, [0, 3, 6, 7], lc.EGO_BOX, 0.5, 5.0), lambda: hp.audit_lane_episode(ego, lanes.verts, lanes.lane_off, lc.EGO_BOX, 1.5, 5.0),
                lambda: hp.audit_lane_episode(ego, lanes.verts, lanes.lane_off, lc.EGO_BOX, 0.5, -1.0), lambda: hp.audit_lane_episode(ego, lanes.verts, lanes.lane_off, lc.EGO_BOX, 0.5, 5.0, 3),
                lambda: hp.audit_lane_episode(ego[:, :, :3], lanes.verts, lanes.lane_off, lc.EGO_BOX, 0.5, 5.0), lambda: hp.audit_lane_plan([flat], [xs[:, :-1]], lanes.verts, lanes.lane_off, lc.EGO_BOX, 0.5, 5.0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.MindError):
        hp.audit_lane_episode(ego, lanes.verts, [0, 1, 6, 8], lc.EGO_BOX, 0.5, 5.0)
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
            hp.audit_lane_plan([flat], [xs], lanes.verts, lanes.lane_off, lc.EGO_BOX, lc.COS_FLOW, 5.0)
    finally:
        xs2, us2, sw, sf = call.wait().finish()
    assert np.array_equal(xs2[0], ref[0][0]) and np.array_equal(us2[0], ref[1][0]) and sw == ref[2] and sf == ref[3]
    assert plan()[0] == _lib.MIND_OK and np.array_equal(margin, lc.host_plan([flat], [xs], lanes)["node_margin"][0], equal_nan=True)
    assert episode() == _lib.MIND_OK and sm[0].tolist() == [3.0] * S
