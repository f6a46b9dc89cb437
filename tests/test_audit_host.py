"""CPU: the geometry of the clearance audit (mind_amd/csrc/box_geom.h through the host entry mind_debug_box_clearance) against its numpy
restatement (tests/box_geom_restate.py) bit for bit, exact cases at yaw = 0, the library's own sin / cos against numpy's, the four recorded
scenes, and what of the device entries and of mind_amd/audit.py needs no device: argument errors and shape checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_cases as ac
import box_geom_restate as rs
from mind_amd import _lib, audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_pairs(n, seed):
    """rectangles a, b as (x, y, yaw, L, W) at AV2-size coordinates: offsets up to +-300 m, yaw in +-7, a fifth of the pairs near each other"""
    g = np.random.default_rng(seed)
    a = np.stack([g.uniform(-6000, 6000, n), g.uniform(-6000, 6000, n), g.uniform(-7, 7, n), g.uniform(0.3, 8, n), g.uniform(0.3, 3, n)], 1)
    off = g.uniform(-300, 300, (n, 2))
    off[::5] = g.uniform(-6, 6, (len(off[::5]), 2))
    b = np.stack([a[:, 0] + off[:, 0], a[:, 1] + off[:, 1], g.uniform(-7, 7, n), g.uniform(0.3, 8, n), g.uniform(0.3, 3, n)], 1)
    return a, b


def _trig(a, b):
    return np.stack([np.cos(a[:, 2]), np.sin(a[:, 2]), np.cos(b[:, 2]), np.sin(b[:, 2])], 1)


def _restate(kind, a, b, tg):
    if kind == 0:
        return np.array([rs.point_rect(b[i, 0] - a[i, 0], b[i, 1] - a[i, 1], tg[i, 0], tg[i, 1], a[i, 3], a[i, 4]) - b[i, 2] for i in range(len(a))])
    return np.array([rs.rect_rect(b[i, 0] - a[i, 0], b[i, 1] - a[i, 1], tg[i, 0], tg[i, 1], a[i, 3], a[i, 4], tg[i, 2], tg[i, 3], b[i, 3], b[i, 4])
                     for i in range(len(a))])


# boxes 4 x 2 at yaw = 0 (the 6 x 0.5 box of the fifth case crosses at 90 degrees, its trig handed in as (0, 1) exactly)
EXACT_RECT = [((0, 0, 0, 4, 2), (4, 0, 0, 4, 2), (1, 0, 1, 0), 0.0),
              ((0, 0, 0, 4, 2), (5, 0, 0, 4, 2), (1, 0, 1, 0), 1.0),
              ((0, 0, 0, 4, 2), (5, 5, 0, 4, 2), (1, 0, 1, 0), np.sqrt(np.float64(10.0))),
              ((0, 0, 0, 4, 2), (3, 0, 0, 4, 2), (1, 0, 1, 0), -1.0),
              ((0, 0, 0, 4, 2), (0, 0, np.pi / 2, 6, 0.5), (1, 0, 0, 1), -2.25)]


def test_host_entry_is_the_restatement_bit_for_bit():
    a, b = _random_pairs(2000, 11)
    tg = _trig(a, b)
    for kind in (0, 1):
        bb = b.copy()
        if kind == 0:
            bb[:, 2] = np.random.default_rng(5).uniform(0.0, 6.0, len(b))          # the disc's radius
        got = _lib.box_clearance(kind, a, bb, tg)
        want = _restate(kind, a, bb, tg)
        assert np.array_equal(got, want), (kind, np.abs(got - want).max())
        assert (got < 0).any() and (got > 0).any()
    # the point ego: L = W = 0 is the distance of the centres minus r
    p = a.copy()
    p[:, 3:] = 0.0
    bb = b.copy()
    bb[:, 2] = 1.5
    got = _lib.box_clearance(0, p, bb, tg)
    assert np.array_equal(got, _restate(0, p, bb, tg))
    assert np.abs(got - (np.hypot(bb[:, 0] - p[:, 0], bb[:, 1] - p[:, 1]) - 1.5)).max() <= 1e-12
    # the exact cases, through both
    ea, eb = np.array([c[0] for c in EXACT_RECT], np.float64), np.array([c[1] for c in EXACT_RECT], np.float64)
    et = np.array([c[2] for c in EXACT_RECT], np.float64)
    assert np.array_equal(_lib.box_clearance(1, ea, eb, et), _restate(1, ea, eb, et))


def test_exact_geometry_at_yaw_zero():
    # the trig header at 0: exactly (1, 0) -- a unit box against a far disc along x then measures the offset exactly
    assert _lib.box_clearance(0, [[0, 0, 0, 2, 2]], [[9, 0, 0, 0, 0]])[0] == 8.0
    assert _lib.box_clearance(0, [[0, 0, 0, 2, 2]], [[0, 9, 0, 0, 0]])[0] == 8.0
    assert _lib.box_clearance(1, [[0, 0, 0, 2, 2]], [[9, 0, 0, 2, 4]])[0] == 7.0          # (b's length along x: its cos is exactly 1 too)
    for A, B, tg, want in EXACT_RECT:
        for trig in ([tg], None) if B[2] == 0 else ([tg],):
            got = _lib.box_clearance(1, [A], [B], trig)[0]
            assert got == want, (A, B, got, want)
    assert not (_lib.box_clearance(1, [EXACT_RECT[0][0]], [EXACT_RECT[0][1]])[0] < 0.0)      # touching is no hit
    # the crossed boxes: no corner of either lies inside the other
    A, B = EXACT_RECT[4][0], EXACT_RECT[4][1]
    for cx, cy in ((2, 1), (2, -1), (-2, -1), (-2, 1)):
        assert rs.point_rect(cx, cy, 0.0, 1.0, B[3], B[4]) > 0
    for cx, cy in ((3, 0.25), (3, -0.25), (-3, -0.25), (-3, 0.25)):
        assert rs.point_rect(-cy, cx, 1.0, 0.0, A[3], A[4]) > 0
    # a disc centre inside the box: minus the distance to the nearest edge, minus r
    assert _lib.box_clearance(0, [[0, 0, 0, 4, 2]], [[1.5, 0.25, 0.5, 0, 0]])[0] == -0.5 - 0.5
    assert _lib.box_clearance(0, [[0, 0, 0, 4, 2]], [[0.5, 0.75, 0.5, 0, 0]])[0] == -0.25 - 0.5
    # two discs mirrored in the box axis: equal clearances, the lower index reported
    d = _lib.box_clearance(0, [[0, 0, 0, 4, 2]] * 2, [[3, 2.5, 0.75, 0, 0], [3, -2.5, 0.75, 0, 0]])
    assert d[0] == d[1] and rs.reduce_agents(d) == (d[0], 1)
    flat = dict(parent=np.array([-1], np.int32), prob=np.ones(1, np.float32), mean=np.array([[[0, 0], [3, 2.5], [3, -2.5]]], np.float32),
                cov=np.array([[0, 0.25, 0.25]], np.float32))
    clear, agent = ac.host_plan_nodes(flat, np.zeros((1, 6)), (4, 2), 0.5)
    assert clear[0] == d[0] and agent[0] == 1


def test_disjoint_clearance_is_the_polygon_distance():
    """bg_rect_rect's disjoint branch against brute-force sampling of the edges (independent method; its accuracy is the sample spacing)"""
    g = np.random.default_rng(3)
    n = 0
    while n < 60:
        dx, dy, ya, yb = g.uniform(-12, 12), g.uniform(-12, 12), g.uniform(-7, 7), g.uniform(-7, 7)
        La, Wa, Lb, Wb = g.uniform(1, 8), g.uniform(0.5, 3), g.uniform(1, 8), g.uniform(0.5, 3)
        d = _lib.box_clearance(1, [[0, 0, ya, La, Wa]], [[dx, dy, yb, Lb, Wb]])[0]
        if d <= 0.05:
            continue
        n += 1
        brute = rs.brute_rect_distance(dx, dy, ya, La, Wa, yb, Lb, Wb)
        assert d <= brute + 1e-9 and brute - d < 0.05, (d, brute)


def test_own_trig_against_numpy():
    """trig = NULL (mind_trig.h on the host) against the restatement fed numpy's cos / sin: both are within an ulp and every later operation
    is the same IEEE operation, so ~1e-15 x the pair's offset is expected; the bar is the 1e-9 m the oracle is held to"""
    a, b = _random_pairs(2000, 12)
    tg = _trig(a, b)
    worst = 0.0
    for kind in (0, 1):
        bb = b.copy()
        if kind == 0:
            bb[:, 2] = 1.0
        worst = max(worst, float(np.abs(_lib.box_clearance(kind, a, bb) - _restate(kind, a, bb, tg)).max()))
    print(f"max |own trig - numpy trig| = {worst:.3e} m")
    assert worst <= 1e-9
    assert worst <= 1e-12, "larger than the derivation expects: find out why"


@pytest.fixture(scope="module")
def scene_audits():
    """per recorded scene: the host entry's per-step audit (numpy's cos / sin handed in) and the restatement's"""
    out = {}
    np_trig = lambda yaw: (np.cos(yaw), np.sin(yaw))
    for name in ("demo_1", "demo_2", "demo_3", "demo_4"):
        w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
        out[name] = (ac.host_episode_steps(ego, exo, valid, boxes, ac.EGO_BOX, trig=np_trig),
                     rs.episode_steps(ego, exo, valid, boxes, ac.EGO_BOX, rs.rect_pair_restated()), w)
    return out


@pytest.mark.parametrize("name", ["demo_1", "demo_2", "demo_3", "demo_4"])
def test_recorded_scenes(scene_audits, name):
    (clear, track), (rclear, rtrack), w = scene_audits[name]
    assert np.array_equal(clear, rclear) and np.array_equal(track, rtrack)
    mn, step, trk, hits, first = rs.reduce_ego(clear, track)
    print(f"{name}: min clearance {mn:+.3f} m at step {step} with track {trk} ({w.agent_ids[trk]}), {hits} hit steps of {len(clear)}, first {first}")
    assert len(clear) == int(w.max_step) + 1 and np.isfinite(mn) and 1 <= trk < w.n_agents
    if name == "demo_1":      # the recorded ego overlaps one track's nominal box for a long stretch
        assert hits > 0 and mn < 0.0 and first >= 0 and clear[first] < 0.0 and np.all(clear[:first] >= 0.0)
        assert track[step] == trk and (track[clear < 0.0] == trk).any()
    else:
        assert hits == 0 and first == -1 and mn > 0.0


def test_ego_fold_is_one_restatement_with_the_nan_rule_as_a_parameter(scene_audits):
    """k_audit_episode_egos<false> (clearance) and <true> (road) are one body: on a finite trace the rule changes nothing; a NaN step in
    the middle is passed over without the rule and reported with it; a NaN at step 0 stays the minimum without the rule"""
    import road_geom_restate as rr
    assert rr.reduce_tree is rs.reduce_tree
    for name, ((clear, track), _, _) in scene_audits.items():
        assert rs.reduce_ego(clear, track, nan_step=True) == rs.reduce_ego(clear, track, nan_step=False) == rs.reduce_ego(clear, track), name
        assert rr.reduce_ego(clear, track) == rs.reduce_ego(clear, track), name
    val, tag = np.array([3.0, -1.0, np.nan, -2.5, 4.0]), np.array([7, 8, 9, 10, 11], np.int32)
    assert rs.reduce_ego(val, tag) == (-2.5, 3, 10, 2, 1)
    on = rs.reduce_ego(val, tag, nan_step=True)
    assert np.isnan(on[0]) and on[1:] == (2, -1, -1, -1) and rr.reduce_ego(val, tag)[1:] == on[1:]
    first = rs.reduce_ego(val[::-1][2:], tag[2:])                          # (nan, -1.0, 3.0): nothing compares below a NaN
    assert np.isnan(first[0]) and first[1:] == (0, 9, 1, 1)
    # the partial summaries of the two episode auditors follow the same split
    per = dict(step_clear=val, step_track=tag)
    idx = np.arange(1, 5)
    off = audit._part(per, idx, "step_clear", "track", nan_step=False)
    assert np.isnan(off["ego_min"]) and (off["ego_step"], off["ego_track"], off["ego_hits"], off["ego_first"]) == (2, 9, 2, 1)      # (numpy's argmin)
    on = audit._part(dict(step_margin=val, step_corner=tag), idx, "step_margin", "corner", nan_step=True)
    assert np.isnan(on["ego_min"]) and (on["ego_step"], on["ego_corner"], on["ego_hits"], on["ego_first"]) == (2, -1, -1, -1)
    assert audit._part(per, idx[:0], "step_clear", "track", nan_step=False) is None


def test_box_table():
    assert audit.box_for("vehicle") == (4.5, 2.0) and audit.box_for("PEDESTRIAN") == (0.5, 0.75)
    assert audit.box_for("cyclist") == audit.box_for("MOTORCYCLIST") == (1.5, 0.75) and audit.box_for("bus") == (7.0, 2.1)
    for other in ("unknown", "static", "riderless_bicycle", "construction_cone"):
        assert audit.box_for(other) == (1.0, 1.0)
    w = ac.recorded_scene("demo_3")[0]
    assert audit.box_for(w.object_type(0)) == (4.5, 2.0)


# ---- error surface --------------------------------------------------------------------------------------------------------------------

def test_entries_fail_cleanly_without_a_context():
    lib = _lib.load()
    box = _lib.AuditBox(4.5, 2.0, 0.0)
    assert lib.mind_audit_plan(None, C.byref(box), 2.5, None, 0, 0, None, None) == _lib.MIND_EINVAL
    assert lib.mind_audit_episode(None, C.byref(box), 1, 1, 1, None, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_clearance(2, 0, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_clearance(0, -1, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_clearance(1, 1, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_clearance(1, 0, None, None, None, None) == _lib.MIND_OK
    with pytest.raises(ValueError):
        _lib.box_clearance(3, np.zeros((1, 5)), np.zeros((1, 5)))
    with pytest.raises(ValueError):
        _lib.box_clearance(1, np.zeros((2, 5)), np.zeros((1, 5)))


@pytest.mark.parametrize("name,n_args", [("mind_audit_plan", 8), ("mind_audit_episode", 10), ("mind_debug_box_clearance", 6)])
def test_binding_matches_header(name, n_args):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mind_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
    assert m, f"{name} is not declared in include/mind_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    fn = getattr(_lib.load(), name)
    assert len(args) == len(fn.argtypes) == n_args and fn.restype is C.c_int and name in _lib.EXPORTS
    for a, t in zip(args, fn.argtypes):
        assert ("*" in a) == (t is C.c_void_p or hasattr(t, "contents")), (a, t)
    assert C.sizeof(_lib.AuditBox) == 24 and C.sizeof(_lib.AuditPlanOut) == 64 and C.sizeof(_lib.AuditEpisodeOut) == 56


class _Runtime:
    """stands in for HipPredictor: records the calls, answers with arrays of the right shapes"""

    def __init__(self):
        self.plan_calls, self.episode_calls = [], []

    def audit_plan(self, flats, xs, ego_box, exo_margin):
        self.plan_calls.append((flats, xs, ego_box, exo_margin))
        C_, n = (xs[0] if isinstance(xs, list) else xs).shape[0], len(flats)
        Ms = [len(f["parent"]) for f in flats]
        res = {k: np.zeros((C_, n), np.float64 if k in ("tree_min", "tree_mass") else np.int32)
               for k in ("tree_min", "tree_node", "tree_agent", "tree_hits", "tree_first", "tree_mass")}
        res["node_clear"], res["node_agent"] = [np.ones((C_, M)) for M in Ms], [np.ones((C_, M), np.int32) for M in Ms]
        return res

    def audit_episode(self, ego, exo, valid, boxes, ego_box):
        self.episode_calls.append((ego, exo, valid, boxes, ego_box))
        E, S = ego.shape[:2]
        return dict(step_clear=np.tile(np.arange(S, dtype=np.float64) - 2.0, (E, 1)), step_track=np.ones((E, S), np.int32), ego_min=np.full(E, -2.0),
                    ego_step=np.zeros(E, np.int32), ego_track=np.ones(E, np.int32), ego_hits=np.full(E, 2, np.int32), ego_first=np.zeros(E, np.int32))


def test_plan_audit_restated_on_a_solved_tree():
    """the plan audit of the scripted branch3 tree as the C oracle solves it: the restatement's node loop over the host entry pair by pair
    equals the batched evaluation the GPU tests compare with (bit for bit), the restatement on numpy's trig agrees to 1e-9 m with the same
    agents, and the tree has what the audit exists to find: nodes inside a disc"""
    from mind_amd.synth import scripted_scenario_tree
    from oracle import ilqr as oi
    sst = scripted_scenario_tree("branch3", 12)
    flat = oi.flatten(sst["nodes"])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    w = oi.solve(oi.default_cfg(), flat, x0, sst["target_lane"], sst["target_vel"], 0)
    xs = oi.solve(oi.default_cfg(), flat, x0, sst["target_lane"], sst["target_vel"], 1, us_init=w["us"])["xs"].copy()
    xs[7, 1] = np.nan                                              # one state that is not finite
    entry = lambda a, d: _lib.box_clearance(0, [a], [list(d) + [0.0, 0.0]])[0]
    clear, agent = ac.host_plan_nodes(flat, xs, ac.EGO_BOX, 2.5)
    c1, a1 = rs.plan_pairs(flat, xs, ac.EGO_BOX, 2.5, entry)
    assert np.array_equal(clear, c1, equal_nan=True) and np.array_equal(agent, a1)
    c2, a2 = rs.plan_pairs(flat, xs, ac.EGO_BOX, 2.5, rs.disc_pair_restated())
    ok = np.isfinite(clear)
    assert np.isnan(clear[7]) and agent[7] == -1 and ok.sum() == len(clear) - 1
    assert np.abs(clear[ok] - c2[ok]).max() <= 1e-9 and np.array_equal(agent, a2)
    assert np.abs(clear[ok]).min() > 1e-4                          # no hit flag on a last-bit edge
    r = rs.reduce_tree(np.where(ok, clear, 1.0), agent, flat["prob"])
    print(f"branch3: {r[3]} of {len(clear)} nodes inside a disc, min {r[0]:+.3f} m at node {r[1]} (agent {r[2]}), first {r[4]}, mass {r[5]:.4f}")
    assert r[3] > 0 and r[0] < 0 and r[4] >= 0 and 0 < r[5]
    assert np.isnan(rs.reduce_tree(clear, agent, flat["prob"])[0]) and rs.reduce_tree(clear, agent, flat["prob"])[1:5] == (7, -1, -1, -1)


def _scripted(kind, a):
    from mind_amd.planners.mind.trajectory_tree import to_traj_tree
    from mind_amd.synth import scripted_scenario_tree
    from oracle import ilqr as oi
    sst = scripted_scenario_tree(kind, a)
    flat = oi.flatten(sst["nodes"])
    return sst, flat, to_traj_tree


def test_audit_module_checks_shapes_and_calls_the_runtime_once():
    rt = _Runtime()
    sst, flat, to_traj_tree = _scripted("lead", 4)
    M = len(flat["parent"])
    xs = np.arange(M * 6, dtype=np.float64).reshape(M, 6)
    # audit_rollouts: one candidate, several, a bad shape, a bad tree
    r = audit.audit_rollouts(flat, xs, runtime=rt)
    assert len(rt.plan_calls) == 1 and r["node_clear"].shape == (M,) and np.ndim(r["tree_min"]) == 0
    assert rt.plan_calls[0][2] == (4.5, 2.0) and rt.plan_calls[0][3] == 2.5 and rt.plan_calls[0][1].shape == (1, M, 6)
    r = audit.audit_rollouts(flat, np.stack([xs] * 3), ego_box=(5.0, 2.2, 1.4), exo_margin=0.5, runtime=rt)
    assert len(rt.plan_calls) == 2 and r["node_clear"].shape == (3, M) and r["tree_hits"].shape == (3,)
    assert rt.plan_calls[1][2] == (5.0, 2.2, 1.4) and rt.plan_calls[1][3] == 0.5
    with pytest.raises(ValueError, match="xs must be"):
        audit.audit_rollouts(flat, xs[:-1], runtime=rt)
    with pytest.raises(TypeError):
        audit.audit_rollouts(object(), xs, runtime=rt)
    assert len(rt.plan_calls) == 2
    # audit_plan: a trajectory tree of the same flat tree, its states read from keys 0..M-1 (the root, key -1, is x0)
    x0 = np.full(6, -7.0)
    tt = to_traj_tree(flat, x0, xs, np.zeros((M, 2)))

    class Scen:      # (a scenario tree that was flattened already, as the native plan's are)
        _flat = flat
    r = audit.audit_plan([Scen()], [tt], runtime=rt)
    assert len(rt.plan_calls) == 3 and np.array_equal(rt.plan_calls[2][1][0][0], xs) and rt.plan_calls[2][0][0] is flat
    assert len(r["node_clear"]) == 1 and r["node_clear"][0].shape == (M,) and r["tree_min"].shape == (1,)
    with pytest.raises(ValueError, match="scenario trees"):
        audit.audit_plan([Scen(), Scen()], [tt], runtime=rt)
    with pytest.raises(ValueError, match="trajectory nodes"):
        audit.audit_plan([Scen()], [to_traj_tree(dict(flat, parent=flat["parent"][:-1]), x0, xs[:-1], np.zeros((M - 1, 2)))], runtime=rt)
    assert len(rt.plan_calls) == 3

    class Planner:
        class traj_tree_opt:
            class config:
                opt_cfg = {"w_exo_cov_offset": 1.25}
    audit.audit_plan(Scen(), tt, planner=Planner, runtime=rt)
    assert rt.plan_calls[3][3] == 1.25


def test_predictor_methods_check_their_arguments():
    """HipPredictor.audit_plan / audit_episode reject bad shapes before any library call (no context is needed to get that far)"""
    from mind_amd.predictor import HipPredictor
    hp = HipPredictor.__new__(HipPredictor)
    sst, flat, _ = _scripted("lead", 4)
    M = len(flat["parent"])
    with pytest.raises(ValueError, match="xs must be"):
        hp.audit_plan([flat], np.zeros((2, M + 1, 6)), (4.5, 2.0), 2.5)
    with pytest.raises(ValueError, match="exo_margin"):
        hp.audit_plan([flat], np.zeros((2, M, 6)), (4.5, 2.0), -1.0)
    with pytest.raises(ValueError, match="ego_box"):
        hp.audit_plan([flat], np.zeros((2, M, 6)), (4.5, -2.0), 2.5)
    with pytest.raises(ValueError, match="ego_box"):
        hp.audit_plan([flat], np.zeros((2, M, 6)), (4.5, np.nan), 2.5)
    with pytest.raises(ValueError, match="do not match"):
        hp.audit_plan([dict(flat, cov=flat["cov"][:-1])], np.zeros((2, M, 6)), (4.5, 2.0), 2.5)
    S, n = 5, 3
    ok = dict(ego_states=np.zeros((S, 4)), exo=np.zeros((S, n, 5)), valid=np.zeros((S, n), np.uint8), boxes=np.ones((n, 2)), ego_box=(4.5, 2.0))
    for key, bad, msg in (("ego_states", np.zeros((S, 3)), "ego_states"), ("exo", np.zeros((S + 1, n, 5)), "exo must be"),
                          ("valid", np.zeros((S, n + 1), np.uint8), "valid must be"), ("boxes", np.ones((n, 3)), "valid must be"),
                          ("boxes", -np.ones((n, 2)), "boxes must be"), ("ego_box", (1.0,), "ego_box")):
        with pytest.raises(ValueError, match=msg):
            hp.audit_episode(**dict(ok, **{key: bad}))


def test_episode_auditor_records_and_reports_once():
    from types import SimpleNamespace

    class World:
        n_agents, agent_ids = 3, ["AV", "a", "b"]

        def agent_state(self, i, t):
            return np.array([10.0 * i + t, float(i), 1.0, 0.0])

        def object_type(self, i):
            return ("vehicle", "pedestrian", "bus")[i]

        def is_valid(self, i, t):
            return not (i == 2 and t == 0.0)

    class Sim:
        def __init__(self):
            self.world, self.sim_time, self.enabled, self.state, self.n = World(), 0.0, False, np.array([-1.0, -1.0, 0.0, 0.0]), 0

        def step(self):
            self.sim_time += 0.02
            self.n += 1
            self.enabled = self.n >= 3
            return False

    rt, sim = _Runtime(), Sim()
    au = audit.EpisodeAuditor(sim, runtime=rt).run(5)
    assert sim.n == 5 and not rt.episode_calls
    rep = au.report()
    assert len(rt.episode_calls) == 1
    ego, exo, valid, boxes, box = rt.episode_calls[0]
    assert ego.shape == (1, 5, 4) and exo.shape == (5, 3, 5) and valid.shape == (5, 3) and box == (4.5, 2.0)
    assert np.array_equal(rep["times"], ac.sim_times(5)) and rep["enabled"].tolist() == [False, False, False, True, True]
    assert np.array_equal(ego[0, :3, 0], rep["times"][:3]) and np.all(ego[0, 3:, 0] == -1.0)          # the recording, then the simulator's own state
    assert valid[:, 0].tolist() == [0] * 5 and valid[:, 1].tolist() == [1] * 5 and valid[:, 2].tolist() == [0, 1, 1, 1, 1]
    assert np.array_equal(boxes, [[4.5, 2.0], [0.5, 0.75], [7.0, 2.1]]) and exo[1, 2, 0] == 20.0 + rep["times"][1]
    # the split at the take-over: steps 0..2 before (clearances -2, -1, 0), 3..4 after (1, 2)
    b, a = rep["before"], rep["after"]
    assert b["steps"].tolist() == [0, 1, 2] and b["ego_min"] == -2.0 and b["ego_step"] == 0 and b["ego_hits"] == 2 and b["ego_first"] == 0
    assert a["steps"].tolist() == [3, 4] and a["ego_min"] == 1.0 and a["ego_step"] == 3 and a["ego_hits"] == 0 and a["ego_first"] == -1
    assert rep["ego_hits"] == 2 and rep["ego_min"] == -2.0
    with pytest.raises(RuntimeError):
        audit.EpisodeAuditor(Sim(), runtime=rt).report()
