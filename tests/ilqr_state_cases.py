"""Start states, headings and lanes that take the tree-iLQR's dynamics, its trigonometry (mind_trig.h) and its line search / regulariser to
the places the scripted trees never visit: every quadrant of the heading and the thresholds of the argument reduction, standstill and
reversing, states on and beyond the bounds at the root, degenerate lanes.  The cases use the dict format of tests/ilqr_cost_cases.py
(family, name, cfg, flat, x0, lane, tv, M, queries, solve) and its scene builder; all share ONE base scene -- the 35-node tree of
``ilqr_cost_cases.branching()``, 6 agents, the 0.4 m x 256 x 256 grid -- so a case costs milliseconds.  No GPU, no test in here:
tests/test_ilqr_state_cases_host.py proves on the oracle alone what each family reaches and which cases are well enough conditioned for
solve-level assertions, tests/test_gpu_ilqr_state_edges.py runs the kernels on them.

``solve`` is True where the oracle is a valid witness for a solve (the conditioning rule of the host test); ``cfg.max_iter`` is the largest
of 6, 4, 3, 2 at which the case meets that rule (``MAX_ITER``); a case that meets it at none is evaluation-only and listed in
``ILL_CONDITIONED`` with the measured movement.

Queries at which the oracle itself returns NaN would be named in ``NAN_QUERIES`` (family -> case name -> query indices); there are none."""
import numpy as np

import ilqr_cost_cases as cc

NAN_QUERIES = {}
PI = np.pi

# the largest max_iter of (6, 4, 3, 2) at which a case meets the conditioning rule, where that is not 6 (found once on the oracle;
# tests/test_ilqr_state_cases_host.py checks the rule at the recorded value and that the next larger one fails it)
MAX_ITER = {("limits", "a_under"): 2, ("limits", "d_over"): 2, ("limits", "a_under_d_under"): 3, ("limits", "a_under_z"): 2, ("lanes", "behind"): 3}

# evaluation-only cases: (family, name) -> (trace rows kept, movement of xs relative to max(1, |xs|max), relative movement of J) under
# x0[2:] *= 1 +- 1e-13 and the C library's sin / cos / tan, measured at max_iter = 6 and at max_iter = 2; the rule asks for kept rows,
# 1e-10 and 1e-12.  A start exactly ON a bound switches that bound's term on or off under the perturbation; v = 8.5 and 9.5 put the whole
# cost into 50 (v - 8)^2, whose relative slope alone moves J by more than 1e-12; the lane 200 m away has costs of 6e5 and steps of metres;
# a and delta beyond their upper bounds together are stiff in the plain fit from zero controls.
ILL_CONDITIONED = {("speed", "v_on_ub"): ((False, 3.3e-03, 1.1e-04), (True, 3.3e-03, 6.9e-02)),
                   ("speed", "v_over"): ((False, 9.4e+00, 1.2e+04), (False, 8.1e-01, 1.4e+00)),
                   ("speed", "v_over_coast"): ((True, 6.0e-14, 2.2e-12), (True, 6.0e-14, 2.2e-12)),
                   ("limits", "a_ub"): ((False, 3.0e-03, 2.9e-04), (False, 3.4e-02, 4.7e+00)),
                   ("limits", "a_lb"): ((False, 5.8e-01, 2.4e-01), (False, 1.3e+00, 3.9e+00)),
                   ("limits", "d_ub"): ((False, 1.1e+01, 1.0e+00), (False, 2.0e-01, 2.5e+00)),
                   ("limits", "d_lb"): ((False, 1.4e-01, 1.4e-01), (False, 2.5e-01, 2.2e+00)),
                   ("limits", "a_ub_d_ub"): ((False, 6.5e-01, 4.0e-01), (False, 5.3e-01, 6.7e-01)),
                   ("limits", "a_over_d_over"): ((True, 1.5e-08, 1.5e-10), (True, 2.1e-10, 1.7e-12)),
                   ("lanes", "outside"): ((False, 1.0e+00, 1.0e+00), (True, 8.0e-11, 1.0e-12))}


# ---- the base scene ----------------------------------------------------------------------------------------------------------------------
_base = {}


def base():
    """cfg, flat, lane of the base scene about ``cc.X0`` (lane: a sine along +x, 0.4 m beside the start)"""
    if not _base:
        rng = np.random.default_rng(7006)
        cfg = cc.cfg_for()
        parent, prob = cc.branching()
        flat, lane = cc._scene(rng, cfg, parent, prob, cc.X0, 6, (30.0, 24.0), sigma=(0.31, 0.8), lane_dy=0.4, drift=0.5)
        _base.update(cfg=cfg, flat=flat, lane=lane)
    return _base


def rigid(flat, lane, x0, phi):
    """the scene turned by phi about the start position: the lane in float64, the agents in float64 and then cast to float32, x0[3] += phi"""
    c, s = np.cos(phi), np.sin(phi)
    R = np.array([[c, -s], [s, c]])
    f = dict(flat)
    f["mean"] = np.ascontiguousarray((flat["mean"].astype(np.float64) - x0[:2]) @ R.T + x0[:2], np.float32)
    x = np.array(x0, np.float64)
    x[3] += phi
    return f, (np.asarray(lane, np.float64) - x0[:2]) @ R.T + x0[:2], x


def edge_queries(cfg, x0, M, seed):
    """states on and one ulp either side of every finite bound (``cc.bound_states``), headings k pi / 4 and one ulp either side of it for
    k = -8 .. 8 (the thresholds of the argument reduction and of its quadrant choice), v = +0 and -0 -> (node [Q], x [Q, 6], u [Q, 2])"""
    xs = [cc.bound_states(cfg, x0)]
    for k in range(-8, 9):
        t = k * (PI / 4)
        for v in (t, np.nextafter(t, -np.inf), np.nextafter(t, np.inf)):
            x = np.array(x0, np.float64)
            x[3] = v
            xs.append(x[None])
    for v in (0.0, -0.0):
        x = np.array(x0, np.float64)
        x[2] = v
        xs.append(x[None])
    xs = np.concatenate(xs)
    rng = np.random.default_rng(seed)
    return (np.arange(len(xs)) % M).astype(np.int32), xs, rng.normal(size=(len(xs), 2))


def _mk(family, name, x0=None, lane=None, tv=4.0, phi=None):
    b = base()
    x0 = np.array(cc.X0 if x0 is None else x0, np.float64)
    flat, lane = b["flat"], b["lane"] if lane is None else lane
    if phi is not None:
        flat, lane, x0 = rigid(flat, lane, x0, phi)
    key = (family, name)
    cfg = cc.copy_cfg(b["cfg"], max_iter=MAX_ITER.get(key, 6))
    M = len(flat["parent"])
    c = cc._case(family, name, cfg, flat, x0, np.ascontiguousarray(lane), tv, queries=edge_queries(cfg, x0, M, 11), solve=key not in ILL_CONDITIONED)
    return c


def _x(v=None, th=None, a=None, d=None):
    x = cc.X0.copy()
    for k, val in ((2, v), (3, th), (4, a), (5, d)):
        if val is not None:
            x[k] = val
    return x


# ---- families ----------------------------------------------------------------------------------------------------------------------------
# the turn that puts two branches of the base case's full fit on either side of pi / 4 at one tree level (found on the oracle's iterates;
# test_heading_reaches_every_quadrant_and_a_mixed_level checks it)
PHI_MIXED = 0.669261

HEADING_TV = 7.0
HEADINGS = [("base", 0.0), ("below_pi4", PI / 4 - 0.04 - 1.5e-3), ("above_pi4", PI / 4 - 0.04 + 1e-3), ("rot0.755", 0.755), ("pi2", PI / 2),
            ("below_3pi4", 3 * PI / 4 - 0.04 - 1.5e-3), ("above_3pi4", 3 * PI / 4 - 0.04 + 1e-3), ("rot3.0", 3.0), ("pi_minus", PI - 0.04),
            ("neg_pi_plus", -PI + 0.04), ("neg_pi_minus", -PI - 0.04), ("neg_pi2", -PI / 2), ("two_pi_plus", 2 * PI + 0.5), ("near_bound", -9.7),
            ("mixed", PHI_MIXED)]


def straight_lane():
    """the base lane's x stations on the line y = x0.y + 0.4: the squared distance to it is a quadratic, which the field's finite differences
    reproduce exactly, so the lane-only cost of a turned copy does not depend on how the turn lies to the grid"""
    L = base()["lane"].copy()
    L[:, 1] = cc.X0[1] + 0.4
    return L


def heading():
    """the whole base scene moved rigidly: every quadrant, x0's heading 1.5e-3 below and 1e-3 above pi / 4 and 3 pi / 4, a turn of exactly pi / 2,
    starts at +-pi -+ 0.04 and at -pi whose iterates cross +-pi, one |theta| > 2 pi, one near the heading bound of -10, and ``mixed``: a turn
    after which nodes of one tree level lie on both sides of pi / 4, so one wave of the state chain holds k = 0 and k != 0 lanes"""
    return [_mk("heading", name, lane=None if name == "mixed" else straight_lane(), tv=HEADING_TV, phi=phi) for name, phi in HEADINGS]


def speed():
    """standstill with and without a target speed (``on_lane``: the lane runs through the start, so the first pass gains less than 1e-6 of
    J and the lane-only fit stops after one iteration, at step index 6), reversing, v just below, on and above the upper bound of 8, a target speed above it"""
    return [_mk("speed", "v0_tv4", _x(v=0.0, a=0.0, d=0.0), tv=4.0), _mk("speed", "v0_tv0", _x(v=0.0, a=0.0, d=0.0), tv=0.0),
            _mk("speed", "v0_tv0_on_lane", _x(v=0.0, a=0.0, d=0.0), lane=base()["lane"] - np.array([0.0, 0.4]), tv=0.0),
            _mk("speed", "v_neg", _x(v=-1.0), tv=4.0), _mk("speed", "v_below_ub", _x(v=7.9, a=0.0), tv=4.0),
            _mk("speed", "v_on_ub", _x(v=8.0, a=0.0), tv=4.0), _mk("speed", "v_over", _x(v=9.5, a=4.0), tv=4.0),
            _mk("speed", "v_over_coast", _x(v=8.5, a=0.0), tv=4.0), _mk("speed", "tv_over", _x(), tv=9.0)]


def limits():
    """acceleration and steering angle on and beyond each bound at the start (a in [-6, 4], weight 50; delta in [-0.2, 0.2], weight 500),
    alone and together; the other of the two is the scripted tree's initial control (0.1, 0.01) or, in the ``_z`` cases, zero"""
    out = []
    for name, a, d in (("a_ub", 4.0, None), ("a_over", 4.5, None), ("a_lb", -6.0, None), ("a_under", -6.5, None), ("d_ub", None, 0.2),
                       ("d_over", None, 0.25), ("d_lb", None, -0.2), ("d_under", None, -0.3), ("a_ub_d_ub", 4.0, 0.2), ("a_under_d_under", -6.5, -0.3),
                       ("a_over_d_over", 4.5, 0.25)):
        out.append(_mk("limits", name, _x(a=a, d=d)))
    for name, a, d in (("a_over_z", 4.5, 0.0), ("a_under_z", -6.5, 0.0), ("d_over_z", 0.0, 0.25), ("d_under_z", 0.0, -0.3)):
        out.append(_mk("limits", name, _x(a=a, d=d)))
    return out


def lanes():
    """a two-point lane, the lane reversed, a lane that ends behind the ego, a lane wholly outside the 102 m field, a lane with one repeated
    point at its start, in its middle and at its end, and a lane with a segment of 1e-9 m.

    A repeated point is a zero-length segment: t = 0 / 0 is NaN and so is the segment's distance.  ``k_lane_field`` and the oracle
    (oracle/ilqr_ref.c lane_dist_field) both DROP that segment -- ``d = dj < d ? dj : d`` keeps d when dj is NaN -- and the field is the one
    of the lane without the repeat.  The reference's ``gen_dist_field`` (planners/ilqr/utils.py with common/geometry.py
    get_point_line_distance) folds with ``np.minimum``, which propagates the NaN: its whole field is NaN for such a lane.  The GPU test
    holds the device to the oracle; DESIGN.md lists the difference to the reference.  (The plan's tree pricing, ``mind_eval_traj_trees``,
    restates numpy's ``min`` and returns NaN: tests/test_eval_native.py.)"""
    L = base()["lane"]
    x0 = cc.X0
    mid = int(np.argmin(np.abs(L[:, 0] - (x0[0] + 8.0))))
    behind = L[L[:, 0] < x0[0] - 1.0]
    tiny = np.insert(L, mid + 1, L[mid] + np.array([1e-9, 0.0]), axis=0)
    assert len(behind) >= 3
    return [_mk("lanes", "P2", lane=L[[0, -1]]), _mk("lanes", "reversed", lane=L[::-1].copy()), _mk("lanes", "behind", lane=behind),
            _mk("lanes", "outside", lane=L + np.array([0.0, 200.0])), _mk("lanes", "dup_start", lane=np.insert(L, 0, L[0], axis=0)),
            _mk("lanes", "dup_mid", lane=np.insert(L, mid, L[mid], axis=0)), _mk("lanes", "dup_end", lane=np.insert(L, len(L), L[-1], axis=0)),
            _mk("lanes", "seg_1e-9", lane=tiny)]


FAMILIES = dict(heading=heading, speed=speed, limits=limits, lanes=lanes)
_built = {}


def family(name):
    if name not in _built:
        _built[name] = FAMILIES[name]()
    return _built[name]


def all_cases():
    return [c for f in FAMILIES for c in family(f)]


def case_ids():
    return [(c["family"], c["name"]) for c in all_cases()]


def solve_ids():
    return [(c["family"], c["name"]) for c in all_cases() if c["solve"]]


def get(fam, name):
    return next(c for c in family(fam) if c["name"] == name)


# the oracle's results and the evaluation points are those of the cost cases, computed once per case: cc.oracle_of(c), cc.eval_points(c)
oracle_of = cc.oracle_of
eval_points = cc.eval_points
