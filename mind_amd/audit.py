"""Clearance audit of plans and closed-loop episodes: what the planner did to the other road users.

The reference gives every agent a ``BBox`` by object type (agent.py:92-105, common/bbox.py), carries it in each observation and draws it
centred on ``state[:2]`` (visualization.py:69-72), but never tests it against anything; ``evaluate_traj_tree`` (planner.py:180-198) prices
comfort, speed and lane distance and ignores every exo agent.  This module measures outcomes -- it is called from no planning cycle and
changes no choice:

* ``audit_plan(scen_tree, traj_tree)``: signed distance of the ego box at every trajectory node to the discs the solver's exo term prices
  (the predicted mean of the node's step, radius max-sigma + ``w_exo_cov_offset``; trajectory_tree.py:78-118), per node and per tree;
* ``audit_rollouts(flat, xs)``: the same for candidate state sets ``[C, M, 6]`` as ``HipPredictor.ilqr_score`` / ``ilqr_policy_rollouts``
  return them;
* ``EpisodeAuditor(sim)``: box-to-box clearance of the ego actually driven in a ``ClosedLoopSim`` against the replayed tracks, per step.

All numbers come from the device (mind_audit_plan / mind_audit_episode; geometry: mind_amd/csrc/box_geom.h).  Hit convention:
clearance < 0; touching (0.0) is no hit.  The nominal boxes are nominal: every box is an argument.

The ROAD audit says what the ego did to the road, by the same conventions (mind_audit_road_plan / mind_audit_road_episode; geometry:
mind_amd/csrc/road_geom.h): ``Road`` holds the drivable area of a map as rings, ``audit_road_plan`` / ``audit_road_rollouts`` /
``EpisodeRoadAuditor`` mirror the three above with the signed margin of the ego box's corners to the road (negative: off the road).

The TIME-TO-COLLISION audit says how close to a collision the ego drove (mind_audit_ttc; geometry: mind_amd/csrc/ttc_geom.h):
``EpisodeTtcAuditor(sim)`` gives per step the first time at which the ego box and a track's box would overlap if both kept their
velocity -- the reference tests no box against anything (agent.py:92-105, visualization.py:69-72), so the definition is this project's.

The LANE audit says whether the ego drove where it was told to drive (mind_audit_lane_plan / mind_audit_lane_episode; geometry:
mind_amd/csrc/lane_geom.h): ``Lanes`` holds lane centrelines as open polylines, ``audit_lane_plan`` / ``audit_lane_rollouts`` /
``EpisodeLaneAuditor`` give the lateral offset from the nearest centreline, the heading against its direction of travel and the arc length
covered -- lane keeping, driving-direction compliance and progress, the terms of a closed-loop score the other audits leave open."""
import numpy as np

from .planners.mind.utils import _name

# (length, width) by object type: the table of agent.py:92-105 over common/bbox.py
BOXES = {"VEHICLE": (4.5, 2.0), "PEDESTRIAN": (0.5, 0.75), "CYCLIST": (1.5, 0.75), "MOTORCYCLIST": (1.5, 0.75), "BUS": (7.0, 2.1)}
UNKNOWN_BOX = (1.0, 1.0)        # ObjectType.UNKNOWN and every static object
DEFAULT_EXO_MARGIN = 2.5        # opt_cfg["w_exo_cov_offset"] of every planning config (configs/planning/_base.py)


def box_for(object_type):
    """(length, width) of an av2 ObjectType (or a look-alike, or its name)"""
    return BOXES.get(_name(object_type), UNKNOWN_BOX)


def _runtime(runtime):
    if runtime is not None:
        return runtime
    from .runtime import get_runtime
    return get_runtime()


def _margin(exo_margin, planner):
    if exo_margin is not None:
        return float(exo_margin)
    if planner is not None:
        return float(planner.traj_tree_opt.config.opt_cfg["w_exo_cov_offset"])
    return DEFAULT_EXO_MARGIN


def _flat_of(scen_tree):
    from .planners.mind.trajectory_tree import flatten_scenario_tree
    return getattr(scen_tree, "_flat", None) or flatten_scenario_tree(scen_tree)


def _states_of(traj_tree, M):
    """states [M, 6] of the trajectory-tree keys 0..M-1 (the root, key -1, holds x0 and is no trajectory node)"""
    arr = getattr(traj_tree, "_arrays", None)
    xs = np.asarray(arr[0], np.float64)[1:] if arr is not None else np.array([traj_tree.get_node(k).data[0] for k in range(M)], np.float64)
    if xs.shape != (M, 6):
        raise ValueError(f"the trajectory tree holds {list(xs.shape)} states, the scenario tree flattens to {M} trajectory nodes")
    return xs


def _plan_args(who, scen_tree, traj_tree):
    """the arguments of the two plan audits -> (flat cost trees, one [1, M_t, 6] state set per tree)"""
    scen = list(scen_tree) if isinstance(scen_tree, (list, tuple)) else [scen_tree]
    traj = list(traj_tree) if isinstance(traj_tree, (list, tuple)) else [traj_tree]
    if len(scen) != len(traj) or not scen:
        raise ValueError(f"{who}: {len(scen)} scenario trees, {len(traj)} trajectory trees")
    flats = [_flat_of(t) for t in scen]
    return flats, [_states_of(t, len(f["parent"]))[None] for t, f in zip(traj, flats)]


def _plan_result(res):
    """one candidate on n trees: per-tree lists of the node_* arrays [M_t], the tree_* arrays [n_trees]"""
    return {k: [a[0] for a in v] if k.startswith("node_") else v[0] for k, v in res.items()}


def _rollout_args(who, solver_or_flat, xs):
    """the arguments of the two rollout audits -> (flat cost tree, xs [C, M, 6], whether xs was one [M, 6] set)"""
    flat = solver_or_flat if isinstance(solver_or_flat, dict) else getattr(solver_or_flat, "cost_tree", None)
    if not isinstance(flat, dict) or not all(k in flat for k in ("parent", "prob", "mean", "cov")):
        raise TypeError(f"{who}: a flat cost tree (parent, prob, mean, cov) or a TrajectoryTreeOptimizer with a prepared cost tree is needed")
    x = np.asarray(xs, np.float64)
    one = x.ndim == 2
    x = x[None] if one else x
    M = len(flat["parent"])
    if x.ndim != 3 or x.shape[1:] != (M, 6):
        raise ValueError(f"{who}: xs must be [C, {M}, 6] or [{M}, 6], got {list(np.shape(xs))}")
    return flat, x, one


def _rollout_result(res, one):
    """C candidates on one tree: the node_* arrays [C, M], the tree_* arrays [C]; without the C axis for one [M, 6] set"""
    out = {k: v[0] if k.startswith("node_") else v[:, 0] for k, v in res.items()}
    return {k: v[0] for k, v in out.items()} if one else out


def audit_plan(scen_tree, traj_tree, ego_box=BOXES["VEHICLE"], exo_margin=None, runtime=None, planner=None):
    """Audit what ``plan()`` returned (``[[scen_tree], [traj_tree]]`` of MINDPlanner.plan, native_plan or the native loop's
    ``last_result``): ``scen_tree`` / ``traj_tree`` are the two lists (or one tree each).  Tree t's states are read from its trajectory-tree
    keys 0..M-1 and paired with the flattened scenario tree's agents; ONE device call for all trees.  ``exo_margin``: None = the
    ``w_exo_cov_offset`` of ``planner``'s config, 2.5 without a planner.  Returns a dict: per-tree lists node_clear [M_t] / node_agent [M_t]
    and arrays tree_min, tree_node, tree_agent, tree_hits, tree_first, tree_mass [n_trees]."""
    flats, xs = _plan_args("audit_plan", scen_tree, traj_tree)
    return _plan_result(_runtime(runtime).audit_plan(flats, xs, ego_box, _margin(exo_margin, planner)))


def audit_rollouts(solver_or_flat, xs, ego_box=BOXES["VEHICLE"], exo_margin=None, runtime=None):
    """The audit of C candidate state sets ``xs`` [C, M, 6] (or [M, 6]) on ONE cost tree: a flat dict (parent, prob, mean, cov) or a
    ``TrajectoryTreeOptimizer`` (its last prepared cost tree; ``exo_margin`` then defaults to its config's).  Returns node_clear [C, M],
    node_agent [C, M] and tree_min, tree_node, tree_agent, tree_hits, tree_first, tree_mass [C]."""
    flat, x, one = _rollout_args("audit_rollouts", solver_or_flat, xs)
    if exo_margin is None and not isinstance(solver_or_flat, dict) and getattr(solver_or_flat, "config", None) is not None:
        exo_margin = solver_or_flat.config.opt_cfg["w_exo_cov_offset"]
    return _rollout_result(_runtime(runtime).audit_plan([flat], x, ego_box, _margin(exo_margin, None)), one)


def tabulate_exo(world, times):
    """The world's exo rows at ``times``: exo [S, n, 5] = (x, y, heading, vx, vy), valid uint8 [S, n] (the layouts of the native loop's
    tables; row 0, the ego's, stays empty) and boxes [n, 2] from the tracks' object types"""
    n, S = int(world.n_agents), len(times)
    is_valid = getattr(world, "is_valid", None)
    exo, valid = np.zeros((S, n, 5)), np.zeros((S, n), np.uint8)
    for s, t in enumerate(times):
        for i in range(1, n):
            if is_valid is None or is_valid(i, t):
                x, y, v, yaw = (float(q) for q in world.agent_state(i, t))
                exo[s, i] = (x, y, yaw, v * np.cos(yaw), v * np.sin(yaw))
                valid[s, i] = 1
    boxes = np.array([box_for(world.object_type(i)) for i in range(n)], np.float64).reshape(n, 2)
    return exo, valid, boxes


class EpisodeAuditor:
    """Wraps a ClosedLoopSim the way FrameRecorder does: ``step()`` records the ego state in force, the ``enabled`` flag and the time, then
    advances the simulation; ``report()`` tabulates the world's tracks at the recorded times and audits the whole trace in one device call."""

    def __init__(self, sim, ego_box=BOXES["VEHICLE"], runtime=None):
        self.sim, self.ego_box, self.runtime = sim, ego_box, runtime
        self.states, self.enabled, self.times = [], [], []

    def step(self):
        sim = self.sim
        t = sim.sim_time
        self.states.append(np.array(sim.state if sim.enabled else sim.world.agent_state(0, t), dtype=np.float64))
        self.enabled.append(bool(sim.enabled))
        self.times.append(t)
        return sim.step()

    def run(self, n_steps):
        for _ in range(n_steps):
            self.step()
        return self

    def report(self):
        """-> dict: ego_min, ego_step, ego_track, ego_hits, ego_first of the whole trace; times [S], enabled [S], step_clear [S],
        step_track [S]; ``before`` / ``after``: the same summary and per-step arrays of the steps before and from the take-over (None
        when there is no such step); steps are indices into the recorded trace"""
        S = len(self.times)
        if S == 0:
            raise RuntimeError("EpisodeAuditor.report: no step was recorded")
        ego = np.stack(self.states)
        exo, valid, boxes = tabulate_exo(self.sim.world, self.times)
        res = _runtime(self.runtime).audit_episode(ego[None], exo, valid, boxes, self.ego_box)
        per = {k: res[k][0] for k in ("step_clear", "step_track")}
        en = np.array(self.enabled, bool)
        out = dict(times=np.array(self.times), enabled=en, **per,
                   **{k: (float if k == "ego_min" else int)(res[k][0]) for k in ("ego_min", "ego_step", "ego_track", "ego_hits", "ego_first")})
        out["before"], out["after"] = (_part(per, i, "step_clear", "track", nan_step=False) for i in (np.flatnonzero(~en), np.flatnonzero(en)))
        return out


def _part(per, idx, value, tag, nan_step, bar=0.0):
    """summary of the steps ``idx`` of a trace whose per-step arrays are ``per``, by the rules of the whole-trace summary over
    per[value] with the tag per["step_" + tag] (the lowest step wins ties); a step is a hit when its value is below ``bar`` (0.0 for the
    clearance and road audits, the bound for the time to collision).  ``nan_step`` (the road audit): a NaN step reports NaN, that
    step, -1, -1, -1; without it (the clearance audit) the first minimum is numpy's argmin"""
    if len(idx) == 0:
        return None
    m = per[value][idx]
    out = dict(steps=idx, **{k: v[idx] for k, v in per.items()})
    bad = np.flatnonzero(np.isnan(m)) if nan_step else ()
    if len(bad):
        out.update({"ego_min": float("nan"), "ego_step": int(idx[bad[0]]), "ego_" + tag: -1, "ego_hits": -1, "ego_first": -1})
        return out
    hit, k = np.flatnonzero(m < bar), int(np.argmin(m))               # (first minimum)
    out.update({"ego_min": float(m[k]), "ego_step": int(idx[k]), "ego_" + tag: int(per["step_" + tag][idx[k]]), "ego_hits": int(len(hit)),
                "ego_first": int(idx[hit[0]]) if len(hit) else -1})
    return out


# ---- the time-to-collision audit ------------------------------------------------------------------------------------------------------

DEFAULT_TTC_HORIZON = 3.0       # seconds: a time to collision above it counts as none
DEFAULT_TTC_BOUND = 0.95        # seconds: a step with a time to collision below it is a hit


class EpisodeTtcAuditor:
    """Wraps a ClosedLoopSim exactly as EpisodeAuditor does; ``report()`` gives, per recorded step, the time to collision of the ego box
    with the nearest-in-time track's box when both keep the velocity they have at that step (mind_audit_ttc; geometry:
    mind_amd/csrc/ttc_geom.h), in one device call.  ``horizon`` and ``bound`` (seconds) are defaults only: the first is the look-ahead
    beyond which a collision counts as none, the second the bar below which a step is a hit."""

    def __init__(self, sim, ego_box=BOXES["VEHICLE"], horizon=DEFAULT_TTC_HORIZON, bound=DEFAULT_TTC_BOUND, runtime=None):
        self.sim, self.ego_box, self.horizon, self.bound, self.runtime = sim, ego_box, float(horizon), float(bound), runtime
        self.states, self.enabled, self.times = [], [], []

    step = EpisodeAuditor.step
    run = EpisodeAuditor.run

    def report(self):
        """-> dict: ego_min, ego_step, ego_track, ego_hits (steps with ttc < bound), ego_first of the whole trace; times [S], enabled [S],
        step_ttc [S] (seconds; 0.0: overlapping now, +inf: none within the horizon), step_track [S] (-1 for +inf); ``before`` / ``after``:
        the same summary and per-step arrays of the steps before and from the take-over (None when there is no such step); steps are
        indices into the recorded trace"""
        if len(self.times) == 0:
            raise RuntimeError("EpisodeTtcAuditor.report: no step was recorded")
        ego = np.stack(self.states)
        exo, valid, boxes = tabulate_exo(self.sim.world, self.times)
        res = _runtime(self.runtime).audit_ttc(ego[None], exo, valid, boxes, self.ego_box, self.horizon, self.bound)
        per = {k: res[k][0] for k in ("step_ttc", "step_track")}
        en = np.array(self.enabled, bool)
        out = dict(times=np.array(self.times), enabled=en, **per,
                   **{k: (float if k == "ego_min" else int)(res[k][0]) for k in ("ego_min", "ego_step", "ego_track", "ego_hits", "ego_first")})
        out["before"], out["after"] = (_part(per, i, "step_ttc", "track", nan_step=False, bar=self.bound) for i in (np.flatnonzero(~en), np.flatnonzero(en)))
        return out


# ---- the road audit -----------------------------------------------------------------------------------------------------------------

class Road:
    """The drivable area of a map as the road audit takes it: ``verts`` float64 [V, 2] (world coordinates) and ``poly_off`` int32 [P + 1];
    ring r = verts[poly_off[r]:poly_off[r + 1]], implicitly closed, at least three vertices, no holes."""

    def __init__(self, verts, poly_off):
        self.verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 2)
        self.poly_off = np.ascontiguousarray(poly_off, np.int32).ravel()
        n = np.diff(self.poly_off)
        if len(n) < 1 or self.poly_off[0] != 0 or self.poly_off[-1] != len(self.verts) or np.any(n < 3):
            raise ValueError(f"Road: poly_off {self.poly_off.tolist()[:8]} must start at 0, end at V = {len(self.verts)} and give every ring three vertices")
        if not np.all(np.isfinite(self.verts)):
            raise ValueError("Road: a vertex is not finite")

    @property
    def n_rings(self):
        return len(self.poly_off) - 1

    def ring(self, r):
        return self.verts[self.poly_off[r]:self.poly_off[r + 1]]

    @classmethod
    def from_polygons(cls, polygons):
        """rings as [n, 2] (or [n, 3]: z is dropped) arrays; a closing vertex equal to the first is dropped"""
        rings = []
        for p in polygons:
            a = np.asarray(p, np.float64)
            if a.ndim != 2 or a.shape[1] not in (2, 3):
                raise ValueError(f"Road.from_polygons: a ring must be [n, 2], got {list(a.shape)}")
            a = a[:, :2]
            if len(a) > 1 and np.array_equal(a[0], a[-1]):
                a = a[:-1]
            rings.append(a)
        if not rings:
            raise ValueError("Road.from_polygons: no ring")
        return cls(np.concatenate(rings), np.concatenate([[0], np.cumsum([len(r) for r in rings])]))

    @classmethod
    def from_static_map(cls, static_map):
        """the ``drivable_areas`` of an ``av2_lite.StaticMap`` read from a map JSON"""
        areas = getattr(static_map, "drivable_areas", None)
        if areas is None:
            raise ValueError("this map holds no drivable areas: it was loaded from a compact scene file (or built from arrays), which keeps the lane "
                             "segments only.  Load the map JSON (log_map_archive_<seq_id>.json) with av2_lite.StaticMap.from_json or "
                             "Road.from_map_json")
        if not areas:
            raise ValueError("the map JSON holds no drivable_areas polygon")
        return cls.from_polygons(areas)

    @classmethod
    def from_map_json(cls, path):
        from . import av2_lite
        return cls.from_static_map(av2_lite.StaticMap.from_json(path))


def _road(road):
    if not isinstance(road, Road):
        road = Road.from_static_map(road) if hasattr(road, "vector_lane_segments") else Road.from_polygons(road)
    return road


def audit_road_plan(scen_tree, traj_tree, road, ego_box=BOXES["VEHICLE"], runtime=None):
    """The road audit of what ``plan()`` returned, the lists ``audit_plan`` takes; ``road``: a ``Road`` (or a StaticMap read from a map
    JSON, or a list of rings).  ONE device call for all trees.  Returns a dict: per-tree lists node_margin / node_corner / node_ring /
    node_edge [M_t] and arrays tree_min, tree_node, tree_corner, tree_hits, tree_first, tree_mass [n_trees]."""
    road = _road(road)
    flats, xs = _plan_args("audit_road_plan", scen_tree, traj_tree)
    return _plan_result(_runtime(runtime).audit_road_plan(flats, xs, road.verts, road.poly_off, ego_box))


def audit_road_rollouts(solver_or_flat, xs, road, ego_box=BOXES["VEHICLE"], runtime=None):
    """The road audit of C candidate state sets ``xs`` [C, M, 6] (or [M, 6]) on ONE cost tree: a flat dict (parent, prob, mean, cov) or a
    ``TrajectoryTreeOptimizer`` (its last prepared cost tree).  Returns node_margin, node_corner, node_ring, node_edge [C, M] and tree_min,
    tree_node, tree_corner, tree_hits, tree_first, tree_mass [C]."""
    road = _road(road)
    flat, x, one = _rollout_args("audit_road_rollouts", solver_or_flat, xs)
    return _rollout_result(_runtime(runtime).audit_road_plan([flat], x, road.verts, road.poly_off, ego_box), one)


class EpisodeRoadAuditor:
    """Wraps a ClosedLoopSim exactly as EpisodeAuditor does; ``report()`` audits the recorded ego trace against ``road`` in one device call."""

    def __init__(self, sim, road, ego_box=BOXES["VEHICLE"], runtime=None):
        self.sim, self.road, self.ego_box, self.runtime = sim, _road(road), ego_box, runtime
        self.states, self.enabled, self.times = [], [], []

    step = EpisodeAuditor.step
    run = EpisodeAuditor.run

    def report(self):
        """-> dict: ego_min, ego_step, ego_corner, ego_hits, ego_first of the whole trace; times [S], enabled [S], step_margin, step_corner,
        step_ring, step_edge [S]; ``before`` / ``after``: the same summary and per-step arrays of the steps before and from the take-over
        (None when there is no such step); steps are indices into the recorded trace"""
        if len(self.times) == 0:
            raise RuntimeError("EpisodeRoadAuditor.report: no step was recorded")
        ego = np.stack(self.states)
        res = _runtime(self.runtime).audit_road_episode(ego[None], self.road.verts, self.road.poly_off, self.ego_box)
        per = {k: res[k][0] for k in ("step_margin", "step_corner", "step_ring", "step_edge")}
        en = np.array(self.enabled, bool)
        out = dict(times=np.array(self.times), enabled=en, **per,
                   **{k: (float if k == "ego_min" else int)(res[k][0]) for k in ("ego_min", "ego_step", "ego_corner", "ego_hits", "ego_first")})
        out["before"], out["after"] = (_part(per, i, "step_margin", "corner", nan_step=True) for i in (np.flatnonzero(~en), np.flatnonzero(en)))
        return out


# ---- the lane audit -----------------------------------------------------------------------------------------------------------------

DEFAULT_LANE_ANGLE = np.pi / 4.0    # radians: the angle threshold of scene_io.get_closest_semantic_lane
DEFAULT_LANE_BOUND = 5.0            # metres: scene_io.ON_LANE_THRES


class Lanes:
    """Lane centrelines as the lane audit takes them: ``verts`` float64 [V, 2] (world coordinates) and ``lane_off`` int32 [P + 1]; lane l =
    verts[lane_off[l]:lane_off[l + 1]], an open polyline of at least two vertices in the direction of travel."""

    def __init__(self, verts, lane_off):
        self.verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 2)
        self.lane_off = np.ascontiguousarray(lane_off, np.int32).ravel()
        n = np.diff(self.lane_off)
        if len(n) < 1 or self.lane_off[0] != 0 or self.lane_off[-1] != len(self.verts) or np.any(n < 2):
            raise ValueError(f"Lanes: lane_off {self.lane_off.tolist()[:8]} must start at 0, end at V = {len(self.verts)} and give every lane two vertices")
        if not np.all(np.isfinite(self.verts)):
            raise ValueError("Lanes: a vertex is not finite")

    @property
    def n_lanes(self):
        return len(self.lane_off) - 1

    def lane(self, l):
        return self.verts[self.lane_off[l]:self.lane_off[l + 1]]

    @classmethod
    def from_polylines(cls, polylines):
        """lanes as [n, 2] (or [n, 3]: z is dropped) arrays, in the direction of travel"""
        lanes = []
        for p in polylines:
            a = np.asarray(p, np.float64)
            if a.ndim != 2 or a.shape[1] not in (2, 3):
                raise ValueError(f"Lanes.from_polylines: a lane must be [n, 2], got {list(a.shape)}")
            lanes.append(a[:, :2])
        if not lanes:
            raise ValueError("Lanes.from_polylines: no lane")
        return cls(np.concatenate(lanes), np.concatenate([[0], np.cumsum([len(l) for l in lanes])]))

    @classmethod
    def from_semantic_map(cls, smp):
        """the ``semantic_lanes`` of a ``scene_io.SemanticMap`` (or of a planner's local map), in id order"""
        lanes = getattr(smp, "semantic_lanes", None)
        if not lanes:
            raise ValueError("this map holds no semantic lanes")
        return cls.from_polylines([lanes[k] for k in sorted(lanes)])

    @classmethod
    def from_target_lane(cls, polyline):
        """one lane: ``ReplayWorld.target_lane`` or the planner's own target lane"""
        return cls.from_polylines([polyline])


def _lanes(lanes):
    if not isinstance(lanes, Lanes):
        lanes = Lanes.from_semantic_map(lanes) if hasattr(lanes, "semantic_lanes") else Lanes.from_polylines(lanes)
    return lanes


def _cos_flow(angle):
    angle = float(angle)
    if not 0.0 <= angle <= np.pi:
        raise ValueError(f"angle must lie in [0, pi], got {angle!r}")
    return float(np.cos(angle))


def _heading_err(res, per):
    """the heading error arctan2(across, along) beside the arrays of a lane audit's result (NaN where there is no segment)"""
    with np.errstate(invalid="ignore"):
        add = lambda ac, al: np.arctan2(ac, al)
        a, b = res[per + "_across"], res[per + "_along"]
        res[per + "_heading_err"] = [add(x, y) for x, y in zip(a, b)] if isinstance(a, list) else add(a, b)
    return res


def audit_lane_plan(scen_tree, traj_tree, lanes, ego_box=BOXES["VEHICLE"], angle=DEFAULT_LANE_ANGLE, bound=DEFAULT_LANE_BOUND, form=0, runtime=None):
    """The lane audit of what ``plan()`` returned, the lists ``audit_plan`` takes; ``lanes``: a ``Lanes`` (or a SemanticMap, or a list of
    polylines); a segment goes the ego's way when the heading is within ``angle`` of it, a node further than ``bound`` from every such
    segment is a hit.  ONE device call for all trees.  Returns a dict: per-tree lists node_lat, node_s, node_along, node_across,
    node_heading_err, node_lane, node_edge [2, M_t] (0 = any segment, 1 = with the flow), node_margin [M_t], and arrays tree_min, tree_node,
    tree_lane, tree_hits, tree_first, tree_mass, tree_progress [n_trees]."""
    lanes = _lanes(lanes)
    flats, xs = _plan_args("audit_lane_plan", scen_tree, traj_tree)
    res = _runtime(runtime).audit_lane_plan(flats, xs, lanes.verts, lanes.lane_off, ego_box, _cos_flow(angle), bound, form)
    return _heading_err({k: [a[..., 0, :] for a in v] if k.startswith("node_") else v[0] for k, v in res.items()}, "node")


def audit_lane_rollouts(solver_or_flat, xs, lanes, ego_box=BOXES["VEHICLE"], angle=DEFAULT_LANE_ANGLE, bound=DEFAULT_LANE_BOUND, form=0, runtime=None):
    """The lane audit of C candidate state sets ``xs`` [C, M, 6] (or [M, 6]) on ONE cost tree: a flat dict (parent, prob, mean, cov) or a
    ``TrajectoryTreeOptimizer`` (its last prepared cost tree).  Returns node_lat, node_s, node_along, node_across, node_heading_err,
    node_lane, node_edge [2, C, M], node_margin [C, M] and tree_min, tree_node, tree_lane, tree_hits, tree_first, tree_mass,
    tree_progress [C] (without the C axis for one [M, 6] set)."""
    lanes = _lanes(lanes)
    flat, x, one = _rollout_args("audit_lane_rollouts", solver_or_flat, xs)
    res = _runtime(runtime).audit_lane_plan([flat], x, lanes.verts, lanes.lane_off, ego_box, _cos_flow(angle), bound, form)
    out = {k: v[0] if k.startswith("node_") else v[:, 0] for k, v in res.items()}
    if one:
        out = {k: v[..., 0, :] if k.startswith("node_") else v[0] for k, v in out.items()}
    return _heading_err(out, "node")


def lane_progress(lane_any, s_any):
    """the episode's progress rule in numpy (k_lane_progress): sequentially from 0.0 over the steps k >= 1 whose lane equals the step
    before's and is >= 0, d = s[k] - s[k - 1]: progress += d, back += d when d < 0 -> (progress, back)"""
    prog, back = np.float64(0.0), np.float64(0.0)
    for k in range(1, len(lane_any)):
        if lane_any[k] < 0 or lane_any[k] != lane_any[k - 1]:
            continue
        d = np.float64(s_any[k]) - np.float64(s_any[k - 1])
        prog = prog + d
        if d < 0.0:
            back = back + d
    return float(prog), float(back)


class EpisodeLaneAuditor:
    """Wraps a ClosedLoopSim exactly as EpisodeAuditor does; ``report()`` audits the recorded ego trace against ``lanes`` in one device call:
    how far from a lane centreline the ego got, whether it pointed along the traffic flow, how much arc length it covered.  ``angle``
    (radians) and ``bound`` (metres) are defaults only, the project's own lane matching in scene_io."""

    def __init__(self, sim, lanes, angle=DEFAULT_LANE_ANGLE, bound=DEFAULT_LANE_BOUND, ego_box=BOXES["VEHICLE"], form=0, runtime=None):
        self.sim, self.lanes, self.ego_box, self.form, self.runtime = sim, _lanes(lanes), ego_box, form, runtime
        self.angle, self.bound = float(angle), float(bound)
        self.states, self.enabled, self.times = [], [], []

    step = EpisodeAuditor.step
    run = EpisodeAuditor.run

    def report(self):
        """-> dict: ego_min, ego_step, ego_lane, ego_hits, ego_first, ego_progress, ego_back of the whole trace; times [S], enabled [S];
        per step, of the nearest segment that goes the ego's way: step_lat, step_s, step_along, step_across, step_heading_err, step_lane,
        step_edge [S], of the nearest segment of all the same names ending in ``_any``, and step_margin [S] = bound - |step_lat|;
        ``before`` / ``after``: the same summary and per-step arrays of the steps before and from the take-over (None when there is no such
        step), the progress of a part by the same rule over its steps; steps are indices into the recorded trace"""
        if len(self.times) == 0:
            raise RuntimeError("EpisodeLaneAuditor.report: no step was recorded")
        ego = np.stack(self.states)
        res = _heading_err(_runtime(self.runtime).audit_lane_episode(ego[None], self.lanes.verts, self.lanes.lane_off, self.ego_box, _cos_flow(self.angle),
                                                                     self.bound, self.form), "step")
        per = {"step_margin": res["step_margin"][0]}
        for k in ("lat", "s", "along", "across", "heading_err", "lane", "edge"):
            per["step_" + k], per["step_" + k + "_any"] = res["step_" + k][1, 0], res["step_" + k][0, 0]
        en = np.array(self.enabled, bool)
        out = dict(times=np.array(self.times), enabled=en, **per,
                   **{k: (int if res[k].dtype == np.int32 else float)(res[k][0]) for k in ("ego_min", "ego_step", "ego_lane", "ego_hits", "ego_first", "ego_progress",
                                                                                          "ego_back")})
        parts = []
        for i in (np.flatnonzero(~en), np.flatnonzero(en)):
            p = _part(per, i, "step_margin", "lane", nan_step=True, bar=0.0)
            if p is not None:
                p["ego_progress"], p["ego_back"] = lane_progress(per["step_lane_any"][i], per["step_s_any"][i])
            parts.append(p)
        out["before"], out["after"] = parts
        return out
