"""Shared by tests/test_lane_host.py and tests/test_gpu_lane.py: seeded lane families, the two lane audits evaluated through the library's
HOST entry (mind_debug_lane_project, all boxes of a case in one call) and reduced by the restatement's rules (tests/lane_geom_restate.py),
and the recorded maps.  Not a test module."""
import functools

import numpy as np

import audit_cases as ac
import lane_geom_restate as lr
from mind_amd import _lib, audit

EGO_BOX = audit.BOXES["VEHICLE"]
COS_FLOW = float(np.cos(audit.DEFAULT_LANE_ANGLE))
BOUND = audit.DEFAULT_LANE_BOUND
BOX_KEYS = lr.KEYS
PLAN_KEYS = tuple("node_" + k for k in BOX_KEYS) + ("node_margin",)
TREE_KEYS = ("tree_min", "tree_node", "tree_lane", "tree_hits", "tree_first", "tree_mass", "tree_progress")
STEP_KEYS = tuple("step_" + k for k in BOX_KEYS) + ("step_margin",)
EGO_KEYS = ("ego_min", "ego_step", "ego_lane", "ego_hits", "ego_first", "ego_progress", "ego_back")
INT_KEYS = ("lane", "edge", "node", "step", "hits", "first")


@functools.lru_cache(maxsize=None)
def demo_lanes(name):
    return audit.Lanes.from_semantic_map(ac.recorded_scene(name)[0].smp)


def wiggle(rng, n, start, heading, step=4.0, turn=0.12):
    """an open polyline of n vertices from ``start``: steps of about ``step`` metres, the heading a random walk of ``turn`` radians a step"""
    ang = heading + np.cumsum(rng.normal(0.0, turn, n - 1))
    d = step * rng.uniform(0.6, 1.4, n - 1)
    return np.concatenate([[start], start + np.cumsum(np.stack([d * np.cos(ang), d * np.sin(ang)], 1), axis=0)])


def synth_lanes(seed, sizes, origin=(0.0, 0.0)):
    """len(sizes) lanes, lane l of sizes[l] vertices: side by side 3.6 m apart about ``origin``, every other one running the other way"""
    rng = np.random.default_rng(seed)
    lanes = []
    for l, n in enumerate(sizes):
        back = l % 2 == 1
        x0 = origin[0] + (4.0 * (n - 1) if back else 0.0)
        lanes.append(wiggle(rng, n, np.array([x0, origin[1] + 3.6 * l]), np.pi if back else 0.0))
    return audit.Lanes.from_polylines(lanes)


def boxes_about(lanes, n, seed, pad=8.0):
    """n boxes (x, y, yaw): every other one near a lane vertex (a few metres off it, the heading within a radian of the lane's or against
    it), the others spread over the lanes' bounding box and ``pad`` metres beyond it at any heading"""
    rng = np.random.default_rng(seed)
    lo, hi = lanes.verts.min(0) - pad, lanes.verts.max(0) + pad
    out = np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.uniform(-3.5, 3.5, n)], 1)
    v = rng.integers(0, len(lanes.verts) - 1, n)
    d = lanes.verts[v + 1] - lanes.verts[v]                     # (across a lane boundary: some direction, as good as any)
    near = np.concatenate([lanes.verts[v] + rng.normal(0.0, 2.5, (n, 2)), (np.arctan2(d[:, 1], d[:, 0]) + rng.normal(0.0, 0.6, n) + np.pi * (rng.uniform(size=n) < 0.2))[:, None]], 1)
    out[::2] = near[::2]
    return out


def nan_rows(rows, cols):
    """the (x, y, yaw) of state rows, NaN where ANY column of the row is not finite (the kernels' rule)"""
    return np.where(np.isfinite(rows).all(1, keepdims=True), rows[:, cols], np.nan)


# ---- the audits through the host entry ------------------------------------------------------------------------------------------------

def host_plan(flats, xs_per_tree, lanes, box=EGO_BOX, cos_flow=COS_FLOW, bound=BOUND):
    """what HipPredictor.audit_lane_plan returns, from the host entry + the restatement's reductions; xs_per_tree: one [C, M_t, 6] per tree"""
    C, n = xs_per_tree[0].shape[0], len(flats)
    out = {k: [] for k in PLAN_KEYS}
    out.update({k: np.zeros((C, n), np.int32 if k.split("_")[1] in INT_KEYS else np.float64) for k in TREE_KEYS})
    for t, (f, xs) in enumerate(zip(flats, xs_per_tree)):
        M = xs.shape[1]
        res = _lib.lane_project(nan_rows(xs.reshape(-1, 6), [0, 1, 3]), box, lanes.verts, lanes.lane_off, cos_flow, bound)
        for k in BOX_KEYS:
            out["node_" + k].append(res[k].reshape(2, C, M))
        out["node_margin"].append(res["margin"].reshape(C, M))
        for c in range(C):
            r = lr.reduce_tree(out["node_margin"][t][c], out["node_lane"][t][1, c], f["prob"])
            r = r + (lr.progress_tree(f["parent"], f["prob"], out["node_lane"][t][0, c], out["node_s"][t][0, c]),)
            for k, v in zip(TREE_KEYS, r):
                out[k][c, t] = v
    return out


def _same(g, w, what):
    assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w, equal_nan=w.dtype == np.float64), (what, g, w)


def same_plan(got, want):
    """bitwise equality of two audit_lane_plan results (NaN == NaN)"""
    for k in PLAN_KEYS:
        assert len(got[k]) == len(want[k]), k
        for t, (g, w) in enumerate(zip(got[k], want[k])):
            _same(g, w, (k, t))
    for k in TREE_KEYS:
        _same(got[k], want[k], k)


def host_episode(egos, lanes, box=EGO_BOX, cos_flow=COS_FLOW, bound=BOUND):
    """what HipPredictor.audit_lane_episode returns, from the host entry + the restatement's reductions; egos [E, S, 4]"""
    E, S = egos.shape[:2]
    res = _lib.lane_project(nan_rows(egos.reshape(-1, 4), [0, 1, 3]), box, lanes.verts, lanes.lane_off, cos_flow, bound)
    out = {"step_" + k: res[k].reshape(2, E, S) for k in BOX_KEYS}
    out["step_margin"] = res["margin"].reshape(E, S)
    out.update({k: np.zeros(E, np.int32 if k.split("_")[1] in INT_KEYS else np.float64) for k in EGO_KEYS})
    for e in range(E):
        r = lr.reduce_ego(out["step_margin"][e], out["step_lane"][1, e]) + lr.progress_ego(out["step_lane"][0, e], out["step_s"][0, e])
        for k, v in zip(EGO_KEYS, r):
            out[k][e] = v
    return out


def same_episode(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        _same(got[k], w, k)
