"""Shared by tests/test_road_host.py and tests/test_gpu_road.py: roads, the two road audits evaluated through the library's HOST entry
(mind_debug_road_margin, all boxes of a case in one call) and reduced by the restatement's rules (tests/road_geom_restate.py), an
independent vectorised witness, and the recorded maps.  Not a test module."""
import functools
import os

import numpy as np

import road_geom_restate as rr
from mind_amd import _lib, audit, scene_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EGO_BOX = audit.BOXES["VEHICLE"]
RECT = [(-20.0, -4.0), (20.0, -4.0), (20.0, 4.0), (-20.0, 4.0)]           # the 40 x 8 m rectangle road
PLAN_KEYS = ("node_margin", "node_corner", "node_ring", "node_edge")
TREE_KEYS = ("tree_min", "tree_node", "tree_corner", "tree_hits", "tree_first", "tree_mass")
STEP_KEYS = ("step_margin", "step_corner", "step_ring", "step_edge")
EGO_KEYS = ("ego_min", "ego_step", "ego_corner", "ego_hits", "ego_first")


def map_json(name):
    seq = scene_io.DEMO_SCENES[name]
    return os.path.join(ROOT, "tests", "golden", "raw", seq, f"log_map_archive_{seq}.json")


@functools.lru_cache(maxsize=None)
def demo_road(name):
    return audit.Road.from_map_json(map_json(name))


def blob(rng, n, centre=(0.0, 0.0), radius=30.0, wobble=0.35):
    """a simple (star-shaped) ring of n vertices about ``centre``: jittered increasing angles, radii within (1 +- wobble) radius"""
    ang = (np.arange(n) + 0.8 * rng.uniform(0.0, 1.0, n)) * (2.0 * np.pi / n)
    rad = radius * rng.uniform(1.0 - wobble, 1.0 + wobble, n)
    return np.stack([centre[0] + rad * np.cos(ang), centre[1] + rad * np.sin(ang)], 1)


def synth_road(seed, sizes, origin=(0.0, 0.0), spread=45.0):
    """a road of len(sizes) star-shaped rings (they may overlap), ring r of sizes[r] vertices, about ``origin``"""
    rng = np.random.default_rng(seed)
    rings = [blob(rng, n, (origin[0] + spread * k, origin[1] + 7.0 * (k % 2)), 30.0) for k, n in enumerate(sizes)]
    return audit.Road.from_polygons(rings)


def boxes_about(road, n, seed, pad=15.0):
    """n boxes (x, y, yaw) spread over the road's bounding box and ``pad`` metres beyond it"""
    rng = np.random.default_rng(seed)
    lo, hi = road.verts.min(0) - pad, road.verts.max(0) + pad
    return np.stack([rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.uniform(-3.5, 3.5, n)], 1)


# ---- the audits through the host entry ------------------------------------------------------------------------------------------------

def host_plan(flats, xs_per_tree, road, box=EGO_BOX):
    """what HipPredictor.audit_road_plan returns, from the host entry + the restatement's reductions; xs_per_tree: one [C, M_t, 6] per tree"""
    C, n = xs_per_tree[0].shape[0], len(flats)
    out = {k: [] for k in PLAN_KEYS}
    out.update(tree_min=np.zeros((C, n)), tree_node=np.zeros((C, n), np.int32), tree_corner=np.zeros((C, n), np.int32),
               tree_hits=np.zeros((C, n), np.int32), tree_first=np.zeros((C, n), np.int32), tree_mass=np.zeros((C, n)))
    for t, (f, xs) in enumerate(zip(flats, xs_per_tree)):
        M = xs.shape[1]
        rows = xs.reshape(-1, 6)
        res = _lib.road_margin(np.where(np.isfinite(rows).all(1, keepdims=True), rows[:, [0, 1, 3]], np.nan), box, road.verts, road.poly_off)
        for k, h in zip(PLAN_KEYS, ("margin", "corner", "ring", "edge")):
            out[k].append(res[h].reshape(C, M))
        for c in range(C):
            r = rr.reduce_tree(out["node_margin"][t][c], out["node_corner"][t][c], f["prob"])
            for k, v in zip(TREE_KEYS, r):
                out[k][c, t] = v
    return out


def same_plan(got, want):
    """bitwise equality of two audit_road_plan results (NaN == NaN)"""
    for k in PLAN_KEYS:
        assert len(got[k]) == len(want[k]), k
        for t, (g, w) in enumerate(zip(got[k], want[k])):
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype == np.float64), (k, t)
    for k in TREE_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=got[k].dtype == np.float64), (k, got[k], want[k])


def host_episode(egos, road, box=EGO_BOX):
    """what HipPredictor.audit_road_episode returns, from the host entry + the restatement's reductions; egos [E, S, 4]"""
    E, S = egos.shape[:2]
    rows = egos.reshape(-1, 4)
    res = _lib.road_margin(np.where(np.isfinite(rows).all(1, keepdims=True), rows[:, [0, 1, 3]], np.nan), box, road.verts, road.poly_off)
    out = {k: res[h].reshape(E, S) for k, h in zip(STEP_KEYS, ("margin", "corner", "ring", "edge"))}
    out.update(ego_min=np.zeros(E), ego_step=np.zeros(E, np.int32), ego_corner=np.zeros(E, np.int32), ego_hits=np.zeros(E, np.int32),
               ego_first=np.zeros(E, np.int32))
    for e in range(E):
        for k, v in zip(EGO_KEYS, rr.reduce_ego(out["step_margin"][e], out["step_corner"][e])):
            out[k][e] = v
    return out


def same_episode(got, want):
    for k, w in want.items():
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w, equal_nan=w.dtype == np.float64), (k, got[k], w)


# ---- an independent witness: world coordinates, vectorised, projection form, matplotlib's point-in-polygon ------------------------------

def corners_world(boxes, box=EGO_BOX):
    """[n, 4, 2]: the corners of the boxes (x, y, yaw) in world coordinates, in the order (+,+), (+,-), (-,-), (-,+)"""
    b = np.asarray(boxes, np.float64).reshape(-1, 3)
    L, W = box[0], box[1]
    off = box[2] if len(box) == 3 else 0.0
    loc = np.array([[L / 2, W / 2], [L / 2, -W / 2], [-L / 2, -W / 2], [-L / 2, W / 2]]) + np.array([off, 0.0])
    c, s = np.cos(b[:, 2]), np.sin(b[:, 2])
    rot = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)          # [n, 2, 2]
    return b[:, None, :2] + np.einsum("nij,kj->nki", rot, loc)


def witness(boxes, road, box=EGO_BOX):
    """-> dict over boxes: margin [n], corner [n], ring [n], edges [n] (the set of edges of that ring whose nearest point is the winning
    one), inside [n, 4, P], dist [n, 4, P], and ``gap``: the least distance of any decision from its edge -- min over |corner-ring
    distance|, best-vs-second corner, best-vs-second ring among the rings that decide, nearest-vs-next edge with another nearest point"""
    from matplotlib.path import Path
    pts = corners_world(boxes, box).reshape(-1, 2)
    n, P = len(pts), road.n_rings
    dist, inside, near_edges, edge_gap = np.zeros((n, P)), np.zeros((n, P), bool), [], np.full((n, P), np.inf)
    for r in range(P):
        ring = road.ring(r)
        A, B = ring, np.roll(ring, -1, axis=0)
        idx = np.flatnonzero(np.any(A != B, axis=1))
        A, B = A[idx], B[idx]
        E = B - A
        t = np.clip(np.einsum("nej,ej->ne", pts[:, None, :] - A[None], E) / np.einsum("ej,ej->e", E, E), 0.0, 1.0)
        Q = A[None] + t[:, :, None] * E[None]                                  # nearest point of every edge
        d = np.linalg.norm(pts[:, None, :] - Q, axis=2)
        k = np.argmin(d, axis=1)
        dist[:, r] = d[np.arange(n), k]
        same = np.linalg.norm(Q - Q[np.arange(n), k][:, None, :], axis=2) <= 1e-9
        near_edges.append([idx[row] for row in same])
        edge_gap[:, r] = np.where(same, np.inf, d - dist[:, r:r + 1]).min(axis=1)
        closed = np.concatenate([ring, ring[:1]])
        inside[:, r] = Path(closed, closed=True).contains_points(pts)
    any_in = inside.any(1)
    score = np.where(any_in[:, None], np.where(inside, dist, -np.inf), -dist)   # the deciding ring maximises this
    ring_of = np.argmax(score, axis=1)
    cm = score[np.arange(n), ring_of]
    srt = np.sort(score, axis=1)
    ring_gap = srt[:, -1] - srt[:, -2] if P > 1 else np.full(n, np.inf)
    nb = n // 4
    cm4 = cm.reshape(nb, 4)
    corner = np.argmin(cm4, axis=1)
    lim = np.arange(nb) * 4 + corner
    c_srt = np.sort(cm4, axis=1)
    gap = min(float(np.abs(dist).min()), float((c_srt[:, 1] - c_srt[:, 0]).min()), float(ring_gap[lim].min()),
              float(edge_gap[lim, ring_of[lim]].min()))
    return dict(margin=cm4[np.arange(nb), corner], corner=corner, ring=ring_of[lim], edges=[near_edges[ring_of[i]][i] for i in lim],
                inside=inside.reshape(nb, 4, P), dist=dist.reshape(nb, 4, P), corner_margin=cm4, gap=gap)
