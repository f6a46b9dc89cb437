"""Shared by tests/test_audit_host.py and tests/test_gpu_audit.py: the two audits evaluated through the library's HOST entry
(mind_debug_box_clearance, all pairs of a case in one call) and reduced by the restatement's rules (tests/box_geom_restate.py), and the
recorded scenes as audit inputs.  Not a test module."""
import functools

import numpy as np

import box_geom_restate as rs
from mind_amd import _lib, audit

EGO_BOX = audit.BOXES["VEHICLE"]


def host_plan_nodes(flat, xs, box=EGO_BOX, margin=audit.DEFAULT_EXO_MARGIN):
    """node_clear [M] / node_agent [M] of one candidate xs [M, 6] on one flat cost tree, pairs through the host entry with its own trig"""
    M, a = flat["cov"].shape
    clear, agent = np.full(M, np.inf), np.full(M, -1, np.int32)
    fin = np.all(np.isfinite(xs), axis=1)
    clear[~fin] = np.nan
    if a > 1 and fin.any():
        ii, jj = np.meshgrid(np.flatnonzero(fin), np.arange(1, a), indexing="ij")
        ii, jj = ii.ravel(), jj.ravel()
        A = np.stack([xs[ii, 0], xs[ii, 1], xs[ii, 3], np.full(len(ii), box[0]), np.full(len(ii), box[1])], 1)
        B = np.zeros((len(ii), 5))
        B[:, 0], B[:, 1] = flat["mean"][ii, jj, 0].astype(np.float64), flat["mean"][ii, jj, 1].astype(np.float64)
        B[:, 2] = flat["cov"][ii, jj].astype(np.float64) + np.float64(margin)
        d = _lib.box_clearance(0, A, B).reshape(-1, a - 1)
        for r, i in enumerate(np.flatnonzero(fin)):
            clear[i], agent[i] = rs.reduce_agents(d[r])
    return clear, agent


def host_plan(flats, xs_per_tree, box=EGO_BOX, margin=audit.DEFAULT_EXO_MARGIN):
    """what HipPredictor.audit_plan returns, from the host entry + the restatement's reductions; xs_per_tree: one [C, M_t, 6] per tree"""
    C, n = xs_per_tree[0].shape[0], len(flats)
    out = dict(node_clear=[], node_agent=[], tree_min=np.zeros((C, n)), tree_node=np.zeros((C, n), np.int32), tree_agent=np.zeros((C, n), np.int32),
               tree_hits=np.zeros((C, n), np.int32), tree_first=np.zeros((C, n), np.int32), tree_mass=np.zeros((C, n)))
    for t, (f, xs) in enumerate(zip(flats, xs_per_tree)):
        nc, na = np.zeros(xs.shape[:2]), np.zeros(xs.shape[:2], np.int32)
        for c in range(C):
            nc[c], na[c] = host_plan_nodes(f, xs[c], box, margin)
            r = rs.reduce_tree(nc[c], na[c], f["prob"])
            for k, v in zip(("tree_min", "tree_node", "tree_agent", "tree_hits", "tree_first", "tree_mass"), r):
                out[k][c, t] = v
        out["node_clear"].append(nc)
        out["node_agent"].append(na)
    return out


def same_plan(got, want):
    """bitwise equality of two audit_plan results (NaN == NaN)"""
    for k in ("node_clear", "node_agent"):
        assert len(got[k]) == len(want[k]), k
        for t, (g, w) in enumerate(zip(got[k], want[k])):
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype == np.float64), (k, t)
    for k in ("tree_min", "tree_node", "tree_agent", "tree_hits", "tree_first", "tree_mass"):
        assert np.array_equal(got[k], want[k], equal_nan=got[k].dtype == np.float64), (k, got[k], want[k])


def host_episode_steps(ego, exo, valid, boxes, ego_box=EGO_BOX, trig=None):
    """step_clear [S] / step_track [S] of one ego trace [S, 4], pairs through the host entry; trig: None = its own, else a function
    yaw -> (cos, sin) handed to it"""
    S, n = valid.shape
    clear, track = np.full(S, np.inf), np.full(S, -1, np.int32)
    ss, jj = np.nonzero(valid[:, 1:])
    jj = jj + 1
    if len(ss):
        A = np.stack([ego[ss, 0], ego[ss, 1], ego[ss, 3], np.full(len(ss), ego_box[0]), np.full(len(ss), ego_box[1])], 1)
        B = np.stack([exo[ss, jj, 0], exo[ss, jj, 1], exo[ss, jj, 2], boxes[jj, 0], boxes[jj, 1]], 1)
        tg = None
        if trig is not None:
            ca, sa = trig(A[:, 2])
            cb, sb = trig(B[:, 2])
            tg = np.stack([ca, sa, cb, sb], 1)
        d = _lib.box_clearance(1, A, B, tg)
        for s, j, v in zip(ss, jj, d):          # (np.nonzero: steps ascending, tracks ascending within a step)
            if v < clear[s]:
                clear[s], track[s] = v, j
    return clear, track


def host_episode(egos, exo, valid, boxes, ego_box=EGO_BOX):
    """what HipPredictor.audit_episode returns, from the host entry + the restatement's reductions; egos [E, S, 4]"""
    E, S = egos.shape[:2]
    out = dict(step_clear=np.zeros((E, S)), step_track=np.zeros((E, S), np.int32), ego_min=np.zeros(E), ego_step=np.zeros(E, np.int32),
               ego_track=np.zeros(E, np.int32), ego_hits=np.zeros(E, np.int32), ego_first=np.zeros(E, np.int32))
    for e in range(E):
        out["step_clear"][e], out["step_track"][e] = host_episode_steps(egos[e], exo, valid, boxes, ego_box)
        r = rs.reduce_ego(out["step_clear"][e], out["step_track"][e])
        for k, v in zip(("ego_min", "ego_step", "ego_track", "ego_hits", "ego_first"), r):
            out[k][e] = v
    return out


def same_episode(got, want):
    for k, w in want.items():
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (k, got[k], w)


def sim_times(n, step=0.02):
    """the simulator's clock: repeated float additions of SIM_STEP from 0.0 (closed_loop.py step_end, NativeLoop._tabulate)"""
    out, t = [], 0.0
    for _ in range(n):
        out.append(t)
        t += step
    return out


@functools.lru_cache(maxsize=None)
def recorded_scene(name):
    """(world, times, ego [S, 4], exo [S, n, 5], valid [S, n], boxes [n, 2]) of a recorded demo scene: the recorded ego against the
    recorded tracks at every recorded step"""
    from mind_amd.scene_io import ReplayWorld, scene_fixture_path
    w = ReplayWorld.from_scene_file(scene_fixture_path(name))
    times = sim_times(int(w.max_step) + 1)
    ego = np.stack([np.asarray(w.agent_state(0, t), np.float64) for t in times])
    exo, valid, boxes = audit.tabulate_exo(w, times)
    return w, times, ego, exo, valid, boxes
