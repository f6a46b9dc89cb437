"""numpy float64 restatement of mind_amd/csrc/road_geom.h and of the reductions of the road audit (audit_kernels.hip): scalar operations in
the header's order on np.float64 values -- IEEE double, no fused multiply-add -- so that the host entry and the kernels can be held to it
bit for bit.  (cos, sin) are inputs, as in the header.  Not a test module."""
import numpy as np

from box_geom_restate import reduce_ego as _ego_fold, reduce_tree  # noqa: F401  (reduce_tree: k_audit_plan_trees over node_margin / node_corner)

F = np.float64
_SL = (1.0, 1.0, -1.0, -1.0)
_SW = (1.0, -1.0, -1.0, 1.0)


class Corner:
    """rg_corner"""

    def __init__(self, ox, oy):
        self.ox, self.oy = ox, oy
        self.d2, self.par, self.edge = F(0.0), 0, -1
        self.in_d, self.out_d = F(0.0), F(0.0)
        self.in_ring = self.in_edge = self.out_ring = self.out_edge = -1


def rel(vx, vy, px, py, off, c, s):
    """rg_rel"""
    return (F(vx) - F(px)) - F(off) * F(c), (F(vy) - F(py)) - F(off) * F(s)


def box_begin(c, s, L, W):
    """rg_box_begin"""
    c, s = F(c), F(s)
    hl, hw = F(0.5) * F(L), F(0.5) * F(W)
    q = []
    for k in range(4):
        lx, ly = F(_SL[k]) * hl, F(_SW[k]) * hw
        q.append(Corner(c * lx - s * ly, s * lx + c * ly))
    return q


def ring_begin(q):
    """rg_ring_begin"""
    for k in q:
        k.d2, k.par, k.edge = F(np.inf), 0, -1


def edge(q, Ax, Ay, Bx, By, e):
    """rg_edge"""
    if Ax == Bx and Ay == By:
        return
    Ex, Ey = Bx - Ax, By - Ay
    ll = Ex * Ex + Ey * Ey
    with np.errstate(over="ignore", divide="ignore"):
        rl = F(1.0) / ll
    for k in q:
        ax, ay, bx, by = Ax - k.ox, Ay - k.oy, Bx - k.ox, By - k.oy
        cr = ax * by - ay * bx
        if (ay > 0.0) != (by > 0.0):
            if (cr > 0.0) if by > ay else (cr < 0.0):
                k.par ^= 1
        t = -(ax * Ex + ay * Ey)
        if t <= 0.0:
            d2 = ax * ax + ay * ay
        elif t >= ll:
            d2 = bx * bx + by * by
        else:
            d2 = (cr * cr) * rl
        if d2 < k.d2:
            k.d2, k.edge = d2, e


def ring_end(q, r):
    """rg_ring_end"""
    for k in q:
        d = np.sqrt(k.d2)
        if k.par and (k.in_ring < 0 or d > k.in_d):
            k.in_d, k.in_ring, k.in_edge = d, r, k.edge
        if k.out_ring < 0 or d < k.out_d:
            k.out_d, k.out_ring, k.out_edge = d, r, k.edge


def corner_margin(k):
    """one corner's (margin, ring, edge), as rg_box_end forms it"""
    return (k.in_d, k.in_ring, k.in_edge) if k.in_ring >= 0 else (-k.out_d, k.out_ring, k.out_edge)


def box_end(q):
    """rg_box_end -> (margin, corner, ring, edge)"""
    best = None
    for i, k in enumerate(q):
        m, r, e = corner_margin(k)
        if best is None or m < best[0]:
            best = (m, i, r, e)
    return best


def box_road(px, py, c, s, L, W, off, verts, poly_off, corners=False):
    """rg_box_road -> (margin, corner, ring, edge); corners=True: also the four corner margins"""
    q = box_begin(c, s, L, W)
    for r in range(len(poly_off) - 1):
        v0, n = int(poly_off[r]), int(poly_off[r + 1] - poly_off[r])
        Fx, Fy = rel(verts[v0][0], verts[v0][1], px, py, off, c, s)
        Ax, Ay = Fx, Fy
        ring_begin(q)
        for i in range(1, n):
            Bx, By = rel(verts[v0 + i][0], verts[v0 + i][1], px, py, off, c, s)
            edge(q, Ax, Ay, Bx, By, i - 1)
            Ax, Ay = Bx, By
        edge(q, Ax, Ay, Fx, Fy, n - 1)
        ring_end(q, r)
    return box_end(q) + ((tuple(corner_margin(k)[0] for k in q),) if corners else ())


def numpy_trig(yaw):
    """(cos, sin) from numpy, as float64 scalars"""
    return np.cos(F(yaw)), np.sin(F(yaw))


def margins(boxes, ego_box, verts, poly_off, trig=numpy_trig):
    """what _lib.road_margin returns, for boxes [n, 3] = (x, y, yaw), with (cos, sin) from ``trig``; a non-finite row: NaN / -1 / -1 / -1"""
    b = np.asarray(boxes, np.float64).reshape(-1, 3)
    L, W = ego_box[0], ego_box[1]
    off = ego_box[2] if len(ego_box) == 3 else 0.0
    out = dict(margin=np.zeros(len(b)), corner=np.zeros(len(b), np.int32), ring=np.zeros(len(b), np.int32), edge=np.zeros(len(b), np.int32))
    for i, (x, y, yaw) in enumerate(b):
        if not np.all(np.isfinite(b[i])):
            r = (np.nan, -1, -1, -1)
        else:
            c, s = trig(yaw)
            r = box_road(x, y, c, s, L, W, off, verts, poly_off)
        out["margin"][i], out["corner"][i], out["ring"][i], out["edge"][i] = r
    return out


# ---- the reductions of the two audits, given the per-box results: the clearance audit's folds, the NaN rule on ----------------------------

def reduce_ego(step_margin, step_corner):
    """k_audit_episode_egos<true>: -> (min, step, corner, n_hit_steps, first_hit_step)"""
    return _ego_fold(step_margin, step_corner, nan_step=True)
