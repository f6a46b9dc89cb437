"""numpy float64 restatement of mind_amd/csrc/lane_geom.h and of the reductions of the lane audit (audit_kernels.hip, k_lane_progress): scalar
operations in the header's order on np.float64 values -- IEEE double, no fused multiply-add -- so that the host entry and the kernels can be
held to it bit for bit.  (cos, sin) are inputs, as in the header.  Below it an independent witness by another route: world coordinates, a
vectorised closed form with argmin, no code shared with the restatement.  Not a test module."""
import numpy as np

from box_geom_restate import reduce_ego as _ego_fold, reduce_tree  # noqa: F401  (reduce_tree: k_audit_plan_trees over node_margin / node_lane)
from road_geom_restate import numpy_trig, rel  # noqa: F401  (rel: rg_rel)

F = np.float64
KEYS = ("lat", "s", "along", "across", "lane", "edge")


def seg(Ax, Ay, Bx, By, c, s):
    """lg_seg -> None when the segment is skipped, else (d2, along, t, ll, cr, across)"""
    if Ax == Bx and Ay == By:
        return None
    Ex, Ey = Bx - Ax, By - Ay
    ll = Ex * Ex + Ey * Ey
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        rl = F(1.0) / ll
        t = -(Ax * Ex + Ay * Ey)
        cr = Ax * By - Ay * Bx
        if t <= 0.0:
            d2 = Ax * Ax + Ay * Ay
        elif t >= ll:
            d2 = Bx * Bx + By * By
        else:
            d2 = (cr * cr) * rl
        ln = np.sqrt(ll)
        along = (c * Ex + s * Ey) / ln
        across = (s * Ex - c * Ey) / ln
    return d2, along, t, ll, cr, across


def take(m, d2, g):
    """lg_take on m = [d2, g]"""
    if d2 < m[0] or (d2 == m[0] and g < m[1]):
        m[0], m[1] = d2, g


def cum_of(verts, lane_off):
    """lg_cum"""
    cum = np.zeros(len(verts))
    for l in range(len(lane_off) - 1):
        acc = F(0.0)
        for v in range(int(lane_off[l]) + 1, int(lane_off[l + 1])):
            dx, dy = F(verts[v][0]) - F(verts[v - 1][0]), F(verts[v][1]) - F(verts[v - 1][1])
            acc = acc + np.sqrt(dx * dx + dy * dy)
            cum[v] = acc
    return cum


def lane_of(lane_off, g):
    """lg_lane_of"""
    return int(np.searchsorted(np.asarray(lane_off), g, side="right")) - 1


def finish(m, px, py, c, s, off, verts, lane_off, cum):
    """lg_finish -> (lat, s, along, across, lane, edge)"""
    g = int(m[1])
    if g < 0:
        return F(np.inf), F(np.nan), F(np.nan), F(np.nan), -1, -1
    Ax, Ay = rel(verts[g][0], verts[g][1], px, py, off, c, s)
    Bx, By = rel(verts[g + 1][0], verts[g + 1][1], px, py, off, c, s)
    d2, along, t, ll, cr, across = seg(Ax, Ay, Bx, By, c, s)
    dist = np.sqrt(d2)
    lat = dist if cr >= 0.0 else -dist
    tc = F(0.0) if t <= 0.0 else (ll if t >= ll else t)
    l = lane_of(lane_off, g)
    return lat, F(cum[g]) + tc / np.sqrt(ll), along, across, l, g - int(lane_off[l])


def box_lanes(px, py, c, s, off, cos_flow, bound, verts, lane_off, cum, order=None):
    """lg_box_lanes -> ((any), (flow), margin); ``order``: the segments in another order than the header's walk (the minimum does not care)"""
    c, s, cos_flow = F(c), F(s), F(cos_flow)
    any_, flow = [F(np.inf), -1], [F(np.inf), -1]
    segs = [v - 1 for l in range(len(lane_off) - 1) for v in range(int(lane_off[l]) + 1, int(lane_off[l + 1]))]
    for g in (segs if order is None else [segs[i] for i in order(len(segs))]):
        Ax, Ay = rel(verts[g][0], verts[g][1], px, py, off, c, s)
        Bx, By = rel(verts[g + 1][0], verts[g + 1][1], px, py, off, c, s)
        r = seg(Ax, Ay, Bx, By, c, s)
        if r is None:
            continue
        take(any_, r[0], g)
        if r[1] >= cos_flow:
            take(flow, r[0], g)
    a = finish(any_, px, py, c, s, off, verts, lane_off, cum)
    f = finish(flow, px, py, c, s, off, verts, lane_off, cum)
    return a, f, F(bound) - abs(f[0])


def project(boxes, ego_box, verts, lane_off, cos_flow, bound, trig=numpy_trig, order=None):
    """what _lib.lane_project returns, for boxes [n, 3] = (x, y, yaw), with (cos, sin) from ``trig``; a non-finite row: NaN / -1"""
    b = np.asarray(boxes, np.float64).reshape(-1, 3)
    off = ego_box[2] if len(ego_box) == 3 else 0.0
    n = len(b)
    out = {k: np.zeros((2, n), np.int32 if k in ("lane", "edge") else np.float64) for k in KEYS}
    out["margin"] = np.zeros(n)
    cum = cum_of(verts, lane_off)
    for i, (x, y, yaw) in enumerate(b):
        if not np.all(np.isfinite(b[i])):
            nan = (np.nan, np.nan, np.nan, np.nan, -1, -1)
            a, f, m = nan, nan, np.nan
        else:
            c, s = trig(yaw)
            a, f, m = box_lanes(x, y, c, s, off, cos_flow, bound, verts, lane_off, cum, order)
        for q, r in enumerate((a, f)):
            for k, v in zip(KEYS, r):
                out[k][q, i] = v
        out["margin"][i] = m
    return out


# ---- the reductions, given the per-box results ------------------------------------------------------------------------------------------

def reduce_ego(step_margin, step_lane_flow):
    """k_audit_episode_egos<true> with the bar 0.0: -> (min, step, lane, n_hit_steps, first_hit_step)"""
    return _ego_fold(step_margin, step_lane_flow, nan_step=True)


def progress_ego(lane_any, s_any):
    """k_lane_progress<false> -> (progress, back)"""
    prog, back = F(0.0), F(0.0)
    for k in range(1, len(lane_any)):
        if lane_any[k] < 0 or lane_any[k] != lane_any[k - 1]:
            continue
        d = F(s_any[k]) - F(s_any[k - 1])
        prog = prog + d
        if d < 0.0:
            back = back + d
    return prog, back


def progress_tree(parent, prob, lane_any, s_any):
    """k_lane_progress<true>; prob float32 [M]"""
    acc = F(0.0)
    for i in range(len(parent)):
        p = int(parent[i])
        if p < 0 or lane_any[i] < 0 or lane_any[i] != lane_any[p]:
            continue
        acc = acc + F(np.float32(prob[i])) * (F(s_any[i]) - F(s_any[p]))
    return acc


# ---- an independent witness: world coordinates, every segment at once, the projected point, argmin ------------------------------------------

def witness(boxes, ego_box, verts, lane_off, cos_flow):
    """-> dict: lat, s, along, across [2, n], lane [2, n], segs (per row and box the set of global segments whose nearest point is the
    winner's), and ``gap``: the least distance of any decision from its edge -- nearest against the next segment with another nearest point,
    |along - cos_flow| of every segment within reach, |cross| of the winners (the sign of lat)"""
    b = np.asarray(boxes, np.float64).reshape(-1, 3)
    off = ego_box[2] if len(ego_box) == 3 else 0.0
    verts, lane_off = np.asarray(verts, np.float64), np.asarray(lane_off)
    h = np.stack([np.cos(b[:, 2]), np.sin(b[:, 2])], 1)
    ctr = b[:, :2] + off * h
    first = np.ones(len(verts), bool)
    first[lane_off[:-1]] = False                               # vertex v ends a segment unless it begins a lane
    g = np.flatnonzero(first) - 1
    A, B = verts[g], verts[g + 1]
    keep = np.any(A != B, axis=1)
    g, A, B = g[keep], A[keep], B[keep]
    E = B - A
    ln = np.linalg.norm(E, axis=1)
    e = E / ln[:, None]
    u = np.clip(np.einsum("nsj,sj->ns", ctr[:, None, :] - A[None], e), 0.0, ln[None])        # arc length along each segment
    Q = A[None] + u[:, :, None] * e[None]
    d = np.linalg.norm(ctr[:, None, :] - Q, axis=2)
    along = h @ e.T
    across = e[None, :, 0] * h[:, None, 1] - e[None, :, 1] * h[:, None, 0]
    cross = e[None, :, 0] * (ctr[:, None, 1] - A[None, :, 1]) - e[None, :, 1] * (ctr[:, None, 0] - A[None, :, 0])      # > 0: left of travel
    start = np.cumsum(np.where(first, np.linalg.norm(np.diff(verts, axis=0, prepend=verts[:1]), axis=1), 0.0))
    base = start - start[lane_off[np.searchsorted(lane_off, np.arange(len(verts)), side="right") - 1]]        # arc length at every vertex
    n = len(b)
    out = {k: np.full((2, n), np.nan) for k in ("lat", "s", "along", "across")}
    out["lane"], segs, gap = np.full((2, n), -1), [[None] * n, [None] * n], np.inf
    gap = min(gap, float(np.abs(along - cos_flow)[d < d.min(1, keepdims=True) + 50.0].min()))
    for q, mask in enumerate((np.ones_like(d, bool), along >= cos_flow)):
        dm = np.where(mask, d, np.inf)
        k = np.argmin(dm, axis=1)
        for i in range(n):
            if not np.isfinite(dm[i, k[i]]):
                out["lat"][q, i] = np.inf
                segs[q][i] = set()
                continue
            same = mask[i] & (np.linalg.norm(Q[i] - Q[i, k[i]], axis=1) <= 1e-9)
            k[i] = np.flatnonzero(same)[0]                     # (segments meeting in the nearest point tie: the header names the lowest)
            segs[q][i] = set(g[same].tolist())
            others = dm[i][~same]
            if len(others):
                gap = min(gap, float(others.min() - dm[i, k[i]]))
            gap = min(gap, abs(float(cross[i, k[i]])))
            out["lat"][q, i] = np.copysign(d[i, k[i]], cross[i, k[i]])
            out["s"][q, i] = base[g[k[i]]] + u[i, k[i]]
            out["along"][q, i], out["across"][q, i] = along[i, k[i]], across[i, k[i]]
            out["lane"][q, i] = np.searchsorted(lane_off, g[k[i]], side="right") - 1
    out["segs"], out["gap"] = segs, gap
    return out
