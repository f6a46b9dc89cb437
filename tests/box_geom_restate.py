"""numpy float64 restatement of mind_amd/csrc/box_geom.h and of the two audits built on it (audit_kernels.hip): scalar operations in the
header's order on np.float64 values -- IEEE double, no fused multiply-add -- so that the host entry and the kernels can be held to it bit
for bit.  (cos, sin) are inputs, as in the header.  Not a test module."""
import math

import numpy as np

F = np.float64


def point_rect(dx, dy, c, s, L, W):
    """bg_point_rect"""
    dx, dy, c, s, L, W = F(dx), F(dy), F(c), F(s), F(L), F(W)
    u = c * dx + s * dy
    v = (-s) * dx + c * dy
    qx = abs(u) - F(0.5) * L
    qy = abs(v) - F(0.5) * W
    if qx > 0.0 or qy > 0.0:
        mx = qx if qx > 0.0 else F(0.0)
        my = qy if qy > 0.0 else F(0.0)
        return np.sqrt(mx * mx + my * my)
    return qx if qx > qy else qy


_SL = (1.0, 1.0, -1.0, -1.0)
_SW = (1.0, -1.0, -1.0, 1.0)


def rect_rect(dx, dy, ca, sa, La, Wa, cb, sb, Lb, Wb):
    """bg_rect_rect; (dx, dy) = centre of B - centre of A"""
    dx, dy, ca, sa, cb, sb = F(dx), F(dy), F(ca), F(sa), F(cb), F(sb)
    hla, hwa, hlb, hwb = F(0.5) * F(La), F(0.5) * F(Wa), F(0.5) * F(Lb), F(0.5) * F(Wb)
    cc = abs(ca * cb + sa * sb)
    cs = abs(sa * cb - ca * sb)
    d = ((abs(ca * dx + sa * dy) - hla) - (hlb * cc + hwb * cs),
         (abs((-sa) * dx + ca * dy) - hwa) - (hlb * cs + hwb * cc),
         (abs(cb * dx + sb * dy) - (hla * cc + hwa * cs)) - hlb,
         (abs((-sb) * dx + cb * dy) - (hla * cs + hwa * cc)) - hwb)
    sep = d[0]
    for k in (1, 2, 3):
        if d[k] > sep:
            sep = d[k]
    if sep <= 0.0:
        return sep
    best = None
    for k in range(4):
        lx, ly = F(_SL[k]) * hla, F(_SW[k]) * hwa
        ox, oy = ca * lx - sa * ly, sa * lx + ca * ly
        v = point_rect(ox - dx, oy - dy, cb, sb, Lb, Wb)
        if best is None or v < best:
            best = v
    for k in range(4):
        lx, ly = F(_SL[k]) * hlb, F(_SW[k]) * hwb
        ox, oy = cb * lx - sb * ly, sb * lx + cb * ly
        v = point_rect(dx + ox, dy + oy, ca, sa, La, Wa)
        if v < best:
            best = v
    return best


def numpy_trig(yaw):
    """(cos, sin) from numpy, as float64 scalars"""
    return np.cos(F(yaw)), np.sin(F(yaw))


# ---- the reductions of the two audits, given the pairwise clearances ---------------------------------------------------------------

def reduce_agents(pair_clear):
    """k_audit_plan's per-node rule: pair_clear [a - 1] for the exo agents 1..a-1 -> (clear, agent); the lowest agent wins ties; none: +inf / -1"""
    best, bj = F(np.inf), -1
    for j, v in enumerate(pair_clear):
        if v < best:
            best, bj = v, j + 1
    return best, bj


def reduce_tree(node_val, node_tag, prob):
    """k_audit_plan_trees, for both audits (clearance: node_clear / node_agent; road: node_margin / node_corner):
    -> (min, node, tag, n_hit, first_hit, hit_mass); prob float32 [M]"""
    mn, mi, mt, hits, first, mass = F(np.inf), -1, -1, 0, -1, F(0.0)
    for i, v in enumerate(node_val):
        if v != v:
            return F(np.nan), i, -1, -1, -1, F(np.nan)
        if i == 0 or v < mn:
            mn, mi, mt = v, i, int(node_tag[i])
        if v < 0.0:
            if first < 0:
                first = i
            hits += 1
            mass = mass + F(np.float32(prob[i]))
    return mn, mi, mt, hits, first, mass


def reduce_ego(step_val, step_tag, nan_step=False):
    """k_audit_episode_egos<nan_step>, for both audits (clearance: step_clear / step_track, nan_step False; road: step_margin /
    step_corner, nan_step True): -> (min, step, tag, n_hit_steps, first_hit_step).  nan_step: a NaN step reports NaN, that step, -1, -1,
    -1; without it a NaN is compared like any value (at step 0 it stays the minimum, later it is passed over)"""
    mn, ms, mt, hits, first = F(np.inf), -1, -1, 0, -1
    for s, v in enumerate(step_val):
        if nan_step and v != v:
            return F(np.nan), s, -1, -1, -1
        if s == 0 or v < mn:
            mn, ms, mt = v, s, int(step_tag[s])
        if v < 0.0:
            if first < 0:
                first = s
            hits += 1
    return mn, ms, mt, hits, first


# ---- the audits themselves ---------------------------------------------------------------------------------------------------------

def plan_pairs(flat, xs, box, exo_margin, pair_fn):
    """node_clear [M] / node_agent [M] of ONE candidate xs [M, 6] on one flat cost tree.  pair_fn(state, disc) -> clearance of the disc
    disc = (x, y, r) from the ego box at state (x, y, yaw): the restatement below or the library's host entry"""
    M, a = flat["cov"].shape
    L, W = box
    clear, agent = np.zeros(M), np.zeros(M, np.int32)
    for i in range(M):
        if not np.all(np.isfinite(xs[i])):
            clear[i], agent[i] = np.nan, -1
            continue
        pc = [pair_fn((xs[i][0], xs[i][1], xs[i][3], L, W),
                      (F(flat["mean"][i, j, 0]), F(flat["mean"][i, j, 1]), F(flat["cov"][i, j]) + F(exo_margin))) for j in range(1, a)]
        clear[i], agent[i] = reduce_agents(pc)
    return clear, agent


def disc_pair_restated(trig=numpy_trig):
    def fn(state, disc):
        x, y, yaw, L, W = state
        c, s = trig(yaw)
        return point_rect(F(disc[0]) - F(x), F(disc[1]) - F(y), c, s, L, W) - F(disc[2])
    return fn


def rect_pair_restated(trig=numpy_trig):
    def fn(a, b):
        ca, sa = trig(a[2])
        cb, sb = trig(b[2])
        return rect_rect(F(b[0]) - F(a[0]), F(b[1]) - F(a[1]), ca, sa, a[3], a[4], cb, sb, b[3], b[4])
    return fn


def episode_steps(ego, exo, valid, boxes, ego_box, pair_fn):
    """step_clear [S] / step_track [S] of ONE ego trace [S, 4] = (x, y, v, yaw).  pair_fn(a, b) -> clearance of the rectangles
    a, b = (x, y, yaw, L, W)"""
    S, n = valid.shape
    clear, track = np.full(S, np.inf), np.full(S, -1, np.int32)
    for s in range(S):
        a = (ego[s][0], ego[s][1], ego[s][3], ego_box[0], ego_box[1])
        for j in range(1, n):
            if not valid[s, j]:
                continue
            v = pair_fn(a, (exo[s, j, 0], exo[s, j, 1], exo[s, j, 2], boxes[j][0], boxes[j][1]))
            if v < clear[s]:
                clear[s], track[s] = v, j
    return clear, track


def brute_rect_distance(dx, dy, ya, La, Wa, yb, Lb, Wb, n=150):
    """distance of two DISJOINT rectangles by sampling their edges (independent of the header's method; accuracy ~ perimeter / n)"""
    def edge_points(cx, cy, yaw, L, W):
        c, s = math.cos(yaw), math.sin(yaw)
        t = np.linspace(-1.0, 1.0, n)
        loc = np.concatenate([np.stack([t * L / 2, np.full(n, W / 2)], 1), np.stack([t * L / 2, np.full(n, -W / 2)], 1),
                              np.stack([np.full(n, L / 2), t * W / 2], 1), np.stack([np.full(n, -L / 2), t * W / 2], 1)])
        return np.stack([cx + c * loc[:, 0] - s * loc[:, 1], cy + s * loc[:, 0] + c * loc[:, 1]], 1)
    pa, pb = edge_points(0.0, 0.0, ya, La, Wa), edge_points(dx, dy, yb, Lb, Wb)
    return float(np.sqrt(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)).min())
