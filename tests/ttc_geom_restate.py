"""numpy float64 restatement of mind_amd/csrc/ttc_geom.h and of the audit built on it (ttc_kernels.hip): scalar operations in the header's
order on np.float64 values -- IEEE double, no fused multiply-add -- so that the host entry and the kernel can be held to it bit for bit.
(cos, sin) are inputs, as in the header.  Not a test module."""
import numpy as np

F = np.float64
INF = F(np.inf)


def _axis(ux, uy, R, dx, dy, wx, wy, enter, exit_):
    """tg_axis: -> (the axis can still be crossed, enter, exit)"""
    p = ux * dx + uy * dy
    q = ux * wx + uy * wy
    if q == 0.0:
        return bool(abs(p) < R), enter, exit_
    with np.errstate(over="ignore"):
        t1 = ((-R) - p) / q
        t2 = (R - p) / q
    lo, hi = (t1, t2) if t1 < t2 else (t2, t1)
    if lo > enter:
        enter = lo
    if hi < exit_:
        exit_ = hi
    return True, enter, exit_


def rect_rect_ttc(dx, dy, wx, wy, ca, sa, La, Wa, cb, sb, Lb, Wb):
    """tg_rect_rect_ttc; (dx, dy) = centre of B - centre of A, (wx, wy) = velocity of B - velocity of A"""
    dx, dy, wx, wy, ca, sa, cb, sb = F(dx), F(dy), F(wx), F(wy), F(ca), F(sa), F(cb), F(sb)
    hla, hwa, hlb, hwb = F(0.5) * F(La), F(0.5) * F(Wa), F(0.5) * F(Lb), F(0.5) * F(Wb)
    cc = abs(ca * cb + sa * sb)
    cs = abs(sa * cb - ca * sb)
    R0 = hla + (hlb * cc + hwb * cs)
    R1 = hwa + (hlb * cs + hwb * cc)
    R2 = (hla * cc + hwa * cs) + hlb
    R3 = (hla * cs + hwa * cc) + hwb
    enter, exit_ = -INF, INF
    for ux, uy, R in ((ca, sa, R0), (-sa, ca, R1), (cb, sb, R2), (-sb, cb, R3)):
        ok, enter, exit_ = _axis(ux, uy, R, dx, dy, wx, wy, enter, exit_)
        if not ok:
            return INF
    if enter < exit_ and exit_ > 0.0:
        return enter if enter > 0.0 else F(0.0)
    return INF


def pairs(a, b, tg):
    """rect_rect_ttc of the pairs a [n, 7], b [n, 7] = (x, y, yaw, L, W, vx, vy) with tg [n, 4] = (cos a, sin a, cos b, sin b), as
    mind_debug_box_ttc forms its arguments"""
    return np.array([rect_rect_ttc(b[i, 0] - a[i, 0], b[i, 1] - a[i, 1], b[i, 5] - a[i, 5], b[i, 6] - a[i, 6], tg[i, 0], tg[i, 1], a[i, 3], a[i, 4],
                                   tg[i, 2], tg[i, 3], b[i, 3], b[i, 4]) for i in range(len(a))])


def reduce_tracks(pair_ttc, tracks, horizon):
    """k_audit_ttc's per-step rule: the minimum over the valid tracks (ascending), the lowest winning ties; above the horizon: +inf / -1"""
    best, bj = INF, -1
    for t, j in zip(pair_ttc, tracks):
        if t < best:
            best, bj = t, int(j)
    if best > horizon:
        best, bj = INF, -1
    return best, bj


def reduce_ego(step_ttc, step_track, bound):
    """k_audit_episode_egos<false> with the bar `bound`: -> (min, step, track, n_hit_steps, first_hit_step)"""
    mn, ms, mt, hits, first = INF, -1, -1, 0, -1
    for s, v in enumerate(step_ttc):
        if s == 0 or v < mn:
            mn, ms, mt = v, s, int(step_track[s])
        if v < bound:
            if first < 0:
                first = s
            hits += 1
    return mn, ms, mt, hits, first
