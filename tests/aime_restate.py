"""Float64 restatement of the AIME glue (the arithmetic k_aime_world, k_aime_select, k_aime_branch / k_aime_select_branch and k_aime_rebase
run on the device), written from the reference's text: scenario_tree.py:82-100 / 592-611 (branch time), 281-412 (prune_merge), 467-567
(update_obser), 613-652 (get_high_level_command), utils.py:113-134 (actor features), 171-242 (lane graph frame, origin / rotation, RPE),
486-513 (distance to a polyline).  Plain numpy and scalar loops; no GPU, no mind_amd import.  No test in here.

Two kinds of function:
 * continuous quantities -- every float32 input is widened to float64 first and nothing is rounded on the way: the truth the float32 host
   path and the kernels are both measured against;
 * decisions -- the reference's float32 comparisons on GIVEN float32 inputs (one rounding per operation, as torch's float32 tensors give),
   each with the float64 margin of its closest comparison, so that a test can tell a decision that is exact by construction or clear of its
   threshold from one that is not."""
import numpy as np

F32 = np.float32
F64 = np.float64
K, T, T_OBS = 6, 60, 50
PI6_F32 = F32(np.pi / 6)


def _d(x):
    return np.asarray(x, F64)


def _rot(th):
    c, s = np.cos(th), np.sin(th)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def wrap(d):
    return np.arctan2(np.sin(d), np.cos(d))


# ------------------------------------------------------------------------------------------------------------------------------
# continuous: prune_merge's world frame (scenario_tree.py:323-347, 381-392)
# ------------------------------------------------------------------------------------------------------------------------------
def world(reg, vel, ctrs, vecs, rot, orig, cov_last):
    """One scene (agent 0 = ego).  reg [a,K,T,5], vel [a,K,T,2], ctrs / vecs [a,2], rot [2,2], orig [2], cov_last [a] float32.
    -> dict pos [a,K,T,2], vel [a,K,T,2], ang [a,K,T] float64, cov [a,K,T] FLOAT32 (one float32 maximum and one float32 addition: a
    bit-level fact), topo [a-1,K] float64 (NaN where the exo agent sits on the ego at some step)."""
    reg64, vel64, ctrs64, vecs64, rot64, orig64 = _d(reg), _d(vel), _d(ctrs), _d(vecs), _d(rot), _d(orig)
    th = np.arctan2(vecs64[:, 1], vecs64[:, 0])
    Ri = _rot(th)                                                                   # [a,2,2]
    RiT = np.transpose(Ri, (0, 2, 1))[:, None]
    pos = np.matmul(reg64[..., :2], RiT) + ctrs64[:, None, None, :]
    pos = np.matmul(pos, rot64.T) + orig64
    v = np.matmul(np.matmul(vel64, RiT), rot64.T)
    theta_g = np.arctan2(rot64[1, 0], rot64[0, 0])
    ang = np.arctan2(vel64[..., 1], vel64[..., 0]) + th[:, None, None] + theta_g
    reg32 = np.asarray(reg, F32)
    cov = np.maximum(reg32[..., 2], reg32[..., 3]) + np.asarray(cov_last, F32)[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = pos[1:] - pos[0:1]
        rel = rel / np.sqrt((rel * rel).sum(-1, keepdims=True))
        phi = np.arctan2(rel[..., 1], rel[..., 0])
        topo = wrap(phi[..., 1:] - phi[..., :-1]).sum(-1)
    return dict(pos=pos, vel=v, ang=ang, cov=cov, topo=topo, phi=phi)


def lane_distance(lane, p):
    """get_distance_to_polyline (utils.py:486-513) with its sequential `distance < min_distance`: a NaN segment distance (zero-length
    segment, 0 / 0 in the projection; torch.clamp keeps a NaN) is never taken, and never left when it is the first.  float64."""
    lane, p = _d(lane), _d(p)
    md = None
    for i in range(len(lane) - 1):
        p1, seg = lane[i], lane[i + 1] - lane[i]
        den = float(seg @ seg)
        t = float((p - p1) @ seg) / den if den != 0.0 else float("nan")            # 0 / 0
        if t < 0.0:
            t = 0.0
        elif t > 1.0:
            t = 1.0
        c = p1 + t * seg - p
        dist = float(np.sqrt(c @ c))
        if md is None or dist < md:
            md = dist
    return md


def ego_end(w, last, lane=None):
    """[K,4] float64: ego x, y at predicted step `last`, its max-sigma there, its distance to the target lane (inf without one)."""
    out = np.full((K, 4), np.inf)
    for k in range(K):
        out[k, :2] = w["pos"][0, k, last]
        out[k, 2] = w["cov"][0, k, last]
        if lane is not None:
            out[k, 3] = lane_distance(lane, out[k, :2])
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# decisions: prune_merge (:313-320, 368-379, 396-410) on given float32 signatures / end points
# ------------------------------------------------------------------------------------------------------------------------------
def select(cls_row, scen_prob, topo_exo, end=None, dist_thres=None, prob_floor=0.001):
    """cls_row [K], scen_prob, topo_exo [n_exo,K], end [K,4] (x, y, sigma, lane distance), float32.  -> sel [K] int (kept mode in visiting
    order, -1 padded), sel_prob [K] float32 (0 padded), margin: float64 distance of the closest wrapped signature difference to pi/6 among
    the pairs the merge compared (inf when none)."""
    cls_row = np.asarray(cls_row, F32)
    order = sorted(range(K), key=lambda k: (-float(cls_row[k]), k))                 # descending, first index first among equals
    cands = []
    for k in order:
        prob = F32(cls_row[k] * F32(scen_prob))
        if prob < F32(prob_floor):
            continue
        if dist_thres is not None:
            if F32(F32(end[k][3]) - F32(end[k][2])) > F32(dist_thres):
                continue
        cands.append((k, prob))
    topo_exo = np.asarray(topo_exo, F32).reshape(-1, K)
    kept, margin = [], np.inf
    while cands:
        k0, p0 = cands[0]
        kept.append((k0, p0))
        rest = []
        for k1, p1 in cands[1:]:
            d = wrap(_d(topo_exo[:, k0] - topo_exo[:, k1]))                         # float32 difference, wrapped in float64
            excess = np.abs(d) - F64(PI6_F32)
            if len(excess) and np.isfinite(excess).any():
                margin = min(margin, float(np.nanmin(np.abs(excess))))
            if (excess > 0).sum() > 0:                                              # NaN: not greater -> merged
                rest.append((k1, p1))
        cands = rest
    sel, selp = np.full(K, -1, np.int64), np.zeros(K, F32)
    for j, (k, p) in enumerate(kept):
        sel[j], selp[j] = k, p
    return sel, selp, margin


def hit_words(sigma, sel, cmp_t):
    """get_branch_time's test (:592-611) for every kept slot: sigma [a,K,T] float32 max-sigma of the scene's agents, sel [K] kept modes,
    cmp_t the compare step.  -> [K,2] uint32: bit t of (word 0: steps 0-31, word 1: steps 32-59) set when some agent's
    float32(sigma[t] / sigma[cmp_t]) > 9."""
    sigma = np.asarray(sigma, F32)
    out = np.zeros((K, 2), np.uint32)
    for j, k in enumerate(sel):
        if k < 0:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = sigma[:, k, :] / sigma[:, k, cmp_t][:, None]                    # float32 / float32
        hit = (ratio > F32(9)).any(axis=0)
        for t in range(T):
            if hit[t]:
                out[j, t // 32] |= np.uint32(1 << (t % 32))
    return out


def window_index(lane, orig, travel0):
    """get_high_level_command's index (:613-636): first minimum of the float32 distances to the lane points, the `travel` loop, the three
    clamps.  lane [n,2], orig [2], travel0 float32.  -> idx, dict(closest, gap: float64 gap between the two smallest DISTINCT-index
    distances, slack: float64 min |travel| at the loop's tests after the first step, steps)."""
    lane, orig = np.asarray(lane, F32), np.asarray(orig, F32)
    n = len(lane)
    d = lane - orig
    dist = np.sqrt((d * d).sum(-1), dtype=F32)
    closest = 0
    for q in range(1, n):
        if dist[q] < dist[closest]:
            closest = q
    d64 = np.sort(np.sqrt(((_d(lane) - _d(orig)) ** 2).sum(-1)))
    idx, travel, slack, steps = closest, F32(travel0), np.inf, 0
    while idx < n - 1 and travel > 0:
        idx += 1
        step = lane[idx] - lane[idx - 1]
        travel = F32(travel - np.sqrt(F32(step[0] * step[0] + step[1] * step[1]), dtype=F32))
        slack = min(slack, abs(float(travel)))
        steps += 1
    if idx == n - 1:
        idx -= 1
    idx = max(5, min(idx, n - 6))
    return idx, dict(closest=closest, gap=float(d64[1] - d64[0]), slack=slack, steps=steps)


# ------------------------------------------------------------------------------------------------------------------------------
# continuous: update_obser (:467-567) for one child scene
# ------------------------------------------------------------------------------------------------------------------------------
def rpe(ctrs, vecs, radius=100.0):
    """get_rpe (utils.py:193-242) -> [5,n,n] float64"""
    ctrs, vecs = _d(ctrs), _d(vecs)
    v_pos = ctrs[None, :, :] - ctrs[:, None, :]
    d_pos = np.sqrt((v_pos * v_pos).sum(-1)) * 2 / radius

    def cs(v1, v2):
        v1, v2 = np.broadcast_arrays(v1, v2)
        den = np.sqrt((v1 * v1).sum(-1)) * np.sqrt((v2 * v2).sum(-1)) + 1e-10
        return (v1[..., 0] * v2[..., 0] + v1[..., 1] * v2[..., 1]) / den, (v1[..., 0] * v2[..., 1] - v1[..., 1] * v2[..., 0]) / den

    c1, s1 = cs(vecs[None, :, :], vecs[:, None, :])
    c2, s2 = cs(vecs[None, :, :], v_pos)
    return np.stack([c1, s1, c2, s2, d_pos])


def rebase(pos, ang, vel, types, pad, lane_ctrs, lane_vecs, tlane, tinfo, idx):
    """One scene.  pos [a,50,2], ang [a,50], vel [a,50,2] world-frame windows, types [a,50,7], pad [a,50], lane_ctrs / lane_vecs [l,2],
    tlane [n,2], tinfo [n,12] float32; idx: the target-lane window index (a decision: window_index).  -> dict of float64 arrays named as
    the kernel's outputs: frames [28], actor_ctrs, actor_vecs [a,2], actors [a,14,48], lane_ctrs, lane_vecs [l,2], tgt_nodes [10,16],
    tgt_rpe [20], cur_vel."""
    pos, ang, vel = _d(pos), _d(ang), _d(vel)
    orig, theta = pos[0, T_OBS - 1], ang[0, T_OBS - 1]
    rot = _rot(theta)
    p1 = np.matmul(pos - orig, rot)
    a1 = ang - theta
    v1 = np.matmul(vel, rot)
    ctrs, th = p1[:, T_OBS - 1].copy(), a1[:, T_OBS - 1].copy()
    R = _rot(th)                                                                    # [a,2,2]
    pos_n = np.matmul(p1 - ctrs[:, None, :], R)
    ang_n = a1 - th[:, None]
    vel_n = np.matmul(v1, R)
    vecs = np.stack([np.cos(th), np.sin(th)], -1)
    disp = np.zeros_like(pos_n)
    disp[:, 1:] = pos_n[:, 1:] - pos_n[:, :-1]
    feat = np.concatenate([disp, np.stack([np.cos(ang_n), np.sin(ang_n)], -1), vel_n, _d(types), _d(pad)[..., None]], -1)
    actors = np.transpose(feat, (0, 2, 1))[..., 2:]
    lc = np.matmul(_d(lane_ctrs).reshape(-1, 2) - orig, rot)
    lv = np.matmul(_d(lane_vecs).reshape(-1, 2), rot)
    pts = _d(tlane)[idx - 5:idx + 6]
    info = _d(tinfo)[idx - 5:idx + 6][1:]
    ctrln = np.matmul(pts - orig, rot)
    anch_pos = ctrln.mean(axis=0)
    dv = ctrln[-1] - ctrln[0]
    anch_vec = dv / np.sqrt((dv * dv).sum())
    anch_rot = np.array([[anch_vec[0], -anch_vec[1]], [anch_vec[1], anch_vec[0]]])
    ctrln = np.matmul(ctrln - anch_pos, anch_rot)
    tgt_nodes = np.concatenate([(ctrln[:-1] + ctrln[1:]) / 2.0, ctrln[1:] - ctrln[:-1], info], -1)
    tgt_rpe = rpe(np.stack([anch_pos, ctrs[0]]), np.stack([anch_vec, vecs[0]])).reshape(-1)
    frames = np.concatenate([rot.reshape(-1), orig, pts.reshape(-1)])
    return dict(frames=frames, actor_ctrs=ctrs, actor_vecs=vecs, actors=actors, lane_ctrs=lc, lane_vecs=lv, tgt_nodes=tgt_nodes,
                tgt_rpe=tgt_rpe, cur_vel=float(np.sqrt((vel_n[0, -1] ** 2).sum())), pos_n=pos_n, ang_n=ang_n, vel_n=vel_n)


# ------------------------------------------------------------------------------------------------------------------------------
# continuous: the root scene (process_data :122-206 with utils.py:345-483's lane graph, prepare_root_data :414-465)
# ------------------------------------------------------------------------------------------------------------------------------
def root_lanes(pts, flags, orig, theta):
    """pts [l,11,2] float64 world-frame lane pieces, flags [l,6] (lane type, intersection, left / right mark class, left / right neighbour).
    -> lane_ctrs, lane_vecs [l,2] (AV frame), LANES [l,10,16] float64"""
    ctrln = np.matmul(_d(pts) - _d(orig), _rot(F64(theta)))
    anch_pos = ctrln.mean(axis=1)
    dv = ctrln[:, -1] - ctrln[:, 0]
    anch_vec = dv / np.sqrt((dv * dv).sum(-1, keepdims=True))
    anch_rot = np.stack([np.stack([anch_vec[:, 0], -anch_vec[:, 1]], -1), np.stack([anch_vec[:, 1], anch_vec[:, 0]], -1)], -2)
    inst = np.matmul(ctrln - anch_pos[:, None, :], anch_rot)
    l = len(inst)
    flags = np.asarray(flags)
    hot = lambda col: np.repeat(np.eye(3)[flags[:, col]][:, None, :], 10, 1)
    rep = lambda col: np.repeat(flags[:, col].astype(F64)[:, None, None], 10, 1)
    lanes = np.concatenate([(inst[:, :-1] + inst[:, 1:]) / 2.0, inst[:, 1:] - inst[:, :-1], rep(1), hot(0), hot(2), hot(3), rep(4), rep(5)], -1)
    assert lanes.shape == (l, 10, 16)
    return anch_pos, anch_vec, lanes


def root_hist(reb, orig, theta):
    """the root's world-frame histories as prepare_root_data rebuilds them from the NORMALISED arrays of rebase(): -> pos [a,50,2],
    ang [a,50], vel [a,50,2] float64"""
    th = np.arctan2(reb["actor_vecs"][:, 1], reb["actor_vecs"][:, 0])
    RiT = np.transpose(_rot(th), (0, 2, 1))
    rot = _rot(F64(theta))
    pos = np.matmul(np.matmul(reb["pos_n"], RiT) + reb["actor_ctrs"][:, None, :], rot.T) + _d(orig)
    vel = np.matmul(np.matmul(reb["vel_n"], RiT), rot.T)
    ang = reb["ang_n"] + th[:, None] + np.arctan2(rot[1, 0], rot[0, 0])
    return pos, ang, vel
