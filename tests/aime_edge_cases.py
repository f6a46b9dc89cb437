"""Named input families for the AIME glue kernels: every family exists because one line of a kernel can go wrong there (the wrap of the
topology angle, the `> 9` edge, the argmin tie-break, the window clamps, ...).  Pure functions of a seed, the smallest shapes that still
reach the mechanism.  No GPU, no mind_amd import.  No test in here.

 world_cases(seed)   -> inputs of one mind_aime_world call each          (families cut, winding, far, lane_ends)
 decide_cases(seed)  -> inputs of one mind_debug_aime_decide call each   (families sig, edges; plus the refused forms)
 rebase_cases(seed)  -> inputs of one mind_aime_rebase call each         (families headings, lane_pos, wide, far)"""
import numpy as np

F32 = np.float32
K, T = 6, 60
PI = np.pi


def _rot2(theta):
    c, s = np.cos(theta, dtype=F32), np.sin(theta, dtype=F32)
    return np.array([[c, -s], [s, c]], dtype=F32)


def _local(world_xy, ctr, vec, rot, orig):
    """the agent-frame coordinates whose world position is world_xy (float64 inverse of prune_merge's transform, rounded once)"""
    th = np.arctan2(float(vec[1]), float(vec[0]))
    Ri = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    x = np.matmul(np.asarray(world_xy, np.float64) - np.asarray(orig, np.float64), np.asarray(rot, np.float64))
    return np.matmul(x - np.asarray(ctr, np.float64), Ri).astype(F32)


def _base_world(rng, counts, thetas, origs, spread=40.0):
    a_off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    A, B = int(a_off[-1]), len(counts)
    t = np.arange(1, T + 1, dtype=F32) * F32(0.1)
    reg = np.zeros((A, K, T, 5), F32)
    reg[..., 0] = rng.uniform(2, 9, (A, K, 1)).astype(F32) * t
    reg[..., 1] = rng.normal(0, 2.0, (A, K, 1)).astype(F32) * (t / 6) ** 2
    reg[..., 2:4] = rng.uniform(0.1, 3.0, (A, K, T, 2))
    vel = rng.normal(0, 3.0, (A, K, T, 2)).astype(F32)
    ctrs = rng.uniform(-spread, spread, (A, 2)).astype(F32)
    th = rng.uniform(-PI, PI, A)
    vecs = np.stack([np.cos(th), np.sin(th)], -1).astype(F32)
    return dict(reg=reg, vel=vel, ctrs=ctrs, vecs=vecs, a_off=a_off, rots=np.stack([_rot2(F32(x)) for x in thetas]),
                origs=np.asarray(origs, F32).reshape(B, 2), cov_last=rng.uniform(1e-5, 0.5, A).astype(F32), last=[T - 1] * B, lane=None,
                dist_thres=None)


def _straight_lane(n, p0, heading, spacing=1.0):
    s = np.arange(n, dtype=np.float64) * spacing
    return (np.asarray(p0, np.float64) + np.stack([s * np.cos(heading), s * np.sin(heading)], -1)).astype(F32)


def world_cases(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    # ---- cut: atan2 at its axes and at the +-pi cut, for the agent frames, the scene rotation and the velocity heading
    c = _base_world(rng, [1, 2, 9], [PI - 1e-3, -PI + 1e-3, 0.3], rng.uniform(-200, 200, (3, 2)))
    c["vecs"][[0, 1, 2, 3, 4, 5]] = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [-1, -0.0], [-1, 0.0]], F32)
    v = c["vel"]
    v[:, 0, 0] = (0.0, 0.0)
    v[:, 1, 0] = (-0.0, -0.0)
    v[:, 2, 0] = (-3.0, 1e-30)
    v[:, 3, 0] = (-3.0, -1e-30)
    v[:, 4, 0] = (-0.0, 0.0)
    v[:, 5, 0] = (0.0, -0.0)
    c["lane"] = _straight_lane(40, c["origs"][0] - 10.0, 0.4)
    out.append(("cut", c))
    # ---- winding: exo agents behind the ego (phi crosses the +-pi cut once and twice), around it (more than one turn), and ON it at one step
    c = _base_world(rng, [5, 2], [2.0, -0.7], rng.uniform(-200, 200, (2, 2)))
    s = np.linspace(0.0, 1.0, T)
    for b, a0 in enumerate(c["a_off"][:-1]):
        rot, orig = c["rots"][b], c["origs"][b]
        for k in range(K):
            f = 1.0 + 0.03 * k
            ego = np.stack([0.05 * np.arange(T), np.zeros(T)], -1)                   # scene-frame metres, before ROT / ORIG
            if b == 0:
                tracks = [ego,
                          np.stack([np.full(T, -5.0 * f), -3.0 + 6.0 * s], -1),                         # behind, once through the cut
                          np.stack([np.full(T, -5.0 * f), -3.0 * np.cos(2 * PI * s)], -1),              # behind and back: twice
                          6.0 * f * np.stack([np.cos(0.3 + 2.6 * PI * s), np.sin(0.3 + 2.6 * PI * s)], -1) + ego,   # 1.3 turns
                          ego + np.stack([0.3 * (np.arange(T) - 20.0), 0.1 * (np.arange(T) - 20.0)], -1)]     # on the ego at step 20
            else:
                tracks = [ego, 4.0 * f * np.stack([np.cos(-1.0 - 4.4 * PI * s), np.sin(-1.0 - 4.4 * PI * s)], -1) + ego]   # 2.2 turns, clockwise
            for i, tr in enumerate(tracks):
                w = np.matmul(tr, np.asarray(rot, np.float64).T) + orig
                c["reg"][a0 + i, k, :, :2] = _local(w, c["ctrs"][a0 + i], c["vecs"][a0 + i], rot, orig)
    a0 = c["a_off"][0]
    c["ctrs"][a0 + 4], c["vecs"][a0 + 4] = c["ctrs"][a0], c["vecs"][a0]               # same frame, same numbers at step 20: exactly on the ego
    c["reg"][a0 + 4, :, :, :2] = c["reg"][a0, :, :, :2] + (c["reg"][a0 + 4, :, :, :2] - c["reg"][a0 + 4, :, 20:21, :2])
    c["reg"][a0 + 4, :, 20, :2] = c["reg"][a0, :, 20, :2]
    out.append(("winding", c))
    # ---- far: origins 5 km out, agents metres apart -- the subtraction exo - ego cancels in float32
    c = _base_world(rng, [9, 2], [1.1, -2.6], [[5000.0, -5000.0], [-5000.0, 5000.0]], spread=12.0)
    c["ctrs"][c["a_off"][:-1]] = 0.0
    c["lane"] = _straight_lane(65, (4990.0, -5010.0), 1.0)
    out.append(("far", c))
    # ---- lane_ends: last in {0, 59, -1}; lanes of 2, 64, 65 and 129 points (one, one, two and three strides of the 64 lanes); end points
    #      before the lane's start (t clamps at 0) and past its end (t clamps at 1); a repeated interior point; a repeated first point
    for name, n, rep in (("lane2", 2, None), ("lane64", 64, None), ("lane65", 65, None), ("lane129", 129, None),
                         ("lane_repeat_interior", 12, 5), ("lane_repeat_first", 12, 1)):
        th = [0.7, -2.2, 0.1]
        c = _base_world(rng, [1, 2, 1], th, rng.uniform(-150, 150, (3, 2)))
        c["last"] = [0, T - 1, -1]
        spacing = 40.0 if n == 2 else 1.0
        p0, hd = c["origs"][0].astype(np.float64) + (3.0, -2.0), 0.9
        lane = _straight_lane(n, p0, hd, spacing)
        if rep is not None:
            lane[rep] = lane[rep - 1]
        c["lane"] = lane
        length = (n - 1) * spacing
        u, nrm = np.array([np.cos(hd), np.sin(hd)]), np.array([-np.sin(hd), np.cos(hd)])
        for b in (0, 1):
            a0 = c["a_off"][b]
            for k in range(K):
                # scene 0 (last = 0): step 0 lies 3 m BEFORE the lane's start (modes 0-2) or beside an interior point; scene 1 (last = 59):
                # step 59 lies 5 m PAST its end (modes 0-2) or beside the repeated / an interior point; lateral offsets 1 .. 30 m
                lat = (1.0, 6.0, 30.0)[k % 3] * (1 if k < 3 else -1)
                if b == 0:
                    along0, along1 = (-3.0, length + 2.0) if k < 3 else (0.37 * length, 0.9 * length)
                else:
                    along0, along1 = (-1.0, length + 5.0) if k < 3 else (0.1 * length, ((rep - 1) * spacing + 0.2) if rep is not None else 0.61 * length)
                al = along0 + (along1 - along0) * np.linspace(0, 1, T)
                w = p0 + al[:, None] * u + lat * nrm
                c["reg"][a0, k, :, :2] = _local(w, c["ctrs"][a0], c["vecs"][a0], c["rots"][b], c["origs"][b])
        c["dist_thres"] = 20.0
        out.append((name, c))
    return out


# --------------------------------------------------------------------------------------------------------------------------------
def _decide_base(rng, B, a):
    A = B * a
    world = np.zeros((A, K, T, 6), F32)
    world[..., 5] = 1.0
    cls = rng.dirichlet(np.full(K, 2.0), B).astype(F32)
    topo = np.zeros((A, K), F32)
    end = np.zeros((B, K, 4), F32)
    end[..., 2], end[..., 3] = 1.0, 5.0
    return dict(a_off=np.arange(B + 1) * a, cmp=np.ones(B, np.int32), cls=cls, scen_prob=np.ones(B, F32), topo=topo, ego_end=end, world=world,
                dist_thres=20.0, prob_floor=0.001)


SIG_VALUES = [2 * PI * k + s * (PI / 6 + m * 1e-4) for k in (0, 1, -1, 3, -3, 15, -15) for s in (1, -1) for m in (1, -1)]


def decide_cases(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    # ---- sig: signature differences at 2 pi k +- (pi/6 +- 1e-4): mode 0 leads with signature 0, five other modes each carry one value
    B, a = 6, 7
    c = _decide_base(rng, B, a)
    vals = SIG_VALUES + [1.0, -2.0]
    for b in range(B):
        c["cls"][b] = np.array([0.3, 0.2, 0.15, 0.14, 0.11, 0.1], F32)
        exo = 1 + (b % (a - 1))
        c["topo"][b * a + exo, 1:] = np.array(vals[5 * b:5 * b + 5], F32)
        c["topo"][b * a + 1 + ((b + 3) % (a - 1))] += F32(0.25 * b)                  # a common offset on another agent changes nothing
    c["topo"][2 * a + 6, 3] = np.nan                                                  # NaN signatures never differ
    c["topo"][4 * a + 1, :] = np.nan
    out.append(("sig", c))
    # ---- edges: one case per agent count (the fused kernel walks the agents eight at a time), eight scenes each
    for a in (1, 7, 8, 9, 16, 17):
        B = 8
        c = _decide_base(rng, B, a)
        c["cmp"][:] = [1, 7, 1, 23, 23, 7, 7, 1]
        last = lambda b: b * a + a - 1                                                # the deciding agent: the scene's last
        sig = c["world"][..., 5]
        for b in range(B):                                                            # well separated signatures: no merge unless stated
            if a > 1:
                c["topo"][b * a + 1, :] = np.arange(K, dtype=F32) * F32(1.0)
        # s0: all six cls equal -- the stable order decides; s1: two pairs of equal cls
        c["cls"][0] = F32(1.0 / 6.0)
        c["cls"][1] = np.array([0.2, 0.3, 0.3, 0.1, 0.05, 0.05], F32)
        if a > 1:
            c["topo"][1 * a + 1, 5] = c["topo"][1 * a + 1, 4]                          # mode 5 merges into mode 4 (tied cls, lower index first)
        # s2: path probability exactly on the floor (kept) and one ulp below (pruned)
        c["cls"][2] = np.array([0.5, 0.001, np.nextafter(F32(0.001), F32(0)), 0.3, 0.15, 0.048], F32)
        # s3: lane excess exactly on the threshold (kept), one ulp above (pruned), NaN distance (kept)
        c["ego_end"][3, 0, 3] = 21.0
        c["ego_end"][3, 1, 3] = np.nextafter(F32(21.0), F32(np.inf))
        c["ego_end"][3, 2, 3] = np.nan
        c["ego_end"][3, 3, 3] = 40.0
        # s3 / s4: sigma ratio exactly 9 (no hit) and the next float above (hit), decided by the LAST agent; compare step 23 holds 1.5, step 1 holds 1
        for b in (3, 4):
            sig[last(b), :, 23] = 1.5
            sig[last(b), :, 10] = 13.5
            sig[last(b), :, 12] = np.nextafter(F32(13.5), F32(np.inf))
        sig[last(4), :, 12] = 13.5
        sig[last(4), :, 30] = np.nextafter(F32(13.5), F32(np.inf))
        # s5: denominator 0: num > 0 is a hit (inf), 0 / 0 is not (NaN)
        sig[last(5), :, :] = 0.0
        sig[last(5), :, 16] = 2.0
        # s6: hits on steps 0, 31, 32 and 59 only -- both words, their first and last bits
        sig[last(6), :, [0, 31, 32, 59]] = 10.0
        # s7: every mode under the floor: all six slots -1
        c["scen_prob"][7] = 1e-4
        c["scen_prob"][1] = 0.5
        # the kept MODE's rows are read: a mode-dependent hit from the first agent
        for b in range(B):
            for k in range(K):
                sig[b * a, k, 40 + k] = 20.0
        out.append((f"edges_a{a}", c))
    return out


def decide_refused(seed=0):
    """forms the entry point must refuse when the tables are asked for by value: more than eight scenes; unequal agent counts"""
    rng = np.random.default_rng(seed)
    many = _decide_base(rng, 9, 2)
    ragged = _decide_base(rng, 1, 39)
    ragged["a_off"] = np.concatenate([[0], np.cumsum([1, 7, 8, 9, 14])])
    for k in ("cmp", "scen_prob", "cls", "ego_end"):
        ragged[k] = np.concatenate([ragged[k]] * 5)
    ragged["topo"][1:, :] = (np.arange(38)[:, None] * 0.37 + np.arange(K)[None, :] * 0.9).astype(F32)
    ragged["world"][[0, 7, 15, 24, 38], :, 33, 5] = 50.0
    return [("nine_scenes", many), ("ragged", ragged)]


# --------------------------------------------------------------------------------------------------------------------------------
def hairpin_lane(P):
    """three legs of unit-spaced points, all coordinates small integers (exact in float32): (q, 0) for q < 256, (q - 256, 4) for q < 512,
    (q - 512, 8) beyond.  Points q and q + 256 of the first two legs fall to the SAME thread of the 256-thread argmin."""
    q = np.arange(P)
    x = np.where(q < 256, q, np.where(q < 512, q - 256, q - 512))
    y = np.where(q < 256, 0, np.where(q < 512, 4, 8))
    return np.stack([x, y], -1).astype(F32)


def _tracks(rng, S, a, ego_xy, ego_heading, ego_speed, spread=15.0, headings=None):
    """world-frame windows [S,a,50,.]: constant-velocity tracks that END at the given ego pose (agent 0) / around it"""
    t = (np.arange(50, dtype=np.float64) - 49.0) * 0.1
    pos, ang, vel = np.zeros((S, a, 50, 2), F32), np.zeros((S, a, 50), F32), np.zeros((S, a, 50, 2), F32)
    for s_ in range(S):
        for i in range(a):
            if i == 0:
                p, h, v = np.asarray(ego_xy[s_], np.float64), F32(ego_heading[s_]), F32(ego_speed[s_])
                wob = 0.0
            else:
                p = np.asarray(ego_xy[s_], np.float64) + rng.uniform(-spread, spread, 2)
                h = F32(rng.uniform(-PI, PI) if headings is None else headings[s_][i])
                v, wob = F32(rng.uniform(0.0, 9.0)), 0.02
            hh = (h + wob * np.sin(3 * t)).astype(F32)
            hh[-1] = h
            ang[s_, i] = hh
            vel[s_, i] = np.stack([v * np.cos(hh, dtype=F32), v * np.sin(hh, dtype=F32)], -1)
            if i == 0 and float(h) == 0.0:
                vel[s_, i] = (v, 0.0)
            pos[s_, i] = (p + t[:, None] * np.array([float(v) * np.cos(float(h)), float(v) * np.sin(float(h))])).astype(F32)
            pos[s_, i, -1] = p.astype(F32)
    return pos, ang, vel


def _point_info(P):
    """per-point flags [P,12] that depend on the point's index alone (a longer lane keeps the shorter one's rows)"""
    q = np.arange(P, dtype=np.uint64)[:, None]
    return (((q * np.uint64(2654435761)) % np.uint64(2 ** 32)) >> (np.arange(12, dtype=np.uint64)[None, :] + np.uint64(8)) & np.uint64(1)).astype(F32)


def _rebase_case(rng, S, a, l, tlane, ego_xy, ego_heading, ego_speed, pad=False, late=False, headings=None, exact=None):
    pos, ang, vel = _tracks(rng, S, a, ego_xy, ego_heading, ego_speed, headings=headings)
    types = np.zeros((a, 50, 7), F32)
    types[np.arange(a), :, np.arange(a) % 7] = 1.0
    if late and a > 2:
        types[2, :7] = 0.0                                                            # an agent first seen 7 steps in
    th = rng.uniform(-PI, PI, l)
    ctr0 = np.asarray(ego_xy[0], np.float64)
    return dict(pos=pos, ang=ang, vel=vel, types=types, pad=(rng.random((S, a, 50)) < 0.8).astype(F32) if pad else None,
                lane_ctrs=(ctr0 + rng.uniform(-60, 60, (l, 2))).astype(F32), lane_vecs=np.stack([np.cos(th), np.sin(th)], -1).astype(F32),
                tlane=np.asarray(tlane, F32), tinfo=_point_info(len(tlane)), time_ahead=5.0, min_vel=0.5,
                exact=exact if exact is not None else [False] * S)


def lane_pos_scenes(P):
    """(ego x, y, heading, speed, decision exact by construction) on hairpin_lane(P); the first six do not depend on P"""
    xe = float(P - 1 - 512) if P > 512 else float(P - 1)
    ye = 8.0 if P > 512 else 0.0
    return [(-0.25, 0.5, 0.0, 0.0, True),          # nearest to point 0, travel 2.5: three steps -> 3 -> clamps up to 5
            (3.0, 0.5, 0.0, 0.0, True),            # nearest to point 3 -> 6
            (10.0, 2.0, 0.0, 2.0, True),           # equidistant (exactly 2) from points 10 and 266 = 10 + 256: ONE thread's stride; travel exactly 10
            (10.5, 1.0, 0.0, 2.0, True),           # equidistant from points 10 and 11: neighbouring threads
            (40.0, -0.5, 0.0, 0.5, True),          # ego exactly at min_vel
            (100.25, 4.5, 0.3, 3.7, False),        # second leg, inexact heading: point 356, decision clear of its thresholds
            (xe - 3.0, ye + 0.5, 0.0, 0.0, True),  # nearest to point n - 4: three steps reach n - 1 -> n - 2 -> clamps down to n - 6
            (xe + 0.25, ye - 0.5, 0.0, 2.0, True)]  # nearest to the last point: no step at all


def rebase_cases(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    short = np.stack([np.arange(12.0), np.zeros(12)], -1).astype(F32)
    # ---- headings: across the +-pi cut (thi ~ -6.2, an up to ~4 pi), exactly 0, exactly pi/2 (float32); stationary ego; ego at min_vel
    S, a = 5, 6
    hd = [[3.1, -3.1, -3.1, 3.1, -3.1 - 2 * PI, 3.1 + 2 * PI], None, None, None, None]
    hd = [h if h is not None else list(rng.uniform(-PI, PI, a)) for h in hd]
    xy = [(5.0 + 0.3 * s_, 0.4 * s_ - 0.8) for s_ in range(S)]
    out.append(("headings", _rebase_case(rng, S, a, 5, short, xy, [3.1, 0.0, F32(PI / 2), 0.3, -2.0], [4.0, 3.0, 2.0, 0.0, 0.5], late=True, headings=hd)))
    # ---- lane_pos: the ego against the ends of the target lane, argmin ties, exact travel; LDS path (P <= 1024) and global path
    for P in (12, 1024, 1025, 2000):
        if P == 12:
            sc = [(-0.25, 0.5, 0.0, 0.0, True), (3.0, 0.5, 0.0, 0.0, True), (5.5, 1.0, 0.0, 2.0, True), (8.0, -0.5, 0.0, 0.0, True), (11.25, 0.5, 0.0, 2.0, True)]
            tl = short
        else:
            sc, tl = lane_pos_scenes(P), hairpin_lane(P)
        out.append((f"lane_pos_P{P}", _rebase_case(rng, len(sc), 1, 0, tl, [(x, y) for x, y, _, _, _ in sc], [h for _, _, h, _, _ in sc],
                                                  [v for _, _, _, v, _ in sc], exact=[e for *_, e in sc])))
    # ---- wide: more agents than the workgroup has threads (257), pad given, an agent first seen late; 16 agents without lanes
    out.append(("wide_a257", _rebase_case(rng, 2, 257, 5, short, [(4.2, 0.7), (6.6, -1.1)], [0.2, -1.3], [2.2, 6.0], pad=True, late=True)))
    out.append(("a16_l0", _rebase_case(rng, 3, 16, 0, short, [(2.2, 0.7), (6.6, -1.1), (9.4, 0.2)], [0.2, 2.9, -1.3], [2.2, 0.1, 6.0], pad=True, late=True)))
    # ---- far: 5 km from the origin, agents metres apart
    far = (np.stack([np.arange(12.0), np.zeros(12)], -1) @ np.array([[0.6, 0.8], [-0.8, 0.6]]) + (5000.0, -5000.0)).astype(F32)
    out.append(("far", _rebase_case(rng, 2, 6, 5, far, [(5003.1, -4996.2), (5004.4, -4993.9)], [0.9, 1.0], [3.0, 5.0], late=True)))
    return out
