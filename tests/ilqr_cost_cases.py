"""Cost trees that take the tree-iLQR's planner-mode cost to the places where its device texts can leave the oracle: crowded window cells,
grids other than 0.4 m x 256 x 256, exact rounding ties, the eight border placements, far origins and degenerate inputs.  The trees are built
directly as the arrays ``oracle.ilqr.flatten`` returns; everything is deterministic from ``numpy.random.default_rng(seed)``.  No GPU, no
test in here: tests/test_ilqr_cost_cases_host.py proves on the oracle alone what each family can catch, tests/test_gpu_ilqr_cost_edges.py
runs the kernels on them.

A case is a dict: family, name, cfg (``IlqrCfg``), flat (parent, prob, mean, cov), x0 [6], lane [P, 2], tv, M, and ``queries`` -- (node [Q],
x [Q, 6], u [Q, 2]) extra evaluation points of the family -- plus ``solve`` (whether the family's solves run on it).

Queries at which the oracle itself returns NaN would be named in ``NAN_QUERIES`` (family -> case name -> query indices) and left out of the
asserted sets; there are none: every family's oracle outputs are finite (test_oracle_is_finite_on_every_asserted_output)."""
import numpy as np

from oracle import ilqr as oi

NAN_QUERIES = {}

IL_RMARGIN = 3.0          # the line search trusts a node's list for candidates within this distance of the nominal state [m]
IL_REL = 15               # records per list; more agents in reach = overflow, the node walks every agent
GRIDS = [(0.4, 256, 256), (0.25, 64, 48), (0.8, 128, 128), (1.0, 103, 77), (0.4, 3, 3)]


def list_reach(res):
    """the window reach the relevant-agent list needs beyond sigma + offset + IL_RMARGIN: 1.5 cells along both axes"""
    return 1.5 * np.sqrt(2.0) * res


def cfg_for(res=0.4, W=256, H=256, max_iter=6):
    c = oi.default_cfg(max_iter=max_iter)
    c.grid_res, c.grid_w, c.grid_h = res, W, H
    return c


def copy_cfg(cfg, **kw):
    c = type(cfg).from_buffer_copy(cfg)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ---- trees -----------------------------------------------------------------------------------------------------------------------------
def chain(M=25):
    return np.arange(-1, M - 1, dtype=np.int32), np.ones(M, np.float32)


def branching(trunk=8, blen=9, probs=(0.5639, 0.3421, 0.094)):
    """a trunk and three branches: three leaves, trunk + 3 blen <= 40 nodes, children after their parents"""
    parent, prob = list(range(-1, trunk - 1)), [1.0] * trunk
    for p in probs:
        for k in range(blen):
            parent.append(trunk - 1 if k == 0 else len(parent) - 1)
            prob.append(p)
    return np.asarray(parent, np.int32), np.asarray(prob, np.float32)


def _depth(parent):
    d = np.zeros(len(parent), int)
    for i in range(1, len(parent)):
        d[i] = d[parent[i]] + 1
    return d


def _branch_id(parent):
    """0 on the trunk, 1.. per branch (by the first node that is not its parent's first child)"""
    b, seen, nxt = np.zeros(len(parent), int), set(), 0
    for i in range(1, len(parent)):
        p = int(parent[i])
        if p in seen:
            nxt += 1
            b[i] = nxt
        else:
            b[i] = b[p]
            seen.add(p)
    return b


def zero_control_rollout(cfg, parent, x0):
    """the bicycle model under zero controls (placement of agents only: numpy's sin / cos / tan)"""
    M, dt, wb = len(parent), cfg.dt, cfg.wheelbase
    xs = np.zeros((M, 6))
    for c in range(M):
        p = x0 if parent[c] < 0 else xs[parent[c]]
        xs[c] = [p[0] + p[2] * np.cos(p[3]) * dt, p[1] + p[2] * np.sin(p[3]) * dt, p[2] + p[4] * dt, p[3] + p[2] / wb * np.tan(p[5]) * dt,
                 p[4], p[5]]
    return xs


def _scene(rng, cfg, parent, prob, x0, n_agents, band, sigma=(0.31, 1.47), clusters=(), ring=0, ring_gap=(0.0, 1.2), lane_dy=0.0, drift=1.0):
    """agents scattered in a band (length, width) [m] round the ego's zero-control path, ``clusters``: (node, count, radius) groups that stand
    together on the path, ``ring``: that many agents aimed just outside the list radius of a path node on the side the lane pulls to"""
    M, A = len(parent), n_agents
    path = zero_control_rollout(cfg, parent, x0)
    dep, br = _depth(parent), _branch_id(parent)
    t = (dep + 1) * cfg.dt
    mean, cov = np.zeros((M, A, 2)), np.zeros((M, A))
    mean[:, 0] = path[:, :2] + 0.05 * rng.standard_normal((M, 2))                 # the ego's own prediction
    cov[:, 0] = rng.uniform(0.23, 0.61) + 0.017 * dep
    e = 1
    base, vel = np.zeros((A, 2)), drift * rng.uniform(-1.0, 1.0, (A, 2))
    sg = rng.uniform(sigma[0], sigma[1], A)
    for node, count, radius in clusters:
        for _ in range(count):
            if e < A:
                base[e] = path[node, :2] + radius * rng.uniform(-1.0, 1.0, 2)
                vel[e] *= 0.1
                e += 1
    for _ in range(ring):
        if e < A:
            node = int(rng.integers(M // 2, M))
            ang = np.pi / 2 * np.sign(lane_dy if lane_dy else 1.0) + rng.uniform(-0.7, 0.7)
            r = (sg[e] + cfg.w_exo_cov_offset) + IL_RMARGIN + rng.uniform(*ring_gap)
            base[e] = path[node, :2] + r * np.array([np.cos(ang), np.sin(ang)])
            vel[e] = 0.0
            e += 1
    n_rest = A - e
    base[e:] = x0[:2] + np.stack([rng.uniform(-0.125, 0.875, n_rest) * band[0], rng.uniform(-0.5, 0.5, n_rest) * band[1]], 1)
    for a in range(1, A):
        mean[:, a] = base[a] + vel[a] * t[:, None] + 0.3 * br[:, None] * vel[a][::-1]       # the branches see the agents apart
        cov[:, a] = sg[a] + 0.011 * dep * rng.uniform(0.0, 1.0)
    P = 40
    lx = np.linspace(x0[0] - 0.4 * band[0] - 5.0, x0[0] + 1.2 * band[0] + 5.0, P)
    lane = np.stack([lx, x0[1] + lane_dy + 0.02 * band[1] * np.sin((lx - x0[0]) / (0.5 * band[0] + 1.0))], 1)
    flat = dict(parent=parent, prob=prob, mean=np.ascontiguousarray(mean, np.float32), cov=np.ascontiguousarray(cov, np.float32))
    return flat, lane


def _case(family, name, cfg, flat, x0, lane, tv, queries=None, solve=True):
    M = len(flat["parent"])
    if queries is None:
        queries = (np.zeros(0, np.int32), np.zeros((0, 6)), np.zeros((0, 2)))
    return dict(family=family, name=name, cfg=cfg, flat=flat, x0=np.asarray(x0, np.float64), lane=lane, tv=float(tv), M=M, queries=queries, solve=solve)


def _queries_at(rng, M, x0, pts):
    """one query per point: node q % M, the start state's other components, a random control"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    Q = len(pts)
    x = np.tile(np.asarray(x0, np.float64), (Q, 1))
    x[:, :2] = pts
    x[:, 2:] += rng.normal(size=(Q, 4)) * np.array([0.5, 0.05, 0.5, 0.05])
    return (np.arange(Q) % M).astype(np.int32), x, rng.normal(size=(Q, 2))


X0 = np.array([0.3, 0.2, 4.0, 0.04, 0.1, 0.01])


# ---- families --------------------------------------------------------------------------------------------------------------------------
def crowd():
    """9, 17, 40 and 128 agents round the ego path; groups of 8 and 9 on one spot; sigmas are not round numbers"""
    out = []
    for n, tree, seed, clusters, band in ((9, "chain", 3, ((10, 8, 0.6),), (24.0, 10.0)), (17, "branch", 4, ((6, 9, 0.5), (14, 3, 0.8)), (24.0, 10.0)),
                                          (40, "chain", 5, ((12, 6, 1.5),), (26.0, 9.0)), (40, "branch", 6, (), (24.0, 8.0)),
                                          (128, "chain", 7, (), (30.0, 14.0))):
        rng = np.random.default_rng(1000 + seed)
        parent, prob = chain() if tree == "chain" else branching()
        cfg = cfg_for()
        flat, lane = _scene(rng, cfg, parent, prob, X0, n, band, clusters=clusters, lane_dy=0.4)
        out.append(_case("crowd", f"a{n}_{tree}", cfg, flat, X0, lane, 4.0))
    return out


GRID_SEEDS = {(0.4, 256, 256): 0, (0.25, 64, 48): 12, (0.8, 128, 128): 5, (1.0, 103, 77): 10, (0.4, 3, 3): 15}
GRID_LANE_DY = {(0.4, 256, 256): 13.0, (0.25, 64, 48): 2.0, (0.8, 128, 128): 5.0, (1.0, 103, 77): 5.0, (0.4, 3, 3): 0.3}

# (agent slot, node, x, y, sigma) of the aimed agents, found once on the oracle's iterates (tests/test_ilqr_cost_cases_host.py checks them)
GRID_AIMED = {(0.4, 256, 256): [(-1, 24, 22.9805850982666, 8.896659851074219, 0.83)],
              (0.8, 128, 128): [(-1, 13, 4.740302085876465, -1.090232014656067, 0.83)],
              (1.0, 103, 77): [(-1, 31, 7.355005741119385, -5.7209906578063965, 0.83)]}


def grids(only=None):
    """every grid with use_exo = 1 and a crowd-like band scaled to the field; the lane lies beside the start, so the first iterations move the
    far nodes by metres, and a third of the agents stand in the ring just outside the list radius on that side"""
    out = []
    for res, W, H in GRIDS:
        if only is not None and (res, W, H) != only:
            continue
        rng = np.random.default_rng(2000 + GRID_SEEDS[(res, W, H)])
        fw, fh = (W - 1) * res, (H - 1) * res
        small = fw < 30.0
        x0 = X0.copy()
        if small:
            x0[2] = 1.0                                       # 5 m in 25 nodes: the path stays on a field of 15.75 m x 11.75 m
        tv = float(x0[2])
        cfg = cfg_for(res, W, H)
        parent, prob = branching() if (res, W, H) == (1.0, 103, 77) else chain()
        band = (min(32.0, 1.2 * fw), min(18.0, 1.2 * fh)) if fw > 2.0 else (6.0, 6.0)
        sigma = (0.31, 1.47) if not small or fw < 2.0 else (0.12, 0.59)
        lane_dy = GRID_LANE_DY[(res, W, H)]
        flat, lane = _scene(rng, cfg, parent, prob, x0, 40, band, sigma=sigma, ring=13, ring_gap=(0.0, 1.5 * res + 0.6), lane_dy=lane_dy, drift=0.3)
        # the last two agents are aimed: each stands, at ONE node, in the ring between the list radius a reach of 1.0 m (0.0 m on the 0.4 m
        # grid) gives and the one 1.5 sqrt(2) res gives, on the ray from an oracle iterate through a window cell of the next one; parked
        # 400 m away at every other node
        flat["mean"][:, -2:] = (x0[:2] + 400.0).astype(np.float32)
        for slot, node, ax, ay, sg in GRID_AIMED.get((res, W, H), ()):
            flat["mean"][node, slot] = (ax, ay)
            flat["cov"][node, slot] = sg
        out.append(_case("grids", f"res{res}_{W}x{H}", cfg, flat, x0, lane, tv))
    return out


def tie_points():
    """the 0.25 m grid of 64 x 48 about x0 = (1.0, 0.5): field_offset = (-6.875, -5.375) is dyadic, so off + (k + 0.5) res is exact and
    (p - off) / res is exactly k + 0.5 -> dict(off, res, W, H, ties [(px, py, kx, ky)], borders [(px, py, xi, yi)], outside [(px, py)])"""
    res, W, H = 0.25, 64, 48
    x0 = np.array([1.0, 0.5])
    off = x0 - 0.5 * np.array([(W - 1) * res, (H - 1) * res])
    ties = []
    for kx, ky in ((10, 7), (11, 8), (10, 8), (11, 7), (0, 0), (1, 21), (W - 2, H - 2), (W - 3, 1), (31, 23), (32, 24)):
        ties.append((off[0] + (kx + 0.5) * res, off[1] + (ky + 0.5) * res, kx, ky))
    ties.append((off[0] + 20.5 * res, off[1] + 9.3 * res, 20, None))           # a tie along one axis only
    ties.append((off[0] + 20.2 * res, off[1] + 15.5 * res, None, 15))
    borders = []
    for xi in (0, 17, W - 1):
        for yi in (0, 29, H - 1):
            for dx, dy in ((0.0, 0.0), (0.37, -0.21), (-0.44, 0.48)):
                borders.append((off[0] + (xi + dx) * res, off[1] + (yi + dy) * res, xi, yi))
    fs = np.array([(W - 1) * res, (H - 1) * res])
    outside = [(off[0] - 3.3, x0[1]), (off[0] + fs[0] + 2.7, x0[1] + 1.1), (x0[0], off[1] - 1.9), (x0[0] - 2.2, off[1] + fs[1] + 4.6),
               (off[0] - 0.13, off[1] - 0.12), (off[0] + fs[0] + 0.126, off[1] + fs[1] + 0.3), (off[0] - 40.0, off[1] + fs[1] + 55.0),
               (off[0] + fs[0] + 0.125, x0[1])]
    return dict(off=off, res=res, W=W, H=H, ties=ties, borders=borders, outside=outside)


def ties_borders():
    tp = tie_points()
    rng = np.random.default_rng(3001)
    res, W, H, off = tp["res"], tp["W"], tp["H"], tp["off"]
    x0 = np.array([1.0, 0.5, 1.0, 0.04, 0.1, 0.01])
    cfg = cfg_for(res, W, H)
    parent, prob = chain()
    flat, lane = _scene(rng, cfg, parent, prob, x0, 24, (18.0, 14.0), sigma=(0.12, 0.59), lane_dy=0.7, drift=0.2)
    # agents near the border cells: the corners, the edge centres, and two on the tie cells
    fs = np.array([(W - 1) * res, (H - 1) * res])
    spots = [off + fs * np.array(f) for f in ((0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0), (0.5, 1), (0, 0.5), (1, 0.5), (0.27, 0.6))]
    spots += [np.array([off[0] + 10.5 * res, off[1] + 7.5 * res]), np.array([off[0] + 31.5 * res, off[1] + 23.5 * res])]
    mean = flat["mean"].astype(np.float64)
    for a, s in enumerate(spots):
        mean[:, 1 + a] = s + 0.4 * rng.uniform(-1.0, 1.0, 2) + 0.02 * rng.standard_normal((len(parent), 2))
    flat["mean"] = np.ascontiguousarray(mean, np.float32)
    flat["cov"][:, 1:1 + len(spots)] -= np.float32(2.0)               # sigma + offset of 0.6 .. 1.1 m: a few cells of 0.25 m
    pts = [(p[0], p[1]) for p in tp["ties"]] + [(p[0], p[1]) for p in tp["borders"]] + list(tp["outside"])
    return [_case("ties_borders", "res0.25_64x48", cfg, flat, x0, lane, 1.0, queries=_queries_at(rng, len(parent), x0, pts), solve=False)]


def far():
    """the 0.4 m grid with x0 at (4 000, -3 000): float32 agent positions have an ulp of 0.24 mm there"""
    rng = np.random.default_rng(4001)
    x0 = X0.copy()
    x0[:2] = [4000.0, -3000.0]
    cfg = cfg_for()
    parent, prob = chain()
    flat, lane = _scene(rng, cfg, parent, prob, x0, 40, (26.0, 9.0), clusters=((12, 6, 1.5),), lane_dy=0.4)
    return [_case("far", "x0_4000_-3000", cfg, flat, x0, lane, 4.0)]


def bound_states(cfg, x0):
    """states exactly on, one ulp below and one ulp above each finite bound -> [Q, 6]"""
    xs = []
    for arr in (cfg.state_lower, cfg.state_upper):
        for k in range(6):
            b = float(arr[k])
            if np.isfinite(b):
                for v in (b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)):
                    x = np.array(x0, np.float64)
                    x[k] = v
                    xs.append(x)
    return np.array(xs)


def degenerate():
    """evaluation only: sigma + offset (a float32 sum) negative, zero and 50 m; node probabilities 0 and 1e-30; w_exo_cost_offset = 0; states
    on and one ulp either side of every bound"""
    out = []
    rng = np.random.default_rng(5001)
    parent, prob = chain()
    cfg = cfg_for()
    flat, lane = _scene(rng, cfg, parent, prob, X0, 17, (24.0, 10.0), clusters=((8, 4, 1.0),), lane_dy=0.4)
    off = np.float32(cfg.w_exo_cov_offset)
    cov0 = flat["cov"].copy()
    cov = flat["cov"]
    cov[:, 1] = np.float32(-3.1)
    cov[:, 2] = -off
    cov[:, 3] = np.float32(50.0) - off
    cov[:, 4] = np.nextafter(-off, np.float32(0.0))                 # the smallest positive sum
    cov[5:, 0] = -np.float32(cfg.w_ego_cov_offset)                  # the ego's own sum zero on most nodes, negative on some
    cov[15:, 0] = np.float32(-2.2)
    assert float(cov[0, 1] + off) < 0 and float(cov[0, 2] + off) == 0 and float(cov[0, 3] + off) == 50.0
    bx = bound_states(cfg, X0)
    q = ((np.arange(len(bx)) % len(parent)).astype(np.int32), bx, rng.normal(size=(len(bx), 2)))
    out.append(_case("degenerate", "sigma_sums", cfg, flat, X0, lane, 4.0, queries=q, solve=False))
    flat2 = dict(flat, prob=prob.copy(), cov=cov0)
    flat2["prob"][3::4] = np.float32(0.0)
    flat2["prob"][1::4] = np.float32(1e-30)
    out.append(_case("degenerate", "prob_0_1e-30", cfg, flat2, X0, lane, 4.0, queries=q, solve=False))
    cfg3 = copy_cfg(cfg, w_exo_cost_offset=0.0)
    out.append(_case("degenerate", "cost_offset_0", cfg3, dict(flat2, prob=prob.copy()), X0, lane, 4.0, queries=q, solve=False))
    return out


FAMILIES = dict(crowd=crowd, grids=grids, ties_borders=ties_borders, far=far, degenerate=degenerate)
_built = {}


def family(name):
    if name not in _built:
        _built[name] = FAMILIES[name]()
    return _built[name]


def all_cases():
    return [c for f in FAMILIES for c in family(f)]


def case_ids():
    """(family, case name) of every case, without building the oracle's results"""
    return [(c["family"], c["name"]) for c in all_cases()]


def get(fam, name):
    return next(c for c in family(fam) if c["name"] == name)


# ---- the oracle's results, computed once per case and left unchanged ----------------------------------------------------------------------
_oracle = {}


def oracle_of(c):
    """warm: the lane-only fit; full: the full fit from the warm fit's controls (both with traces); sol3: the three-iteration solve from zero
    controls whose states the evaluation points are built around"""
    key = (c["family"], c["name"])
    if key not in _oracle:
        cfg = c["cfg"]
        cfg_w = copy_cfg(cfg, w_ego=0.0, w_exo=0.0)
        w = oi.solve(cfg_w, c["flat"], c["x0"], c["lane"], c["tv"], 0, trace=True)
        f = oi.solve(cfg, c["flat"], c["x0"], c["lane"], c["tv"], 1, us_init=w["us"], trace=True)
        s3 = oi.solve(copy_cfg(cfg, max_iter=3), c["flat"], c["x0"], c["lane"], c["tv"], 1)
        _oracle[key] = dict(cfg_w=cfg_w, warm=w, full=f, sol3=s3)
    return _oracle[key]


_eval = {}


def eval_points(c):
    """(node [Q], x [Q, 6], u [Q, 2], want): every node at the three-iteration solve's state plus the perturbation
    test_tree_cost_derivatives_match_oracle uses, then the family's own queries; want = the oracle's derivatives there"""
    key = (c["family"], c["name"])
    if key not in _eval:
        M = c["M"]
        sol = oracle_of(c)["sol3"]
        rng = np.random.default_rng(1)
        xs = sol["xs"] + rng.normal(size=(M, 6)) * np.array([0.7, 0.7, 2.0, 0.1, 3.0, 0.3])
        us = sol["us"] + rng.normal(size=(M, 2))
        qn, qx, qu = c["queries"]
        node = np.concatenate([np.arange(M, dtype=np.int32), qn])
        x, u = np.concatenate([xs, qx]), np.concatenate([us, qu])
        want = {k: [] for k in ("l", "l_x", "l_u", "l_xx", "l_uu")}
        # the oracle evaluates node i at (xs[i], us[i]): one pass per round of at most M queries
        for r0 in range(0, len(node), M):
            idx = np.arange(r0, min(r0 + M, len(node)))
            if r0 == 0:
                fx, fu = x[:M], u[:M]
            else:
                fx, fu = np.tile(c["x0"], (M, 1)), np.zeros((M, 2))
                assert len(set(node[idx].tolist())) == len(idx)
                fx[node[idx]], fu[node[idx]] = x[idx], u[idx]
            d = oi.node_derivs(c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], 1, fx, fu)
            for k in want:
                want[k].append(d[k][node[idx]])
        _eval[key] = (node, x, u, {k: np.concatenate(v) for k, v in want.items()})
    return _eval[key]


# ---- numpy restatements ----------------------------------------------------------------------------------------------------------------
def grid_of(c):
    """(gx [W], gy [H], off [2]) as oracle/ilqr_ref.c make_grid builds them"""
    cfg = c["cfg"]
    W, H, res = cfg.grid_w, cfg.grid_h, cfg.grid_res
    fsx, fsy = (W - 1) * res, (H - 1) * res
    off = np.array([c["x0"][0] - 0.5 * fsx, c["x0"][1] - 0.5 * fsy])
    gx, gy = np.arange(W) * (fsx / (W - 1)) + 0.0, np.arange(H) * (fsy / (H - 1)) + 0.0
    gx[-1], gy[-1] = fsx, fsy
    return gx + off[0], gy + off[1], off


def cell_of(c, px, py):
    """the cell a query rounds to (half to even, clamped): (xi, yi)"""
    cfg = c["cfg"]
    _, _, off = grid_of(c)
    xi = int(np.clip(np.rint((px - off[0]) / cfg.grid_res), 0, cfg.grid_w - 1))
    yi = int(np.clip(np.rint((py - off[1]) / cfg.grid_res), 0, cfg.grid_h - 1))
    return xi, yi


def placement(c, xi, yi):
    """which of smooth_grid's nine branches a cell takes: (0 | 1 | 2 for first | interior | last column, likewise the row)"""
    cfg = c["cfg"]
    return (0 if xi == 0 else 2 if xi == cfg.grid_w - 1 else 1, 0 if yi == 0 else 2 if yi == cfg.grid_h - 1 else 1)


def exo_terms(c, i, cx, cy):
    """max(sigma_e + offset - d, 0) (+ the cost offset where positive) of node i's exo agents e = 1 .. at the point (cx, cy), in float64 as
    the oracle computes them (sigma + offset is a float32 sum) -> [A - 1]"""
    cfg, flat = c["cfg"], c["flat"]
    ec = (flat["cov"][i, 1:] + np.float32(cfg.w_exo_cov_offset)).astype(np.float64)
    m = flat["mean"][i, 1:].astype(np.float64)
    dx, dy = cx - m[:, 0], cy - m[:, 1]
    v = ec - np.sqrt(dx * dx + dy * dy)
    v = np.where(v > 0.0, v, 0.0)
    return np.where(v > 0.0, v + cfg.w_exo_cost_offset, v)


def sum_ascending(t):
    s = 0.0
    for v in t:
        s += float(v)
    return s


def sum_strided7(t):
    """agent e goes to slot (e - 1) % 7; the seven partial sums are then added in slot order"""
    part = [0.0] * 7
    for j, v in enumerate(t):
        part[j % 7] += float(v)
    s = 0.0
    for p in part:
        s += p
    return s


def window_cells(c, px, py):
    """the interior 3 x 3 window about the query's cell, or None where the window is not the plain one -> [(sx, sy)]"""
    xi, yi = cell_of(c, px, py)
    if placement(c, xi, yi) != (1, 1):
        return None
    return [(xi - 1 + cc, yi - 1 + r) for r in range(3) for cc in range(3)]


def list_members(c, i, nx, ny, reach):
    """the exo agents (0-based among e = 1 ..) the list of node i keeps about the nominal position (nx, ny)"""
    cfg, flat = c["cfg"], c["flat"]
    ec = (flat["cov"][i, 1:] + np.float32(cfg.w_exo_cov_offset)).astype(np.float64)
    m = flat["mean"][i, 1:].astype(np.float64)
    dx, dy = m[:, 0] - nx, m[:, 1] - ny
    rr = ec + IL_RMARGIN + reach
    return dx * dx + dy * dy < rr * rr


def list_misses(c, nominal, query, reach):
    """(node, agent) pairs where the line search would trust node's list -- not overflowed, the query within IL_RMARGIN of the nominal state
    and its window inside the grid -- while an agent outside the list costs more than 0 at one of the query's nine window cells"""
    cfg = c["cfg"]
    gx, gy, off = grid_of(c)
    res, W, H = cfg.grid_res, cfg.grid_w, cfg.grid_h
    in_x0, in_x1 = off[0] + 1.5 * res, off[0] + (W - 2.5) * res
    in_y0, in_y1 = off[1] + 1.5 * res, off[1] + (H - 2.5) * res
    out = []
    for i in range(c["M"]):
        nx, ny, qx, qy = nominal[i, 0], nominal[i, 1], query[i, 0], query[i, 1]
        keep = list_members(c, i, nx, ny, reach)
        if keep.sum() > IL_REL:
            continue
        if not (in_x0 < qx < in_x1 and in_y0 < qy < in_y1 and (qx - nx) ** 2 + (qy - ny) ** 2 < IL_RMARGIN ** 2):
            continue
        cells = window_cells(c, qx, qy)
        hit = np.zeros(len(keep), bool)
        for sx, sy in cells:
            hit |= exo_terms(c, i, gx[sx], gy[sy]) > 0.0
        for e in np.nonzero(hit & ~keep)[0]:
            out.append((i, int(e) + 1))
    return out
