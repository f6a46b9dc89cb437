"""GPU: mind_ilqr_score_trees / HipPredictor.ilqr_score / iLQR.score / multi-start iLQR.fit -- rollout and TreeCost of candidate control
trees without optimisation (k_ilqr_score).  Every output has a bit-exact yardstick: the states are what the solver's line search stores
for the same controls, the node costs are mind_cost_eval's and the C oracle's, the sum is what a fit of one iteration reports as J."""
import ctypes as C
import os

import numpy as np
import pytest

from mind_amd import _lib
from mind_amd.planners.basic.tree import Node, Tree
from mind_amd.planners.ilqr.cost import TreeCost
from mind_amd.planners.ilqr.dynamics import BicycleDynamics
from mind_amd.planners.ilqr.potential import ControlPotential, PotentialField, StateConstraint, StatePotential
from mind_amd.planners.ilqr.solver import iLQR
from mind_amd.predictor import IlqrCall
from mind_amd.synth import scripted_scenario_tree
from oracle import ilqr as oi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("lead", 4), ("branch3", 12), ("deep", 4), ("straight", 1)]
_cases = {}


def _case(hp, kind, a, use_exo=1):
    """the scripted tree, the controls of a six-iteration solve on it and three candidates -- those controls, zeros, those controls plus
    noise of scale 1 -- scored in one call; computed once per (kind, a, use_exo)"""
    key = (kind, a, use_exo)
    if key not in _cases:
        sst = scripted_scenario_tree(kind, a)
        cfg = oi.default_cfg(max_iter=6)
        flat = oi.flatten(sst["nodes"])
        x0 = oi.init_state(sst["state"], sst["ctrl"])
        lane, tv = sst["target_lane"], sst["target_vel"]
        xs, us, _ = hp.ilqr_solve(cfg, [flat], x0, lane, tv, use_exo)
        M = len(flat["parent"])
        rng = np.random.default_rng(17)
        cands = np.stack([us[0], np.zeros((M, 2)), us[0] + rng.normal(size=(M, 2))])
        sxs, sL, sJ = hp.ilqr_score(cfg, [flat], x0, lane, tv, use_exo, cands)
        _cases[key] = dict(cfg=cfg, flat=flat, x0=x0, lane=lane, tv=tv, M=M, xs_star=xs[0], us_star=us[0], cands=cands, xs=sxs[0], L=sL[0], J=sJ[:, 0],
                           use_exo=use_exo)
    return _cases[key]


def _check_node_costs(hp, c):
    for k in range(len(c["cands"])):
        got = hp.cost_eval(c["cfg"], np.arange(c["M"]), c["xs"][k], c["cands"][k], c["flat"], x0=c["x0"], lane=c["lane"], target_vel=c["tv"],
                           use_exo=c["use_exo"])["l"]
        want = oi.node_derivs(c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], c["use_exo"], c["xs"][k], c["cands"][k])["l"]
        assert np.array_equal(c["L"][k], got), (k, np.abs(c["L"][k] - got).max())
        assert np.array_equal(c["L"][k], want), (k, np.abs(c["L"][k] - want).max())


def _check_sums(hp, cfg, flat, x0, lane, tv, use_exo, cands, J):
    cfg1 = oi.default_cfg(max_iter=1)                          # (every case here runs the default weights)
    for k, us_c in enumerate(cands):
        one = hp.ilqr_solve(cfg1, [flat], x0, lane, tv, use_exo, us_init=[us_c])[2][0]["J"]
        ref = oi.solve(cfg1, flat, x0, lane, tv, use_exo, us_init=us_c)["J"]
        print(f"candidate {k}: J {J[k]!r} one-iteration solve {one!r} oracle {ref!r}")
        assert J[k] == one, (k, J[k], one)
        assert abs(J[k] - ref) < 1e-8 * max(1.0, abs(J[k])), (k, J[k], ref)


@pytest.mark.parametrize("kind,a", CASES)
def test_states_are_the_solvers_bits(kind, a, hip_predictor):
    """the line search stores u and then f(x_parent, u) (il_rollout_packed): the rollout of the solver's own controls is the solver's states"""
    c = _case(hip_predictor, kind, a)
    xs, L, J = hip_predictor.ilqr_score(c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"], 1, c["us_star"][None])
    assert xs[0].shape == (1, c["M"], 6) and L[0].shape == (1, c["M"]) and J.shape == (1, 1)
    assert np.array_equal(xs[0][0], c["xs_star"]), np.abs(xs[0][0] - c["xs_star"]).max()
    assert np.array_equal(c["xs"][0], c["xs_star"])          # ... and as the first of three candidates


@pytest.mark.parametrize("kind,a", CASES)
def test_node_costs_are_cost_evals_bits_and_the_oracles(kind, a, hip_predictor):
    c = _case(hip_predictor, kind, a)
    if (kind, a) == ("branch3", 12):
        assert c["M"] > 64 and c["flat"]["mean"].shape[1] > 8      # more nodes than lanes, more agents than il_field's seven slots
    assert np.all(np.isfinite(c["xs"])) and np.all(np.isfinite(c["L"]))
    _check_node_costs(hip_predictor, c)


@pytest.mark.parametrize("kind,a", CASES)
def test_sum_is_what_a_one_iteration_solve_reports(kind, a, hip_predictor):
    c = _case(hip_predictor, kind, a)
    assert 8 <= c["M"] <= 128                                  # numpy's eight-accumulator branch
    _check_sums(hip_predictor, c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], 1, c["cands"], c["J"])


@pytest.mark.parametrize("keep", [1, 3])
def test_sum_of_a_tiny_tree(keep, hip_predictor):
    """one- and two-node trees (as test_tiny_trees_and_ego_only builds them): numpy's sequential branch, M < 8"""
    sst = scripted_scenario_tree("straight", 2)
    cfg = oi.default_cfg(max_iter=6)
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    key, parent, data = sst["nodes"][0]
    flat = oi.flatten([(key, parent, [data[0], data[1][:, :keep], data[2][:, :keep], data[3]])])
    M = len(flat["parent"])
    assert M == (keep + 1) // 2 < 8
    cands = np.stack([np.zeros((M, 2)), np.random.default_rng(5).normal(size=(M, 2))])
    xs, L, J = hip_predictor.ilqr_score(cfg, [flat], x0, sst["target_lane"], sst["target_vel"], 1, cands)
    _check_sums(hip_predictor, cfg, flat, x0, sst["target_lane"], sst["target_vel"], 1, cands, J[:, 0])


def test_sum_of_a_tree_beyond_128_nodes(hip_predictor):
    """numpy's pairwise branch: the smallest scenario tree of the scripted 6-ary AIME tree (as test_wide_cost_tree_matches_oracle) above 128 nodes"""
    from test_aime_host import _full_tree_run
    g, trees = _full_tree_run(True)
    listed = [[(k, n.parent_key, n.data) for k, n in t.nodes.items()] for t in trees]
    nodes = min((nd for nd in listed if len(oi.flatten(nd)["parent"]) > 128), key=lambda nd: len(oi.flatten(nd)["parent"]))
    flat = oi.flatten(nodes)
    M = len(flat["parent"])
    assert 128 < M < 256
    lane = np.asarray(g.target_lane[::2], np.float64)
    d0 = nodes[0][2][1][0, 0]
    x0 = oi.init_state(np.array([float(d0[0]), float(d0[1]), 4.0, 0.0]), np.array([0.0, 0.0]))
    cfg = oi.default_cfg(max_iter=3)
    us = hip_predictor.ilqr_solve(cfg, [flat], x0, lane, 4.0, 1)[1][0]
    cands = np.stack([us, np.zeros((M, 2)), us + np.random.default_rng(3).normal(size=(M, 2))])
    xs, L, J = hip_predictor.ilqr_score(cfg, [flat], x0, lane, 4.0, 1, cands)
    _check_sums(hip_predictor, cfg, flat, x0, lane, 4.0, 1, cands, J[:, 0])
    for k in range(3):
        assert np.array_equal(L[0][k], oi.node_derivs(cfg, flat, x0, lane, 4.0, 1, xs[0][k], cands[k])["l"]), k


def test_batching_changes_nothing(hip_predictor):
    """three trees of different size in one call, 65 candidates (one more than a wave has lanes): every (candidate, tree) slice equals the
    call with that tree and that candidate alone; so does J without the optional outputs"""
    a, nc = 4, 65
    base = _case(hip_predictor, "lead", a)
    cfg, x0, lane, tv = base["cfg"], base["x0"], base["lane"], base["tv"]
    flats = [oi.flatten(scripted_scenario_tree(kind, a)["nodes"]) for kind in ("lead", "straight", "branch3")]
    Ms = [len(f["parent"]) for f in flats]
    assert len(set(Ms)) == 3
    rng = np.random.default_rng(23)
    per_tree = []
    for M in Ms:                                                # the first tree's controls, padded or cut to this tree, + noise (candidate 0: none)
        u0 = np.zeros((M, 2))
        u0[:min(M, Ms[0])] = base["us_star"][:M]
        noise = rng.normal(size=(nc, M, 2)) * np.array([1.0, 0.2])
        noise[0] = 0.0
        per_tree.append(u0[None] + noise)
    xs, L, J = hip_predictor.ilqr_score(cfg, flats, x0, lane, tv, 1, per_tree)
    assert J.shape == (nc, 3) and [x.shape for x in xs] == [(nc, M, 6) for M in Ms] and [l.shape for l in L] == [(nc, M) for M in Ms]
    assert np.all(np.isfinite(J))
    for t, flat in enumerate(flats):
        for c in range(nc):
            x1, l1, j1 = hip_predictor.ilqr_score(cfg, [flat], x0, lane, tv, 1, per_tree[t][c:c + 1])
            assert np.array_equal(xs[t][c], x1[0][0]) and np.array_equal(L[t][c], l1[0][0]) and J[c, t] == j1[0, 0], (t, c)
    # the whole call again as one [C, sum M, 2] array, without the optional outputs
    flat_cands = np.concatenate(per_tree, axis=1)
    for want_xs, want_L in ((False, False), (True, False), (False, True)):
        x2, l2, j2 = hip_predictor.ilqr_score(cfg, flats, x0, lane, tv, 1, flat_cands, want_xs=want_xs, want_L=want_L)
        assert (x2 is None) == (not want_xs) and (l2 is None) == (not want_L) and np.array_equal(j2, J)
    j1 = hip_predictor.ilqr_score(cfg, flats, x0, lane, tv, 1, flat_cands[:1], want_xs=False, want_L=False)[2]
    assert np.array_equal(j1, J[:1])
    # every size of the candidate blocks: a full wave of 64 lanes + a block of one candidate behind it, down to a candidate per workgroup
    try:
        for block in (64, 32, 7, 1):
            hip_predictor.set_tuning("ilqr_score_block", block)
            x3, l3, j3 = hip_predictor.ilqr_score(cfg, flats, x0, lane, tv, 1, flat_cands)
            assert np.array_equal(j3, J) and all(np.array_equal(x3[t], xs[t]) and np.array_equal(l3[t], L[t]) for t in range(3)), block
    finally:
        hip_predictor.set_tuning("ilqr_score_block", 0)
    assert np.array_equal(xs[0][0], base["xs_star"])            # candidate 0 of the first tree is the solver's own trajectory


def test_lane_term_only(hip_predictor):
    """use_exo = 0, the warm-start tree: node costs and sums as above"""
    c = _case(hip_predictor, "lead", 4, use_exo=0)
    assert np.array_equal(c["xs"][0], c["xs_star"])
    _check_node_costs(hip_predictor, c)
    _check_sums(hip_predictor, c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], 0, c["cands"], c["J"])


def _reference_style_cost_tree(cfg, sst, use_exo):
    """the cost tree as trajectory_tree.py:19-124 builds it (tests/test_gpu_ilqr_surface.py): one PotentialField + three quadratic
    potentials per trajectory node, root key -1 holding x0, from the oracle's materialised fields"""
    flat = oi.flatten(sst["nodes"])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    fields, gx, gy, off = oi.node_fields(cfg, flat, x0, sst["target_lane"], use_exo)
    xx, yy = np.meshgrid(gx, gy)
    t = Tree()
    t.add_node(Node(-1, None, x0))
    w_des, w_con, w_ctrl = np.diag(list(cfg.w_des_state)), np.diag(list(cfg.w_state_con)), np.diag(list(cfg.w_ctrl))
    for k in range(len(flat["parent"])):
        p = flat["prob"][k]
        pots = [[PotentialField(off, cfg.grid_res, xx, yy, fields[k]),
                 StatePotential(w_des * p, np.array([0, 0, sst["target_vel"], 0.0, 0.0, 0.0])),
                 StateConstraint(w_con * p, np.array(list(cfg.state_lower)), np.array(list(cfg.state_upper)))],
                [ControlPotential(w_ctrl * p)]]
        t.add_node(Node(k, int(flat["parent"][k]), pots))
    return flat, x0, TreeCost(t, 6, 2)


_generic = {}


def _generic_case(use_exo):
    if use_exo not in _generic:
        sst = scripted_scenario_tree("lead", 4)
        cfg = oi.default_cfg(max_iter=100)
        flat, x0, cost = _reference_style_cost_tree(cfg, sst, use_exo)
        _generic[use_exo] = (cfg, flat, x0, cost)
    return _generic[use_exo]


def test_generic_mode_through_the_solver_surface(hip_predictor):
    """iLQR.score on materialised fields: L against TreeCost.l, J against a fit of one iteration, and the planner mode's bits"""
    cfg, flat, x0, cost = _generic_case(1)
    c = _case(hip_predictor, "lead", 4)
    M = c["M"]
    solver = iLQR(BicycleDynamics(cfg.dt, cfg.wheelbase))
    xs, L, J = solver.score(c["cands"], cost)
    assert xs.shape == (3, M, 6) and L.shape == (3, M) and J.shape == (3,)
    for k in range(3):
        for i in (0, M // 2, M - 1):
            assert L[k, i] == cost.l(xs[k, i], c["cands"][k, i], i), (k, i)
        one = iLQR(BicycleDynamics(cfg.dt, cfg.wheelbase))
        one.fit(c["cands"][k], cost, n_iterations=1)
        assert J[k] == one.J_opt, (k, J[k], one.J_opt)
    assert np.array_equal(xs, c["xs"]) and np.array_equal(L, c["L"]) and np.array_equal(J, c["J"])      # analytic fields: the same bits


def test_candidate_that_leaves_the_grid(hip_predictor):
    """constant controls that carry the ego off the 102 m field (and a lane far from it, as test_hip_ilqr_grid_border_and_outside): the
    states stay finite, the border cells are read (indices clamped behind the cast), the node costs are mind_cost_eval's at those states"""
    sst = scripted_scenario_tree("straight", 3)
    cfg = oi.default_cfg(max_iter=3)
    flat = oi.flatten(sst["nodes"])
    M = len(flat["parent"])
    lane = sst["target_lane"] + np.array([49.0, 50.5])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    T = M * cfg.dt
    rate = 6.0 * 90.0 / T ** 3                                 # constant acceleration rate: 90 m beyond the coasting distance at the last node
    cands = np.stack([np.tile([rate, 0.0], (M, 1)), np.tile([rate, 0.002], (M, 1)), np.zeros((M, 2))])
    xs, L, J = hip_predictor.ilqr_score(cfg, [flat], x0, lane, sst["target_vel"], 1, cands)
    xs, L = xs[0], L[0]
    assert np.all(np.isfinite(xs)) and np.all(np.isfinite(L)) and np.all(np.isfinite(J))
    half = 0.5 * (cfg.grid_w - 1) * cfg.grid_res
    assert abs(xs[0, -1, 0] - x0[0]) > half + 10.0 and np.hypot(*(xs[1, -1, :2] - x0[:2])) > half + 10.0      # well off the field
    assert np.abs(xs[2, :, :2] - x0[:2]).max() < half
    for k in range(3):
        got = hip_predictor.cost_eval(cfg, np.arange(M), xs[k], cands[k], flat, x0=x0, lane=lane, target_vel=sst["target_vel"], use_exo=1)["l"]
        assert np.array_equal(L[k], got), k
        assert np.array_equal(L[k], oi.node_derivs(cfg, flat, x0, lane, sst["target_vel"], 1, xs[k], cands[k])["l"]), k


def test_multi_start_fit(hip_predictor):
    cfg, flat, x0, cost = _generic_case(1)
    M = len(flat["parent"])
    dyn = BicycleDynamics(cfg.dt, cfg.wheelbase)
    warm = iLQR(dyn)
    _, us3 = warm.fit(np.zeros((M, 2)), cost, n_iterations=3)
    cands = np.stack([np.zeros((M, 2)), us3, np.random.default_rng(9).normal(size=(M, 2))])
    multi = iLQR(dyn)
    xs, us = multi.fit(cands, cost, n_iterations=5)
    J = iLQR(dyn).score(cands, cost)[2]
    assert np.array_equal(multi.start_costs, J) and multi.start_index == int(np.argmin(J)) == 1
    single = iLQR(dyn)
    xs1, us1 = single.fit(cands[multi.start_index], cost, n_iterations=5)
    assert np.array_equal(xs, xs1) and np.array_equal(us, us1)
    assert (multi.J_opt, multi.iterations, multi._mu, multi.converged) == (single.J_opt, single.iterations, single._mu, single.converged)
    assert single.start_index is None and single.start_costs is None
    # a 2-D us_init is today's path: the reference golden of the warm-start fit (test_hip_ilqr_matches_reference_golden's tolerance)
    G = dict(np.load(os.path.join(ROOT, "tests", "golden", "ilqr.npz")))
    _, _, _, cost_w = _generic_case(0)
    plain = iLQR(dyn)
    xs_w, us_w = plain.fit(np.zeros((M, 2)), cost_w, n_iterations=100)
    assert np.abs(xs_w - G["lead_a4_it100_xs_w"]).max() < 1e-8 and plain.start_index is None


def _raw_score(hp, call, cfg, n_cand, us, xs, L, J, n_trees=1):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    rc = hp.lib.mind_ilqr_score_trees(hp.ctx, C.byref(cfg), None, call.trees, n_trees, dp(call.x0), dp(call.lane), len(call.lane), call.tv, 1, n_cand,
                                      dp(us), dp(xs), dp(L), dp(J))
    return rc, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode()


def test_rejected_requests(hip_predictor):
    """every bad request is refused on the host, with a message, before any device work"""
    hp = hip_predictor
    c = _case(hp, "lead", 4)
    cfg, M = c["cfg"], c["M"]
    call = IlqrCall(hp.lib, cfg, [c["flat"]], c["x0"], c["lane"], c["tv"])
    us, J = np.zeros((2, M, 2)), np.full((2, 1), -7.0)
    rc, msg = _raw_score(hp, call, cfg, 0, us, None, None, J)
    assert rc == _lib.MIND_EINVAL and "n_cand = 0" in msg
    rc, msg = _raw_score(hp, call, cfg, -3, us, None, None, J)
    assert rc == _lib.MIND_EINVAL and "n_cand = -3" in msg
    rc, msg = _raw_score(hp, call, cfg, 2, us, None, None, None)
    assert rc == _lib.MIND_EINVAL and "null us_cand / J" in msg
    rc, msg = _raw_score(hp, call, cfg, 2, None, None, None, J)
    assert rc == _lib.MIND_EINVAL and "null us_cand / J" in msg
    for bad in (np.nan, np.inf, -np.inf):
        us_bad = us.copy()
        us_bad[1, M - 1, 1] = bad
        rc, msg = _raw_score(hp, call, cfg, 2, us_bad, None, None, J)
        assert rc == _lib.MIND_EINVAL and f"candidate 1 has a non-finite control at node {M - 1}" in msg, msg
    n_big = (1 << 20) // M + 1                                  # n_cand x sum M just above the 2^20 rows a call admits
    rc, msg = _raw_score(hp, call, cfg, n_big, np.zeros((n_big, M, 2)), None, None, np.zeros((n_big, 1)))
    assert rc == _lib.MIND_EINVAL and "rows supported" in msg
    with pytest.raises(_lib.MindError, match="n_cand = 0"):
        hp.ilqr_score(cfg, [c["flat"]], c["x0"], c["lane"], c["tv"], 1, np.zeros((0, M, 2)))
    with pytest.raises(ValueError):
        hp.ilqr_score(cfg, [c["flat"]], c["x0"], c["lane"], c["tv"], 1, np.zeros((2, M + 1, 2)))
    assert np.all(J == -7.0)                                    # nothing was written
    # and the context is as good as before
    assert np.array_equal(hp.ilqr_score(cfg, [c["flat"]], c["x0"], c["lane"], c["tv"], 1, c["cands"])[2][:, 0], c["J"])


def test_score_between_begin_and_finish_is_refused(hip_predictor):
    """MIND_ESTATE while a call begun with mind_ilqr_contingency_begin is pending; that call then finishes with its usual result"""
    hp = hip_predictor
    c = _case(hp, "lead", 4)
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    ref = hp.ilqr_contingency(cfg_w, cfg_f, [c["flat"]], c["x0"], c["lane"], c["tv"])
    call = IlqrCall(hp.lib, cfg_w, [c["flat"]], c["x0"], c["lane"], c["tv"], cfg_full=cfg_f)
    call.begin(hp)
    try:
        J = np.full((3, 1), -7.0)
        rc, msg = _raw_score(hp, call, c["cfg"], 3, c["cands"], None, None, J)
        assert rc == _lib.MIND_ESTATE and "has not been finished" in msg and np.all(J == -7.0)
        with pytest.raises(_lib.MindError):
            hp.ilqr_score(c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"], 1, c["cands"])
    finally:
        xs, us, sw, sf = call.wait().finish()
    assert np.array_equal(xs[0], ref[0][0]) and np.array_equal(us[0], ref[1][0]) and sw == ref[2] and sf == ref[3]
    assert np.array_equal(hp.ilqr_score(c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"], 1, c["cands"])[2][:, 0], c["J"])
