"""GPU: mind_ilqr_gains / mind_ilqr_policy_rollouts (k_ilqr_gains, k_ilqr_policy) and iLQR.policy / the lazy gain attributes / rollout_policy.
Every output has a bit-exact yardstick: the plain-Python restatement of the oracle's backward pass and line-search rule
(tests/ilqr_policy_restate.py, itself held to the oracle by tests/test_ilqr_policy_host.py), the solver's own one- and two-iteration
results and traces, and the scoring call.  The tests pin arithmetic, not optimal-control properties (V_x / V_xx are no Taylor model of the
cost-to-go: f_x is taken at the post state).  np.array_equal is the compare: it treats -0.0 as equal to +0.0."""
import ctypes as C

import numpy as np
import pytest

import ilqr_policy_restate as rs
from mind_amd import _lib
from mind_amd.planners.ilqr.dynamics import BicycleDynamics
from mind_amd.planners.ilqr.solver import iLQR
from mind_amd.predictor import IlqrCall
from mind_amd.runtime import get_runtime
from mind_amd.synth import scripted_scenario_tree
from oracle import ilqr as oi

pytestmark = pytest.mark.gpu
CASES = [("lead", 4), ("branch3", 12), ("deep", 4), ("straight", 1)]
GAIN_KEYS = ("k", "K", "dV", "V_x", "V_xx", "xs", "L")


def _cfg1():
    return oi.default_cfg(max_iter=1)


def _gains(hp, s, use_exo, us, mu, cfg=None):
    return hp.ilqr_gains(cfg or _cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], use_exo, us, mu)


def _rollouts(hp, s, use_exo, us, k, K, alpha, dx0=None, cfg=None, **kw):
    return hp.ilqr_policy_rollouts(cfg or _cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], use_exo, us, k, K, alpha, dx0, **kw)


def _assert_gains_equal(got, want, t=0):
    for name in GAIN_KEYS:
        assert got[name][t].shape == want[name].shape, name
        assert np.array_equal(got[name][t], want[name]), (name, np.abs(got[name][t] - want[name]).max())


@pytest.mark.parametrize("controls", ["zeros", "warm"])
@pytest.mark.parametrize("kind,a", CASES)
def test_gains_equal_the_restatement(kind, a, controls, hip_predictor):
    """k, K, dV, V_x, V_xx, xs, L bit for bit at mu = 1, 0.5 and 0; J is what a one-iteration solve reports"""
    s = rs.scene(kind, a)
    use_exo = 0 if controls == "zeros" else 1
    us = np.zeros((s["M"], 2)) if controls == "zeros" else rs.w6(kind, a, 1)
    if (kind, a) == ("branch3", 12):
        assert s["M"] > 64 and s["flat"]["mean"].shape[1] > 8
    if (kind, a) == ("deep", 4):
        assert s["M"] == 115
    one = hip_predictor.ilqr_solve(_cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], use_exo, us_init=[us])[2][0]["J"]
    for mu in (1.0, 0.5, 0.0):
        got = _gains(hip_predictor, s, use_exo, us, mu)
        want = rs.gains_of(s, use_exo, us, mu)
        assert want["bad"] == -1 and got["bad_node"][0] == -1, mu
        _assert_gains_equal(got, want)
        assert np.all(np.isfinite(got["K"][0])) and got["K"][0].any()
        assert got["J"][0] == one, (mu, got["J"][0], one)


@pytest.mark.parametrize("keep", [1, 3])
def test_gains_and_rollouts_of_a_tiny_tree(keep, hip_predictor):
    """one- and two-node trees (as test_sum_of_a_tiny_tree builds them); M = 1 is a single leaf with nothing to sum"""
    sst = scripted_scenario_tree("straight", 2)
    key, parent, data = sst["nodes"][0]
    flat = oi.flatten([(key, parent, [data[0], data[1][:, :keep], data[2][:, :keep], data[3]])])
    M = len(flat["parent"])
    assert M == (keep + 1) // 2
    s = dict(flat=flat, x0=oi.init_state(sst["state"], sst["ctrl"]), lane=sst["target_lane"], tv=sst["target_vel"], M=M)
    us = np.random.default_rng(5).normal(size=(M, 2))
    got = _gains(hip_predictor, s, 1, us, 1.0)
    want = rs.gains_of(s, 1, us, 1.0)
    assert got["bad_node"][0] == -1 and want["bad"] == -1
    _assert_gains_equal(got, want)
    assert got["J"][0] == hip_predictor.ilqr_solve(_cfg1(), [flat], s["x0"], s["lane"], s["tv"], 1, us_init=[us])[2][0]["J"]
    dx0 = np.array([[0.3, -0.2, 0.5, 0.02, 0.0, 0.0], [0.0] * 6])
    xs, un, L, J = _rollouts(hip_predictor, s, 1, us, got["k"][0], got["K"][0], [1.0, 0.5], dx0)
    for c, alpha in enumerate((1.0, 0.5)):
        xr, ur = rs.policy(_cfg1(), flat["parent"], s["x0"], want["xs"], us, want["k"], want["K"], alpha, dx0[c])
        assert np.array_equal(xs[0][c], xr) and np.array_equal(un[0][c], ur)
        assert J[c, 0] == rs.seq_sum(L[0][c])


@pytest.mark.parametrize("kind,a,use_exo,spec,accepted", rs.LINE_SEARCH)
def test_policy_rollouts_are_the_solvers_line_search(kind, a, use_exo, spec, accepted, hip_predictor):
    """gains at mu = 1 from the start controls, then the ten step sizes in one call: the accepted one is the one-iteration solve's result
    (device and oracle), its J the trace's, every earlier one was rejected"""
    hp = hip_predictor
    s = rs.scene(kind, a)
    us0 = rs.start_controls(kind, a, spec)
    g = _gains(hp, s, use_exo, us0, 1.0)
    assert g["bad_node"][0] == -1
    xs, un, L, J = _rollouts(hp, s, use_exo, us0, g["k"][0], g["K"][0], rs.step_sizes())
    xs, un, L, J = xs[0], un[0], L[0], J[:, 0]
    sx, su, st = hp.ilqr_solve(_cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], use_exo, us_init=[us0])
    tr = hp.ilqr_trace(0)[0]
    ref = oi.solve(_cfg1(), s["flat"], s["x0"], s["lane"], s["tv"], use_exo, us_init=us0, trace=True)
    print(f"{kind} {a}: accepted {tr[2]:.0f} J_opt {tr[1]!r} J {J.tolist()}")
    assert int(tr[2]) == accepted == int(ref["trace"][0][2]) and tr[0] == 1.0      # the fixture is what it was chosen for
    assert g["J"][0] == tr[1]
    for c in range(10):
        assert J[c] == rs.seq_sum(L[c]), c
    if accepted < 0:
        assert np.all(J >= tr[1])
        assert np.array_equal(sx[0], g["xs"][0]) and np.array_equal(su[0], us0)
        return
    assert np.array_equal(xs[accepted], sx[0]) and np.array_equal(un[accepted], su[0])
    assert np.array_equal(xs[accepted], ref["xs"]) and np.array_equal(un[accepted], ref["us"])
    assert J[accepted] == tr[3] and J[accepted] < tr[1]
    assert np.all(J[:accepted] >= tr[1])


def test_second_iteration_runs_at_mu_one_half(hip_predictor):
    """the two-iteration lane-only fit of ("branch3", 12): gains at the trace's mu = 0.5 about the one-iteration result, the accepted step
    size's rollout is the two-iteration result"""
    hp = hip_predictor
    s = rs.scene("branch3", 12)
    us0 = np.zeros((s["M"], 2))
    x1, u1, _ = hp.ilqr_solve(_cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], 0, us_init=[us0])
    x2, u2, _ = hp.ilqr_solve(oi.default_cfg(max_iter=2), [s["flat"]], s["x0"], s["lane"], s["tv"], 0, us_init=[us0])
    tr = hp.ilqr_trace(0)[1]
    ai = int(tr[2])
    assert tr[0] == 0.5 and ai >= 0
    g = _gains(hp, s, 0, u1[0], tr[0])
    assert np.array_equal(g["xs"][0], x1[0]) and g["J"][0] == tr[1]
    _assert_gains_equal(g, rs.gains_of(s, 0, u1[0], 0.5))
    xs, un, L, J = _rollouts(hp, s, 0, u1[0], g["k"][0], g["K"][0], rs.step_sizes())
    assert np.array_equal(xs[0][ai], x2[0]) and np.array_equal(un[0][ai], u2[0]) and J[ai, 0] == tr[3]
    assert np.all(J[:ai, 0] >= tr[1])
    two = oi.solve(oi.default_cfg(max_iter=2), s["flat"], s["x0"], s["lane"], s["tv"], 0, us_init=us0)
    assert np.array_equal(xs[0][ai], two["xs"]) and np.array_equal(un[0][ai], two["us"])


@pytest.mark.parametrize("kind,a", CASES)
def test_zero_step_and_zero_offset_is_the_nominal_trajectory(kind, a, hip_predictor):
    """alpha = 0, dx0 = 0: xs and L are the scoring call's bits for the same controls, us_out is us, J the sequential sum of that L"""
    hp = hip_predictor
    s = rs.scene(kind, a)
    us = rs.w6(kind, a, 1)
    g = _gains(hp, s, 1, us, 1.0)
    sxs, sL, sJ = hp.ilqr_score(_cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us[None])
    for dx0 in (None, np.zeros((1, 6))):
        xs, un, L, J = _rollouts(hp, s, 1, us, g["k"][0], g["K"][0], [0.0], dx0)
        assert np.array_equal(xs[0][0], sxs[0][0]) and np.array_equal(L[0][0], sL[0][0]) and np.array_equal(un[0][0], us)
        assert J[0, 0] == rs.seq_sum(sL[0][0])
    assert np.array_equal(g["xs"][0], sxs[0][0]) and np.array_equal(g["L"][0], sL[0][0]) and g["J"][0] == sJ[0, 0]


@pytest.mark.parametrize("kind,a", [("branch3", 12), ("straight", 1)])
def test_perturbed_starts_equal_the_restatement(kind, a, hip_predictor):
    """dx0 = +-(0.3, -0.2, 0.5, 0.02, 0, 0) and zeros, alpha 0 and 1: the restatement's policy bit for bit (covers K[0] dx0)"""
    hp = hip_predictor
    s = rs.scene(kind, a)
    us = rs.w6(kind, a, 1)
    g = _gains(hp, s, 1, us, 1.0)
    d = np.array([0.3, -0.2, 0.5, 0.02, 0.0, 0.0])
    dx0 = np.stack([d, -d, np.zeros(6)] * 2)
    alpha = np.array([0.0] * 3 + [1.0] * 3)
    xs, un, L, J = _rollouts(hp, s, 1, us, g["k"][0], g["K"][0], alpha, dx0)
    assert g["K"][0][0].any()
    for c in range(6):
        xr, ur = rs.policy(_cfg1(), s["flat"]["parent"], s["x0"], g["xs"][0], us, g["k"][0], g["K"][0], alpha[c], dx0[c])
        assert np.array_equal(xs[0][c], xr), (c, np.abs(xs[0][c] - xr).max())
        assert np.array_equal(un[0][c], ur), (c, np.abs(un[0][c] - ur).max())
        want_L = oi.node_derivs(_cfg1(), s["flat"], s["x0"], s["lane"], s["tv"], 1, xr, ur)["l"]
        assert np.array_equal(L[0][c], want_L) and J[c, 0] == rs.seq_sum(want_L)
    assert not np.array_equal(xs[0][0], xs[0][2]) and not np.array_equal(un[0][0], un[0][1])      # the offset and the feedback act


def test_batching_changes_nothing(hip_predictor):
    """three trees of different size in one call, 130 and 65 candidates: every (candidate, tree) slice equals the call with that tree and
    that candidate alone, with and without the optional outputs, for every size of the candidate blocks; gains likewise"""
    hp = hip_predictor
    a = 4
    scenes = [rs.scene(kind, a) for kind in ("lead", "straight", "branch3")]
    base = scenes[0]
    cfg, x0, lane, tv = _cfg1(), base["x0"], base["lane"], base["tv"]
    flats = [s["flat"] for s in scenes]
    Ms = [s["M"] for s in scenes]
    assert len(set(Ms)) == 3
    rng = np.random.default_rng(29)
    us = [rng.normal(size=(M, 2)) * np.array([0.5, 0.05]) for M in Ms]
    g = hp.ilqr_gains(cfg, flats, x0, lane, tv, 1, us, [1.0, 0.5, 0.25])
    assert np.all(g["bad_node"] == -1)
    for t in range(3):
        g1 = hp.ilqr_gains(cfg, [flats[t]], x0, lane, tv, 1, us[t], [1.0, 0.5, 0.25][t])
        for name in GAIN_KEYS:
            assert np.array_equal(g[name][t], g1[name][0]), (name, t)
        assert g["J"][t] == g1["J"][0]
    assert np.array_equal(hp.ilqr_gains(cfg, flats, x0, lane, tv, 1, np.concatenate(us), np.array([1.0, 0.5, 0.25]))["K"][2], g["K"][2])
    nc = 130
    alpha = rng.uniform(0.0, 1.0, size=nc)
    dx0 = rng.normal(size=(nc, 6)) * np.array([0.3, 0.3, 0.5, 0.02, 0.1, 0.01])
    dx0[0] = 0.0
    xs, un, L, J = hp.ilqr_policy_rollouts(cfg, flats, x0, lane, tv, 1, us, g["k"], g["K"], alpha, dx0)
    assert J.shape == (nc, 3) and [x.shape for x in xs] == [(nc, M, 6) for M in Ms] and [u.shape for u in un] == [(nc, M, 2) for M in Ms]
    assert np.all(np.isfinite(J))
    for t in range(3):
        for c in range(nc):
            x1, u1, l1, j1 = hp.ilqr_policy_rollouts(cfg, [flats[t]], x0, lane, tv, 1, us[t], g["k"][t], g["K"][t], alpha[c:c + 1], dx0[c:c + 1])
            assert np.array_equal(xs[t][c], x1[0][0]) and np.array_equal(un[t][c], u1[0][0]) and np.array_equal(L[t][c], l1[0][0]), (t, c)
            assert J[c, t] == j1[0, 0], (t, c)
    x65 = hp.ilqr_policy_rollouts(cfg, flats, x0, lane, tv, 1, us, g["k"], g["K"], alpha[:65], dx0[:65])
    assert all(np.array_equal(x65[0][t], xs[t][:65]) and np.array_equal(x65[1][t], un[t][:65]) and np.array_equal(x65[2][t], L[t][:65]) for t in range(3))
    assert np.array_equal(x65[3], J[:65])
    for wx, wu, wl in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        x2, u2, l2, j2 = hp.ilqr_policy_rollouts(cfg, flats, x0, lane, tv, 1, us, g["k"], g["K"], alpha, dx0, want_xs=wx, want_us=wu, want_L=wl)
        assert (x2 is None) == (not wx) and (u2 is None) == (not wu) and (l2 is None) == (not wl) and np.array_equal(j2, J)
    try:
        for block in (64, 7, 1):
            hp.set_tuning("ilqr_score_block", block)
            for n in (nc, 65):
                x3, u3, l3, j3 = hp.ilqr_policy_rollouts(cfg, flats, x0, lane, tv, 1, us, g["k"], g["K"], alpha[:n], dx0[:n])
                assert np.array_equal(j3, J[:n]), (block, n)
                assert all(np.array_equal(x3[t], xs[t][:n]) and np.array_equal(u3[t], un[t][:n]) and np.array_equal(l3[t], L[t][:n]) for t in range(3)), (block, n)
    finally:
        hp.set_tuning("ilqr_score_block", 0)


def _singular_fixture():
    """("straight", 4) with w_ctrl = -dt^2 / 2: at mu = 1 the leaf's Q_uu = 2 w p + dt^2 (0 + mu) is exactly zero (node probability 1)"""
    sst = scripted_scenario_tree("straight", 4)
    cfg = _cfg1()
    cfg.w_ctrl[:] = [-(cfg.dt * cfg.dt) / 2] * 2
    flat = oi.flatten(sst["nodes"])
    assert set(flat["prob"].tolist()) == {1.0}
    return cfg, sst, dict(flat=flat, x0=oi.init_state(sst["state"], sst["ctrl"]), lane=sst["target_lane"], tv=sst["target_vel"], M=len(flat["parent"]))


def test_singular_q_uu_is_reported_and_zero_filled(hip_predictor):
    hp = hip_predictor
    cfg, sst, s = _singular_fixture()
    M = s["M"]
    other = rs.scene("branch3", 4)                               # leaves of probability < 1: 2 w p + dt^2 mu != 0
    us = [np.zeros((M, 2)), np.zeros((other["M"], 2))]
    g = hp.ilqr_gains(cfg, [s["flat"], other["flat"]], s["x0"], s["lane"], s["tv"], 1, us, 1.0)
    assert g["bad_node"].tolist() == [M - 1, -1]
    for name in ("k", "K", "dV", "V_x", "V_xx"):
        assert not g[name][0].any(), name
    want = rs.gains_of(s, 1, us[0], 1.0, cfg)
    assert want["bad"] == M - 1
    _assert_gains_equal(g, want)                                 # zeros, and the valid xs / L
    assert g["J"][0] == hp.ilqr_solve(cfg, [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us_init=[us[0]])[2][0]["J"]
    alone = hp.ilqr_gains(cfg, [other["flat"]], s["x0"], s["lane"], s["tv"], 1, us[1], 1.0)
    assert alone["bad_node"][0] == -1 and alone["K"][0].any()
    for name in GAIN_KEYS:
        assert np.array_equal(g[name][1], alone[name][0]), name
    _assert_gains_equal(g, rs.gains_of(dict(other, x0=s["x0"], lane=s["lane"], tv=s["tv"]), 1, us[1], 1.0, cfg), t=1)
    assert hp.ilqr_gains(cfg, [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us[0], 0.5)["bad_node"][0] == -1      # another mu: regular
    # through the solver surface: the fit burns its iteration on the singular pass (mu stays 1), policy() raises as numpy.linalg.solve would
    from test_gpu_ilqr_score import _reference_style_cost_tree
    flat, x0, cost = _reference_style_cost_tree(cfg, sst, 1)
    solver = iLQR(BicycleDynamics(cfg.dt, cfg.wheelbase))
    solver.fit(np.zeros((M, 2)), cost, n_iterations=1)
    assert solver._mu == 1.0
    with pytest.raises(np.linalg.LinAlgError, match=f"node {M - 1}"):
        solver.policy()
    with pytest.raises(np.linalg.LinAlgError):
        solver.K
    assert solver.policy(mu=0.5)["K"].any()


def test_generic_mode_through_the_solver_surface(hip_predictor):
    """iLQR.fit on materialised fields, then the lazy attributes: the generic call's bits, the planner mode's bits (analytic fields: the same
    values) and the restatement fed from cost_eval; rollout_policy reproduces the next fit's first step"""
    from test_gpu_ilqr_score import _generic_case
    hp = hip_predictor
    cfg, flat, x0, cost = _generic_case(1)
    s = rs.scene("lead", 4)
    M = s["M"]
    dyn = BicycleDynamics(cfg.dt, cfg.wheelbase)
    us0 = np.zeros((M, 2))                                       # (the oracle's second iteration from zeros: mu = 0.5, the full step accepted)
    solver = iLQR(dyn)
    xs1, us1 = solver.fit(us0, cost, n_iterations=1)
    assert solver._policy is None
    p = cost.pack()
    cfg0 = solver._cfg(0)
    direct = hp.ilqr_gains(cfg0, [p], p["x0"], None, 0.0, 0, us1, solver._mu, grid=p["grid"])
    assert direct["bad_node"][0] == -1
    for name in ("k", "K", "dV", "V_x", "V_xx"):
        assert np.array_equal(getattr(solver, name), direct[name][0]), name
    pol = solver.policy()
    assert pol["k"] is solver.k and np.array_equal(pol["xs"], xs1) and pol["mu"] == solver._mu
    planner = _gains(hp, s, 1, us1, solver._mu)
    for name in GAIN_KEYS:
        assert np.array_equal(planner[name][0], pol[name]), name
    d = hp.cost_eval(cfg0, np.arange(M), xs1, us1, p, grid=p["grid"])
    k, K, dV, Vx, Vxx, bad = rs.backward(cfg0, p["parent"], xs1, us1, d, solver._mu)
    assert bad == -1 and np.array_equal(rs.rollout(cfg0, p["parent"], p["x0"], us1), xs1)
    assert np.array_equal(solver.k, k) and np.array_equal(solver.K, K) and np.array_equal(solver.V_xx, Vxx) and np.array_equal(solver.V_x, Vx)
    assert np.array_equal(solver.dV, dV)
    # the second iteration of a two-iteration fit starts from (xs1, us1) with this mu: its accepted step is a rollout of this policy
    two = iLQR(dyn)
    xs2, us2 = two.fit(us0, cost, n_iterations=2)
    tr = get_runtime().ilqr_trace(0)
    assert len(tr) == 2 and tr[1][0] == solver._mu
    ai = int(tr[1][2])
    assert ai == 0                                               # the full step: rollout_policy(1.0)
    rx, ru, rL, rJ = solver.rollout_policy(1.0)
    assert np.array_equal(rx, xs2) and np.array_equal(ru, us2) and rJ == tr[1][3]
    bx, bu, bL, bJ = solver.rollout_policy(rs.step_sizes()[:3], dx0=np.zeros(6))
    assert np.array_equal(bx[0], xs2) and np.array_equal(bu[0], us2) and bJ[0] == rJ and bJ.shape == (3,)
    solver.fit(us0, cost, n_iterations=2)                        # the next fit clears the attributes
    assert solver._policy is None and not np.array_equal(solver.k, k)


def test_trajectory_tree_optimizer_policy(hip_predictor):
    """TrajectoryTreeOptimizer.policy(): the gains about the trajectory the last solve / warm_start_solve returned -- that fit's
    configuration block, cost (lane only / full) and final mu -- equal to the direct call"""
    from mind_amd.planners.basic.tree import Node, Tree
    from mind_amd.planners.mind.configs.planning.demo_1 import TrajTreeCfg
    from mind_amd.planners.mind.trajectory_tree import TrajectoryTreeOptimizer, ilqr_cfg_from
    hp = hip_predictor
    sst = scripted_scenario_tree("branch3", 4)
    tree = Tree()
    for key, parent, data in sst["nodes"]:
        tree.add_node(Node(key, parent, data))
    config = TrajTreeCfg()
    opt = TrajectoryTreeOptimizer(config, runtime=hp)
    with pytest.raises(RuntimeError, match="no solve"):
        opt.policy()
    flat = oi.flatten(sst["nodes"])
    x0, lane, tv = oi.init_state(sst["state"], sst["ctrl"]), np.asarray(sst["target_lane"], np.float64), float(sst["target_vel"])
    opt.init_warm_start_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
    xs_w, us_w = opt.warm_start_solve()
    mu_w = opt.debug["mu"]
    pol_w = opt.policy()
    opt.init_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
    assert np.array_equal(opt.policy()["K"], pol_w["K"])         # a new cost tree alone changes nothing: the policy is the last FIT's
    traj = opt.solve(us_w)
    us_f, mu_f = traj._arrays[1][1:], opt.debug["mu"]
    pol_f = opt.policy()
    for pol, block, use_exo, us, xs, mu in ((pol_w, "w_opt_cfg", 0, us_w, xs_w, mu_w), (pol_f, "opt_cfg", 1, us_f, traj._arrays[0][1:], mu_f)):
        want = hp.ilqr_gains(ilqr_cfg_from(config, block), [flat], x0, lane, tv, use_exo, us, mu)
        assert want["bad_node"][0] == -1 and pol["mu"] == mu and pol["J"] == want["J"][0]
        for name in GAIN_KEYS:
            assert np.array_equal(pol[name], want[name][0]), (block, name)
        assert np.array_equal(pol["xs"], xs)
    assert not np.array_equal(pol_w["K"], pol_f["K"])            # the two fits differ in cost and trajectory
    other = hp.ilqr_gains(ilqr_cfg_from(config, "opt_cfg"), [flat], x0, lane, tv, 1, us_f, 2.0)
    assert np.array_equal(opt.policy(mu=2.0)["K"], other["K"][0]) and not np.array_equal(other["K"][0], pol_f["K"])
    with pytest.raises(ValueError, match="mu must be"):
        opt.policy(mu=-1.0)


def test_runtime_level_functions(hip_predictor):
    """mind_amd.runtime.ilqr_gains / ilqr_policy_rollouts: the thread's runtime gives the bits of any other context"""
    from mind_amd import runtime
    s = rs.scene("lead", 4)
    us = rs.w6("lead", 4, 1)
    g = runtime.ilqr_gains(_cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us, 0.5)
    want = _gains(hip_predictor, s, 1, us, 0.5)
    for name in GAIN_KEYS:
        assert np.array_equal(g[name][0], want[name][0]), name
    assert g["J"][0] == want["J"][0] and g["bad_node"][0] == -1
    dx0 = np.array([[0.3, -0.2, 0.5, 0.02, 0.0, 0.0], [0.0] * 6])
    got = runtime.ilqr_policy_rollouts(_cfg1(), [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us, g["k"][0], g["K"][0], [1.0, 0.0], dx0, want_L=False)
    ref = _rollouts(hip_predictor, s, 1, us, want["k"][0], want["K"][0], [1.0, 0.0], dx0)
    assert got[2] is None and np.array_equal(got[0][0], ref[0][0]) and np.array_equal(got[1][0], ref[1][0]) and np.array_equal(got[3], ref[3])


def _raw(hp, call, cfg, fn, *tail, n_trees=1):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if isinstance(a, np.ndarray) else a
    rc = fn(hp.ctx, C.byref(cfg), None, call.trees, n_trees, dp(call.x0), dp(call.lane), len(call.lane), call.tv, 1, *[dp(v) for v in tail])
    return rc, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode()


def _gains_out(M, n_trees=1):
    arrs = dict(k=np.full((M, 2), -7.0), K=np.full((M, 12), -7.0))
    bad = np.full(n_trees, -7, np.int32)
    out = _lib.IlqrGainsOut()
    out.k, out.K = (arrs[n].ctypes.data_as(C.POINTER(C.c_double)) for n in ("k", "K"))
    out.bad_node = bad.ctypes.data_as(C.POINTER(C.c_int32))
    return out, arrs, bad


def test_rejected_requests(hip_predictor):
    """every bad request is refused on the host, with a message, before any device work"""
    hp = hip_predictor
    s = rs.scene("lead", 4)
    cfg, M = _cfg1(), s["M"]
    call = IlqrCall(hp.lib, cfg, [s["flat"]], s["x0"], s["lane"], s["tv"])
    us, mu = np.zeros((M, 2)), np.ones(1)
    out, arrs, bad = _gains_out(M)
    ga, po = hp.lib.mind_ilqr_gains, hp.lib.mind_ilqr_policy_rollouts
    EINVAL = _lib.MIND_EINVAL
    # ---- mind_ilqr_gains
    for tail in ((None, mu, C.byref(out)), (us, None, C.byref(out)), (us, mu, None)):
        rc, msg = _raw(hp, call, cfg, ga, *tail)
        assert rc == EINVAL and "null" in msg, msg
    for miss in ("k", "K", "bad_node"):
        o2, _, _ = _gains_out(M)
        setattr(o2, miss, None)
        rc, msg = _raw(hp, call, cfg, ga, us, mu, C.byref(o2))
        assert rc == EINVAL and "null" in msg, (miss, msg)
    for v in (np.nan, np.inf, -np.inf):
        ub = us.copy()
        ub[M - 2, 1] = v
        rc, msg = _raw(hp, call, cfg, ga, ub, mu, C.byref(out))
        assert rc == EINVAL and f"non-finite control at node {M - 2}" in msg, msg
        rc, msg = _raw(hp, call, cfg, ga, us, np.array([v]), C.byref(out))
        assert rc == EINVAL and "non-finite mu of tree 0" in msg, msg
    rc, msg = _raw(hp, call, cfg, ga, us, np.array([-0.5]), C.byref(out))
    assert rc == EINVAL and "negative mu of tree 0" in msg, msg
    assert np.all(arrs["k"] == -7.0) and np.all(arrs["K"] == -7.0) and bad[0] == -7      # nothing was written
    # ---- mind_ilqr_policy_rollouts
    k, K, alpha, J = np.zeros((M, 2)), np.zeros((M, 12)), np.ones(2), np.full((2, 1), -7.0)
    good = dict(us=us, k=k, K=K, n=2, alpha=alpha, dx0=None, xs=None, uo=None, L=None, J=J)
    tail = lambda **kw: list({**good, **kw}.values())
    for n in (0, -3):
        rc, msg = _raw(hp, call, cfg, po, *tail(n=n))
        assert rc == EINVAL and f"n_cand = {n}" in msg, msg
    for name in ("us", "k", "K", "alpha", "J"):
        rc, msg = _raw(hp, call, cfg, po, *tail(**{name: None}))
        assert rc == EINVAL and "null" in msg, (name, msg)
    for v in (np.nan, np.inf):
        ub, kb, Kb, ab, db = us.copy(), k.copy(), K.copy(), alpha.copy(), np.zeros((2, 6))
        ub[3, 0] = kb[4, 1] = Kb[5, 7] = ab[1] = db[1, 2] = v
        for name, arr, what in (("us", ub, "non-finite control at node 3"), ("k", kb, "non-finite k at node 4"), ("K", Kb, "non-finite K at node 5"),
                                ("alpha", ab, "non-finite alpha of candidate 1"), ("dx0", db, "non-finite dx0 of candidate 1")):
            rc, msg = _raw(hp, call, cfg, po, *tail(**{name: arr}))
            assert rc == EINVAL and what in msg, (name, msg)
    n_big = (1 << 20) // M + 1                                  # n_cand x sum M just above the 2^20 rows a call admits
    rc, msg = _raw(hp, call, cfg, po, *tail(n=n_big, alpha=np.ones(n_big), J=np.zeros((n_big, 1))))
    assert rc == EINVAL and "rows supported" in msg, msg
    assert np.all(J == -7.0)
    # ---- more cost trees than a launch's grid takes (n_trees becomes gridDim.y of the policy launch): 65536 records of the same one-node tree
    n_many = 65536
    one = dict(parent=np.array([-1], np.int32), prob=np.ones(1, np.float32), mean=np.zeros((1, 1, 2), np.float32), cov=np.zeros((1, 1), np.float32))
    many = (_lib.CostTree * n_many)()
    for t in many:
        t.n_nodes, t.n_agents = 1, 1
        t.parent = one["parent"].ctypes.data_as(C.POINTER(C.c_int32))
        t.prob = one["prob"].ctypes.data_as(C.POINTER(C.c_float))
        t.agent_mean = one["mean"].ctypes.data_as(C.POINTER(C.c_float))
        t.agent_cov = one["cov"].ctypes.data_as(C.POINTER(C.c_float))
    call.trees = many
    us_m, k_m, K_m, J_m = np.zeros((n_many, 2)), np.zeros((n_many, 2)), np.zeros((n_many, 12)), np.full((1, n_many), -7.0)
    out_m, arrs_m, bad_m = _gains_out(n_many, n_many)
    rc, msg = _raw(hp, call, cfg, ga, us_m, np.ones(n_many), C.byref(out_m), n_trees=n_many)
    assert rc == EINVAL and "65536 cost trees > 65535 supported" in msg and "mind_ilqr_gains" in msg, msg
    rc, msg = _raw(hp, call, cfg, po, us_m, k_m, K_m, 1, np.ones(1), None, None, None, None, J_m, n_trees=n_many)
    assert rc == EINVAL and "65536 cost trees > 65535 supported" in msg and "mind_ilqr_policy_rollouts" in msg, msg
    assert np.all(arrs_m["k"] == -7.0) and np.all(arrs_m["K"] == -7.0) and np.all(bad_m == -7) and np.all(J_m == -7.0)
    # ---- the Python surface
    with pytest.raises(ValueError, match="us must be"):
        _gains(hp, s, 1, np.zeros((M + 1, 2)), 1.0)
    with pytest.raises(_lib.MindError, match="negative mu"):
        _gains(hp, s, 1, us, -1.0)
    with pytest.raises(_lib.MindError, match="n_cand = 0"):
        _rollouts(hp, s, 1, us, k, K.reshape(M, 2, 6), [])
    with pytest.raises(ValueError, match="dx0 must be"):
        _rollouts(hp, s, 1, us, k, K.reshape(M, 2, 6), [1.0], np.zeros((2, 6)))
    # and the context is as good as before
    assert _gains(hp, s, 1, us, 1.0)["bad_node"][0] == -1


def test_calls_between_begin_and_finish_are_refused(hip_predictor):
    """MIND_ESTATE while a call begun with mind_ilqr_contingency_begin is pending; that call then finishes with its usual result"""
    hp = hip_predictor
    s = rs.scene("lead", 4)
    M = s["M"]
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    ref = hp.ilqr_contingency(cfg_w, cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"])
    call = IlqrCall(hp.lib, cfg_w, [s["flat"]], s["x0"], s["lane"], s["tv"], cfg_full=cfg_f)
    us, k, K = np.zeros((M, 2)), np.zeros((M, 2)), np.zeros((M, 12))
    out, arrs, bad = _gains_out(M)
    J = np.full((1, 1), -7.0)
    call.begin(hp)
    try:
        rc, msg = _raw(hp, call, _cfg1(), hp.lib.mind_ilqr_gains, us, np.ones(1), C.byref(out))
        assert rc == _lib.MIND_ESTATE and "has not been finished" in msg and bad[0] == -7
        rc, msg = _raw(hp, call, _cfg1(), hp.lib.mind_ilqr_policy_rollouts, us, k, K, 1, np.ones(1), None, None, None, None, J)
        assert rc == _lib.MIND_ESTATE and "has not been finished" in msg and np.all(J == -7.0)
        with pytest.raises(_lib.MindError):
            _gains(hp, s, 1, us, 1.0)
    finally:
        xs, un, sw, sf = call.wait().finish()
    assert np.array_equal(xs[0], ref[0][0]) and np.array_equal(un[0], ref[1][0]) and sw == ref[2] and sf == ref[3]
    assert _gains(hp, s, 1, us, 1.0)["bad_node"][0] == -1
