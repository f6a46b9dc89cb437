"""CPU: the yardstick of mind_ilqr_gains / mind_ilqr_policy_rollouts -- the plain-Python restatement (tests/ilqr_policy_restate.py) reproduces the
C oracle's one- and two-iteration solves bit for bit and the imported reference's backward pass to BLAS accuracy -- and what of the new
surface needs no device: the entry points fail cleanly without a context, their bindings match the header, and iLQR.policy / the lazy
attributes / rollout_policy check their arguments and call the runtime once.

These tests pin arithmetic, not optimal-control properties: the reference evaluates f_x at the post state and pairs l_x[key] with V_x[key],
so V_x / V_xx are no Taylor model of the cost-to-go."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ilqr_policy_restate as rs
from mind_amd import _lib
from mind_amd.planners.ilqr import solver as ilqr_solver
from mind_amd.planners.ilqr.dynamics import BicycleDynamics
from mind_amd.predictor import HipPredictor
from mind_amd.synth import scripted_scenario_tree
from oracle import ilqr as oi
from oracle import ref_harness as rh
from ref_golden import Recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# largest |restatement - reference| / max|reference| over the recorded arrays, measured when the golden was recorded: 2.891e-14 (dV, lead,
# noisy controls, mu = 1.0; 1.5e-15 at most from zero controls); both sides are float64 and differ in BLAS summation order and in numpy's libm
# trigonometry.  The bar is 8 x that, far below the 1e-9 the oracle itself is held to against the reference.
REF_MEASURED = 2.9e-14
REF_BAR = 8 * REF_MEASURED


def _line_search(kind, a, use_exo, us0, mu=1.0, derivs_cfg=None):
    """one backward pass and the ten line-search candidates, restated -> (gains, [(xs, us, J)] per step size)"""
    s = rs.scene(kind, a)
    cfg = derivs_cfg or oi.default_cfg(max_iter=1)
    g = rs.restated_gains(kind, a, use_exo, us0, mu, cfg)
    assert g["bad"] == -1
    cands = []
    for alpha in rs.step_sizes():
        xn, un = rs.policy(cfg, s["flat"]["parent"], s["x0"], g["xs"], us0, g["k"], g["K"], alpha, np.zeros(6))
        L = oi.node_derivs(cfg, s["flat"], s["x0"], s["lane"], s["tv"], use_exo, xn, un)["l"]
        cands.append((xn, un, rs.seq_sum(L)))
    return g, cands


@pytest.mark.parametrize("kind,a,use_exo,spec,accepted", rs.LINE_SEARCH)
def test_restatement_is_the_oracles_one_iteration_solve(kind, a, use_exo, spec, accepted):
    """backward + policy at the accepted step size are the oracle's xs / us bit for bit, the candidate's J is its trace's; every step before
    the accepted one was rejected (J >= J_opt)"""
    s = rs.scene(kind, a)
    us0 = rs.start_controls(kind, a, spec)
    one = oi.solve(oi.default_cfg(max_iter=1), s["flat"], s["x0"], s["lane"], s["tv"], use_exo, us_init=us0, trace=True)
    tr = one["trace"][0]
    assert int(tr[2]) == accepted and tr[0] == 1.0      # the fixture is what it was chosen for
    g, cands = _line_search(kind, a, use_exo, us0)
    J_opt = tr[1]
    if accepted < 0:
        assert all(J >= J_opt for _, _, J in cands)
        assert np.array_equal(g["xs"], one["xs"]) and np.array_equal(us0, one["us"])
        return
    xn, un, J = cands[accepted]
    assert np.array_equal(xn, one["xs"]), np.abs(xn - one["xs"]).max()
    assert np.array_equal(un, one["us"]), np.abs(un - one["us"]).max()
    assert J == tr[3] and J < J_opt
    assert all(Jc >= J_opt for _, _, Jc in cands[:accepted])


@pytest.mark.parametrize("kind,a", [("lead", 4), ("branch3", 12), ("deep", 4), ("straight", 1)])
def test_restatement_from_the_warm_controls(kind, a):
    """the full cost from the six-iteration controls: the second control set of the device test"""
    s = rs.scene(kind, a)
    us0 = rs.w6(kind, a, 1)
    one = oi.solve(oi.default_cfg(max_iter=1), s["flat"], s["x0"], s["lane"], s["tv"], 1, us_init=us0, trace=True)
    tr = one["trace"][0]
    g, cands = _line_search(kind, a, 1, us0)
    ai = int(tr[2])
    if ai >= 0:
        assert np.array_equal(cands[ai][0], one["xs"]) and np.array_equal(cands[ai][1], one["us"]) and cands[ai][2] == tr[3]
    assert all(J >= tr[1] for _, _, J in cands[:ai if ai >= 0 else 10])


def test_restatement_at_mu_one_half():
    """the second iteration of a lane-only fit runs its backward pass at mu = 0.5: from the one-iteration result, backward at the trace's mu
    and policy at the accepted step size give the two-iteration solve"""
    kind, a = "branch3", 12
    s = rs.scene(kind, a)
    us0 = np.zeros((s["M"], 2))
    one = oi.solve(oi.default_cfg(max_iter=1), s["flat"], s["x0"], s["lane"], s["tv"], 0, us_init=us0)
    two = oi.solve(oi.default_cfg(max_iter=2), s["flat"], s["x0"], s["lane"], s["tv"], 0, us_init=us0, trace=True)
    tr = two["trace"][1]
    assert tr[0] == 0.5 and int(tr[2]) >= 0
    g, cands = _line_search(kind, a, 0, one["us"], mu=tr[0])
    assert np.array_equal(g["xs"], one["xs"])
    xn, un, J = cands[int(tr[2])]
    assert np.array_equal(xn, two["xs"]) and np.array_equal(un, two["us"]) and J == tr[3]
    assert all(Jc >= tr[1] for _, _, Jc in cands[:int(tr[2])])


def test_singular_q_uu_is_reported_not_raised():
    """w_ctrl = -dt^2 / 2 and mu = 1 make the leaf's Q_uu exactly zero (the fixture of the solver's singular-path test)"""
    sst = scripted_scenario_tree("straight", 4)
    cfg = oi.default_cfg(max_iter=1)
    cfg.w_ctrl[:] = [-cfg.dt * cfg.dt / 2.0] * 2
    flat = oi.flatten(sst["nodes"])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    M = len(flat["parent"])
    us = np.zeros((M, 2))
    xs = rs.rollout(cfg, flat["parent"], x0, us)
    d = oi.node_derivs(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 1, xs, us)
    k, K, dV, Vx, Vxx, bad = rs.backward(cfg, flat["parent"], xs, us, d, 1.0)
    assert bad == M - 1 and not k.any() and not K.any() and not dV.any() and not Vx.any() and not Vxx.any()
    assert oi.solve(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 1, trace=True)["trace"][0][2] == -2.0


REF_CASES = [(kind, a, noisy, mu) for kind, a in (("lead", 5), ("branch3", 6)) for noisy in (False, True) for mu in (1.0, 0.25)]


@pytest.mark.reference
@pytest.mark.parametrize("kind,a,noisy,mu", REF_CASES)
def test_restatement_against_the_imported_references_backward_pass(kind, a, noisy, mu):
    """k, K, dV, V_x, V_xx of the imported reference after _forward_rollout(), _mu = mu, _backward_pass() on the planner's cost tree
    (init_cost_tree).  The reference's root key -1 aliases numpy row -1: its row M-1 of V_x / V_xx also holds node 0's value."""
    sst = scripted_scenario_tree(kind, a, seed=3)
    flat = oi.flatten(sst["nodes"])
    M = len(flat["parent"])
    us = np.zeros((M, 2))
    if noisy:
        us = us + np.random.default_rng(3).normal(size=(M, 2)) * 0.5

    def ref():
        m = rh.ref_modules()
        Tree, Node = m["planners.basic.tree"].Tree, m["planners.basic.tree"].Node
        TTO = m["planners.mind.trajectory_tree"].TrajectoryTreeOptimizer
        cfgmod = m["planners.mind.configs.planning.demo_1"]
        tree = Tree()
        for k_, p, d in sst["nodes"]:
            tree.add_node(Node(k_, p, d))
        opt = TTO(cfgmod.TrajTreeCfg())
        opt.init_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
        il = opt.ilqr
        il.fit(us.copy(), opt.cost_tree, n_iterations=0)      # the arrays of a fit, no iteration
        il._forward_rollout()
        il._mu = mu
        il._backward_pass()
        return dict(k=np.array(il.k), K=np.array(il.K), dV=np.array(il.dV), V_x=np.array(il.V_x), V_xx=np.array(il.V_xx))

    want = Recorded("ilqr_policy_ref")(f"{kind}{a}_{'noisy' if noisy else 'zeros'}_mu{mu}", ref)
    cfg = oi.default_cfg(max_iter=1)
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    xs = rs.rollout(cfg, flat["parent"], x0, us)
    d = oi.node_derivs(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 1, xs, us)
    k, K, dV, Vx, Vxx, bad = rs.backward(cfg, flat["parent"], xs, us, d, mu)
    assert bad == -1
    Vx, Vxx = Vx.copy(), Vxx.copy()
    Vx[M - 1] = Vx[M - 1] + Vx[0]
    Vxx[M - 1] = Vxx[M - 1] + Vxx[0]
    worst = 0.0
    for name, got in (("k", k), ("K", K), ("dV", dV), ("V_x", Vx), ("V_xx", Vxx)):
        ref_a = np.asarray(want[name], np.float64)
        assert ref_a.shape == got.shape, name
        dev = np.abs(got - ref_a).max() / np.abs(ref_a).max()
        print(f"{kind}{a} noisy={noisy} mu={mu} {name}: max|restated - reference| / max|reference| = {dev:.3e}")
        worst = max(worst, dev)
    assert worst <= REF_BAR, worst


# ---- the surface, without a device -------------------------------------------------------------------------------------------------------
def _decl(name):
    txt = open(os.path.join(ROOT, "include", "mind_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
    assert m, f"{name} is not declared in include/mind_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("mind_ilqr_gains", 13), ("mind_ilqr_policy_rollouts", 20)])
def test_bindings_match_the_header(name, n_args):
    args = _decl(name)
    fn = getattr(_lib.load(), name)
    assert len(args) == len(fn.argtypes) == n_args and fn.restype is C.c_int and name in _lib.EXPORTS
    for a, t in zip(args, fn.argtypes):
        if a.startswith("int "):
            assert t is C.c_int, a
        elif a.startswith("double ") and "*" not in a:
            assert t is C.c_double, a
        else:
            assert "*" in a and t not in (C.c_int, C.c_double), a
    assert C.sizeof(_lib.IlqrGainsOut) == 9 * 8


def test_calls_without_a_context_fail_cleanly():
    lib = _lib.load()
    k, K, bad = np.zeros((7, 2)), np.zeros((7, 12)), np.full(1, 5, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = _lib.IlqrGainsOut()
    out.k, out.K, out.bad_node = dp(k), dp(K), bad.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.mind_ilqr_gains(None, None, None, None, 1, None, None, 0, 0.0, 0, dp(k), dp(k), C.byref(out)) == _lib.MIND_EINVAL
    J = np.zeros((1, 1))
    assert lib.mind_ilqr_policy_rollouts(None, None, None, None, 1, None, None, 0, 0.0, 0, dp(k), dp(k), dp(K), 1, dp(k), None, None, None, None,
                                         dp(J)) == _lib.MIND_EINVAL
    assert bad[0] == 5 and not J.any()


def test_per_node_arrays_are_checked():
    assert HipPredictor._per_node([np.zeros((3, 2)), np.ones((2, 2))], 5, (2,), "us").shape == (5, 2)
    assert HipPredictor._per_node(np.zeros((5, 12)).reshape(5, 2, 6), 5, (2, 6), "K").shape == (5, 2, 6)
    with pytest.raises(ValueError, match="us must be"):
        HipPredictor._per_node(np.zeros((4, 2)), 5, (2,), "us")
    with pytest.raises(ValueError, match="K must be"):
        HipPredictor._per_node(np.zeros((5, 12)), 5, (2, 6), "K")


class _Cost:
    def __init__(self, n):
        self.n = n

    def pack(self):
        return dict(parent=np.arange(-1, self.n - 1, dtype=np.int32), grid=dict(), x0=np.zeros(6))


class _Runtime:
    """stands in for the HIP runtime: a fit returns its start controls, the gains are counters, bad_node as told"""

    def __init__(self, bad=-1):
        self.bad, self.gains_calls, self.rollouts = bad, [], []

    def ilqr_solve_fields(self, cfg, grid, tree, x0, us_init=None):
        return np.zeros((len(us_init), 6)), np.array(us_init), dict(iterations=cfg.max_iter, converged=0, J=1.5, mu=0.25)

    def ilqr_gains(self, cfg, flats, x0, lane, target_vel, use_exo, us, mu, grid=None):
        assert grid is not None and len(flats) == 1
        n = len(us)
        self.gains_calls.append((np.array(us), mu))
        c = float(len(self.gains_calls))
        return dict(k=[np.full((n, 2), c)], K=[np.full((n, 2, 6), c)], dV=[np.full(n, c)], V_x=[np.full((n, 6), c)], V_xx=[np.full((n, 6, 6), c)],
                    xs=[np.zeros((n, 6))], L=[np.ones(n)], J=np.array([float(n)]), bad_node=np.array([self.bad], np.int32))

    def ilqr_policy_rollouts(self, cfg, flats, x0, lane, target_vel, use_exo, us, k, K, alpha, dx0=None, grid=None, **kw):
        self.rollouts.append((np.array(alpha), None if dx0 is None else np.array(dx0)))
        c, n = len(alpha), len(us)
        return [np.zeros((c, n, 6))], [np.zeros((c, n, 2))], [np.ones((c, n))], np.full((c, 1), float(n))


def _solver(monkeypatch, bad=-1, n=4):
    rt = _Runtime(bad)
    monkeypatch.setattr(ilqr_solver, "get_runtime", lambda: rt)
    return rt, ilqr_solver.iLQR(BicycleDynamics(0.2, 2.5)), np.arange(n * 2, dtype=np.float64).reshape(n, 2)


def test_policy_needs_a_fit_and_is_computed_once(monkeypatch):
    rt, s, us = _solver(monkeypatch)
    with pytest.raises(RuntimeError, match="no fit"):
        s.policy()
    with pytest.raises(AttributeError):                          # before a fit the gains are missing attributes, not errors
        s.k
    assert not any(hasattr(s, name) for name in ("k", "K", "dV", "V_x", "V_xx"))
    s.fit(us, _Cost(4), n_iterations=3)
    assert not rt.gains_calls                                    # lazy: nothing until somebody asks
    assert s.K.shape == (4, 2, 6) and s.k.shape == (4, 2) and s.dV.shape == (4,) and s.V_x.shape == (4, 6) and s.V_xx.shape == (4, 6, 6)
    assert len(rt.gains_calls) == 1 and rt.gains_calls[0][1] == 0.25 and np.array_equal(rt.gains_calls[0][0], us)      # the fit's mu and controls
    p = s.policy()
    assert len(rt.gains_calls) == 1 and p["mu"] == 0.25 and p["J"] == 4.0 and p["k"] is s.k
    q = s.policy(mu=2.0)                                         # another mu: its own call, the attributes stay
    assert len(rt.gains_calls) == 2 and q["mu"] == 2.0 and s.k[0, 0] == 1.0 and q["k"][0, 0] == 2.0
    s.fit(us + 1.0, _Cost(4), n_iterations=3)                    # the next fit clears them
    assert s.k[0, 0] == 3.0 and len(rt.gains_calls) == 3 and np.array_equal(rt.gains_calls[2][0], us + 1.0)
    with pytest.raises(AttributeError):
        s.no_such_attribute
    for bad_mu in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="mu must be"):
            s.policy(mu=bad_mu)


def test_singular_policy_raises_linalgerror(monkeypatch):
    rt, s, us = _solver(monkeypatch, bad=3)
    s.fit(us, _Cost(4))
    with pytest.raises(np.linalg.LinAlgError, match="node 3"):
        s.policy()
    with pytest.raises(np.linalg.LinAlgError):
        s.K
    with pytest.raises(np.linalg.LinAlgError):
        s.rollout_policy(1.0)


def test_rollout_policy_arguments(monkeypatch):
    rt, s, us = _solver(monkeypatch)
    s.fit(us, _Cost(4))
    xs, un, L, J = s.rollout_policy(0.5)
    assert xs.shape == (4, 6) and un.shape == (4, 2) and L.shape == (4,) and J == 4.0
    xs, un, L, J = s.rollout_policy([1.0, 0.5, 0.0], dx0=[0.1, 0, 0, 0, 0, 0])
    assert xs.shape == (3, 4, 6) and un.shape == (3, 4, 2) and L.shape == (3, 4) and J.shape == (3,)
    assert rt.rollouts[-1][1].shape == (3, 6) and np.all(rt.rollouts[-1][1][:, 0] == 0.1)
    assert len(rt.gains_calls) == 1
    for bad_alpha in ([], [[1.0]]):
        with pytest.raises(ValueError, match="alpha must be"):
            s.rollout_policy(bad_alpha)
    with pytest.raises(ValueError, match="dx0 must be"):
        s.rollout_policy([1.0, 0.5], dx0=np.zeros((3, 6)))
    with pytest.raises(ValueError, match="dx0 must be"):
        s.rollout_policy(1.0, dx0=np.zeros(5))
