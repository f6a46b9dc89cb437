"""CPU: the C tree-iLQR oracle against golden vectors captured from the imported reference
(tests/golden/gen_golden.py: ilqr, potential) and against recorded values of the reference itself (tests/ref_golden.py)."""
import os

import numpy as np
import pytest

from mind_amd.synth import scripted_scenario_tree
from oracle import ilqr as oi
from oracle import ref_harness as rh
from ref_golden import Recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = dict(np.load(os.path.join(ROOT, "tests", "golden", "ilqr.npz")))
CASES = [("straight", 3, 100), ("lead", 4, 100), ("branch3", 6, 100), ("branch3", 40, 100), ("deep", 3, 4)]


def run_oracle(kind, a, max_iter):
    sst = scripted_scenario_tree(kind, a)
    cfg = oi.default_cfg(max_iter=max_iter)
    flat = oi.flatten(sst["nodes"])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    w = oi.solve(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 0)
    f = oi.solve(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 1, us_init=w["us"])
    return flat, w, f


@pytest.mark.parametrize("kind,a,max_iter", CASES)
def test_oracle_ilqr_matches_golden(kind, a, max_iter):
    key = f"{kind}_a{a}_it{max_iter}"
    flat, w, f = run_oracle(kind, a, max_iter)
    assert np.array_equal(flat["parent"], G[key + "_parent"])          # LIFO DFS creation order (Q13)
    # float64, same operation order as numpy up to BLAS summation order: agreement ~1e-13
    assert np.abs(w["xs"] - G[key + "_xs_w"]).max() < 1e-9
    assert np.abs(w["us"] - G[key + "_us_w"]).max() < 1e-9
    assert np.abs(f["xs"] - G[key + "_xs_f"]).max() < 1e-8
    assert np.abs(f["us"] - G[key + "_us_f"]).max() < 1e-8
    assert abs(w["J"] - G[key + "_Jw"][0]) < 1e-9 * max(1, abs(w["J"])) and w["mu"] == G[key + "_Jw"][1]
    assert abs(f["J"] - G[key + "_Jf"][0]) < 1e-9 * max(1, abs(f["J"])) and f["mu"] == G[key + "_Jf"][1]


def test_potential_field_matches_golden():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "potential.npz")))
    F, off, res = g["F"], g["off"], float(g["res"])
    for p, v in zip(g["pts"], g["vals"]):
        out = oi.field_eval(F, res, off, p[0], p[1])
        assert np.allclose(out, v, rtol=1e-12, atol=1e-12), (p, out, v)


def test_flatten_every_even_substep_and_lifo_order():
    sst = scripted_scenario_tree("branch3", 3)
    flat = oi.flatten(sst["nodes"])
    durs = {k: d[1].shape[1] for k, _, d in sst["nodes"]}
    assert len(flat["parent"]) == sum((d + 1) // 2 for d in durs.values())
    assert flat["parent"][0] == -1 and all(flat["parent"][1:] < np.arange(1, len(flat["parent"])))
    # root scenario node has 16 steps -> 8 trajectory nodes; the LAST child ("1_0_4") is expanded first
    assert flat["parent"][8] == 7 and np.isclose(flat["prob"][8], 0.094)


@pytest.mark.reference
def test_oracle_matches_imported_reference_live():
    sst = scripted_scenario_tree("lead", 5, seed=3)

    def ref():
        m = rh.ref_modules()
        Tree, Node = m["planners.basic.tree"].Tree, m["planners.basic.tree"].Node
        TTO = m["planners.mind.trajectory_tree"].TrajectoryTreeOptimizer
        cfgmod = m["planners.mind.configs.planning.demo_1"]
        tree = Tree()
        for k, p, d in sst["nodes"]:
            tree.add_node(Node(k, p, d))
        opt = TTO(cfgmod.TrajTreeCfg())
        opt.init_warm_start_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
        xs_w, us_w = opt.warm_start_solve()
        opt.init_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
        opt.solve(us_w)
        return np.array(xs_w), np.array(opt.ilqr.xs), float(opt.ilqr._mu)
    xs_w, xs_f, mu = Recorded("oracle_ilqr_live")("lead5", ref)
    flat, w, f = oi.contingency(oi.default_cfg(), sst["nodes"], sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
    assert np.abs(w["xs"] - xs_w).max() < 1e-9 and np.abs(f["xs"] - xs_f).max() < 1e-8
    assert f["mu"] == mu


@pytest.mark.reference
@pytest.mark.parametrize("kind,a", [("lead", 5), ("branch3", 6)])
def test_oracle_iteration_trace_equals_the_imported_references(kind, a):
    """iLQR.fit's loop (planners/ilqr/solver.py:133-158) ITERATION BY ITERATION: the Levenberg-Marquardt value every backward pass runs
    with, the cost of the nominal trajectory when the line search starts and its outcome, recorded by wrapping the imported reference's
    _backward_pass / _backtrack_line_search, against the rows of the C oracle's loop (oracle_ilqr_last_trace; the same rows come out of
    the HIP kernel through mind_last_ilqr_trace: tests/test_gpu_ilqr.py::test_iteration_trace_equals_the_oracles)."""
    sst = scripted_scenario_tree(kind, a, seed=3)

    def ref():
        m = rh.ref_modules()
        Tree, Node = m["planners.basic.tree"].Tree, m["planners.basic.tree"].Node
        TTO = m["planners.mind.trajectory_tree"].TrajectoryTreeOptimizer
        iLQR = m["planners.ilqr.solver"].iLQR
        cfgmod = m["planners.mind.configs.planning.demo_1"]
        tree = Tree()
        for k, p, d in sst["nodes"]:
            tree.add_node(Node(k, p, d))
        fits = []
        o_bp, o_ls, o_fit = iLQR._backward_pass, iLQR._backtrack_line_search, iLQR.fit

        def bp(self):
            fits[-1].append([float(self._mu), float(self.J_opt), -2.0])
            return o_bp(self)

        def ls(self, alphas):
            acc, conv = o_ls(self, alphas)
            fits[-1][-1][2] = 1.0 if acc else -1.0
            return acc, conv

        def fit(self, *args, **kw):
            fits.append([])
            return o_fit(self, *args, **kw)

        iLQR._backward_pass, iLQR._backtrack_line_search, iLQR.fit = bp, ls, fit
        try:
            opt = TTO(cfgmod.TrajTreeCfg())
            opt.init_warm_start_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
            xs_w, us_w = opt.warm_start_solve()
            opt.init_cost_tree(tree, sst["state"], sst["ctrl"], sst["target_lane"], sst["target_vel"])
            opt.solve(us_w)
        finally:
            iLQR._backward_pass, iLQR._backtrack_line_search, iLQR.fit = o_bp, o_ls, o_fit
        return fits
    fits = Recorded("oracle_ilqr_trace")(f"{kind}{a}", ref)
    cfg = oi.default_cfg()
    flat = oi.flatten(sst["nodes"])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    w = oi.solve(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 0, trace=True)
    f = oi.solve(cfg, flat, x0, sst["target_lane"], sst["target_vel"], 1, us_init=w["us"], trace=True)
    for got, ref in ((w["trace"], np.array(fits[0])), (f["trace"], np.array(fits[1]))):
        assert len(got) == len(ref) and len(ref) > 3
        assert np.array_equal(got[:, 0], ref[:, 0])                                           # the Levenberg-Marquardt schedule
        assert np.array_equal(np.where(got[:, 2] >= 0, 1.0, got[:, 2]), ref[:, 2])            # accepted / rejected / singular
        assert np.allclose(got[:, 1], ref[:, 1], rtol=1e-9, atol=0.0)                         # cost of the nominal trajectory


@pytest.mark.parametrize("kind,a,max_iter", CASES)
def test_oracle_with_the_c_librarys_trigonometry_meets_the_same_goldens(kind, a, max_iter):
    """Kernel == oracle bit for bit rests on ONE trigonometry routine both include (mind_amd/csrc/mind_trig.h).  The independent witness: the same
    oracle built with the C library's sin / cos / tan (what numpy calls in the reference; oracle/Makefile libilqr_oracle_libm.so) meets the
    reference goldens at the same tolerances, and the shared-header build stays within 1e-9 of it -- a defect of the header would show in
    both comparisons (it cannot cancel on the two sides of a kernel-vs-oracle test)."""
    key = f"{kind}_a{a}_it{max_iter}"
    flat, w, f = run_oracle(kind, a, max_iter)
    with oi.libm_trig():
        flat2, w2, f2 = run_oracle(kind, a, max_iter)
    assert np.abs(w2["xs"] - G[key + "_xs_w"]).max() < 1e-9 and np.abs(w2["us"] - G[key + "_us_w"]).max() < 1e-9
    assert np.abs(f2["xs"] - G[key + "_xs_f"]).max() < 1e-8 and np.abs(f2["us"] - G[key + "_us_f"]).max() < 1e-8
    assert w2["mu"] == G[key + "_Jw"][1] and f2["mu"] == G[key + "_Jf"][1] and w2["iterations"] == w["iterations"] and f2["iterations"] == f["iterations"]
    assert np.abs(w2["xs"] - w["xs"]).max() < 1e-9 and np.abs(f2["xs"] - f["xs"]).max() < 1e-8
    assert np.abs(w2["us"] - w["us"]).max() < 1e-9 and np.abs(f2["us"] - f["us"]).max() < 1e-8
