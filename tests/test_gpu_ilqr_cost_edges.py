"""GPU: the planner-mode cost of the tree-iLQR at its edges -- crowded window cells, grids other than 0.4 m x 256 x 256, exact rounding ties
and border placements, a far origin, degenerate inputs (tests/ilqr_cost_cases.py; tests/test_ilqr_cost_cases_host.py proves on the oracle
what each family can catch).  Evaluation entries are held to the float64 C oracle bit for bit, the scoring, gains and rollout entries with
the comparisons and bars of tests/test_gpu_ilqr_score.py and tests/test_gpu_ilqr_policy.py, solves with those of
tests/test_gpu_random_sweep.py and test_iteration_trace_equals_the_oracles."""
import numpy as np
import pytest

import ilqr_cost_cases as cc
import ilqr_policy_restate as rs
from oracle import ilqr as oi
from test_gpu_ilqr_policy import _assert_gains_equal, _gains, _rollouts
from test_gpu_ilqr_score import _check_node_costs

pytestmark = pytest.mark.gpu
EVAL_IDS = cc.case_ids()
ENTRY_IDS = [i for i in EVAL_IDS if i[0] in ("crowd", "grids")]
SOLVE_IDS = [i for i in EVAL_IDS if i[0] in ("crowd", "grids", "far")]
KEYS = ("l", "l_x", "l_u", "l_xx", "l_uu")


def _scene(c):
    return dict(flat=c["flat"], x0=c["x0"], lane=c["lane"], tv=c["tv"], M=c["M"])


def _cfg1(c):
    return cc.copy_cfg(c["cfg"], max_iter=1)


@pytest.mark.parametrize("fam,name", EVAL_IDS)
def test_cost_eval_equals_the_oracle(fam, name, hip_predictor):
    """mind_cost_eval in planner mode against oracle.ilqr.node_derivs: l, l_x, l_u, l_xx, l_uu bit for bit at every node's perturbed state of
    the oracle's three-iteration solve and at the family's own query points"""
    c = cc.get(fam, name)
    node, x, u, want = cc.eval_points(c)
    got = hip_predictor.cost_eval(c["cfg"], node, x, u, c["flat"], x0=c["x0"], lane=c["lane"], target_vel=c["tv"], use_exo=1)
    keep = np.setdiff1d(np.arange(len(node)), np.asarray(cc.NAN_QUERIES.get(fam, {}).get(name, []), int))
    worst = 0.0
    for k in KEYS:
        g, w = got[k][keep].reshape(len(keep), -1), want[k][keep].reshape(len(keep), -1)
        d = np.abs(g - w).max() if g.size else 0.0
        worst = max(worst, float(d))
        print(f"{fam} {name} {k}: max |device - oracle| = {d:.3e}")
    for k in KEYS:
        g, w = got[k][keep].reshape(len(keep), -1), want[k][keep].reshape(len(keep), -1)
        if not np.array_equal(g, w):
            q = int(np.argmax((g != w).any(1)))
            raise AssertionError(f"family {fam} case {name} query {keep[q]} node {node[keep[q]]} at ({x[keep[q], 0]!r}, {x[keep[q], 1]!r}): first differing "
                                 f"quantity {k}: device {g[q].tolist()} oracle {w[q].tolist()} (largest difference of the case {worst:.3e})")


_score = {}


def _score_case(hp, c):
    """as tests/test_gpu_ilqr_score.py _case: the controls of a six-iteration solve and three candidates -- those controls, zeros, those
    controls plus noise of scale 1 -- scored in one call"""
    key = (c["family"], c["name"])
    if key not in _score:
        cfg, flat, x0, lane, tv, M = c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], c["M"]
        xs, us, _ = hp.ilqr_solve(cfg, [flat], x0, lane, tv, 1)
        rng = np.random.default_rng(17)
        cands = np.stack([us[0], np.zeros((M, 2)), us[0] + rng.normal(size=(M, 2))])
        sxs, sL, sJ = hp.ilqr_score(cfg, [flat], x0, lane, tv, 1, cands)
        _score[key] = dict(cfg=cfg, flat=flat, x0=x0, lane=lane, tv=tv, M=M, xs_star=xs[0], us_star=us[0], cands=cands, xs=sxs[0], L=sL[0], J=sJ[:, 0], use_exo=1)
    return _score[key]


@pytest.mark.parametrize("fam,name", ENTRY_IDS)
def test_score_trees_node_costs_and_sums(fam, name, hip_predictor):
    """mind_ilqr_score_trees: node costs are mind_cost_eval's bits and the oracle's; the sum is what a one-iteration solve reports"""
    c = cc.get(fam, name)
    s = _score_case(hip_predictor, c)
    assert np.all(np.isfinite(s["xs"])) and np.all(np.isfinite(s["L"]))
    try:
        _check_node_costs(hip_predictor, s)
    except AssertionError as e:
        for k in range(len(s["cands"])):
            want = oi.node_derivs(s["cfg"], s["flat"], s["x0"], s["lane"], s["tv"], 1, s["xs"][k], s["cands"][k])["l"]
            if not np.array_equal(s["L"][k], want):
                i = int(np.argmax(s["L"][k] != want))
                raise AssertionError(f"family {fam} case {name} candidate {k} node {i}: first differing quantity L: device {s['L'][k][i]!r} oracle {want[i]!r} "
                                     f"(largest difference {np.abs(s['L'][k] - want).max():.3e})") from e
        raise AssertionError(f"family {fam} case {name}: score L differs from mind_cost_eval's l") from e
    cfg1 = _cfg1(c)
    for k, us_c in enumerate(s["cands"]):             # as _check_sums, with this case's grid in the one-iteration configuration
        one = hip_predictor.ilqr_solve(cfg1, [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us_init=[us_c])[2][0]["J"]
        ref = oi.solve(cfg1, s["flat"], s["x0"], s["lane"], s["tv"], 1, us_init=us_c)["J"]
        print(f"{fam} {name} candidate {k}: J {s['J'][k]!r} one-iteration solve {one!r} oracle {ref!r}")
        assert s["J"][k] == one, (fam, name, "J", k, s["J"][k], one)
        assert abs(s["J"][k] - ref) < 1e-8 * max(1.0, abs(s["J"][k])), (fam, name, "J", k, s["J"][k], ref)


@pytest.mark.parametrize("fam,name", ENTRY_IDS)
def test_gains_equal_the_restatement(fam, name, hip_predictor):
    """mind_ilqr_gains about the oracle's contingency controls: k, K, dV, V_x, V_xx, xs, L bit for bit at mu = 1, 0.5 and 0; J is what a
    one-iteration solve reports"""
    c = cc.get(fam, name)
    s, cfg1 = _scene(c), _cfg1(c)
    us = cc.oracle_of(c)["full"]["us"]
    one = hip_predictor.ilqr_solve(cfg1, [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us_init=[us])[2][0]["J"]
    for mu in (1.0, 0.5, 0.0):
        got = _gains(hip_predictor, s, 1, us, mu, cfg=cfg1)
        want = rs.gains_of(s, 1, us, mu, cfg=cfg1)
        assert want["bad"] == -1 and got["bad_node"][0] == -1, (fam, name, mu)
        try:
            _assert_gains_equal(got, want)
        except AssertionError as e:
            for q in ("xs", "L", "V_x", "V_xx", "k", "K", "dV"):
                g, w = got[q][0].reshape(s["M"], -1), want[q].reshape(s["M"], -1)
                if not np.array_equal(g, w):
                    i = int(np.argmax((g != w).any(1)))
                    raise AssertionError(f"family {fam} case {name} mu {mu} node {i}: first differing quantity {q} (largest difference {np.abs(g - w).max():.3e})") from e
            raise
        assert got["J"][0] == one, (fam, name, mu, got["J"][0], one)


@pytest.mark.parametrize("fam,name", ENTRY_IDS)
def test_policy_rollouts_equal_the_restatement(fam, name, hip_predictor):
    """mind_ilqr_policy_rollouts as test_perturbed_starts_equal_the_restatement: dx0 = +-(0.3, -0.2, 0.5, 0.02, 0, 0) and zeros, alpha 0 and 1"""
    c = cc.get(fam, name)
    s, cfg1 = _scene(c), _cfg1(c)
    us = cc.oracle_of(c)["full"]["us"]
    g = _gains(hip_predictor, s, 1, us, 1.0, cfg=cfg1)
    d = np.array([0.3, -0.2, 0.5, 0.02, 0.0, 0.0])
    dx0 = np.stack([d, -d, np.zeros(6)] * 2)
    alpha = np.array([0.0] * 3 + [1.0] * 3)
    xs, un, L, J = _rollouts(hip_predictor, s, 1, us, g["k"][0], g["K"][0], alpha, dx0, cfg=cfg1)
    for q in range(6):
        xr, ur = rs.policy(cfg1, s["flat"]["parent"], s["x0"], g["xs"][0], us, g["k"][0], g["K"][0], alpha[q], dx0[q])
        assert np.array_equal(xs[0][q], xr), (fam, name, "xs", q, np.abs(xs[0][q] - xr).max())
        assert np.array_equal(un[0][q], ur), (fam, name, "us", q, np.abs(un[0][q] - ur).max())
        want_L = oi.node_derivs(cfg1, s["flat"], s["x0"], s["lane"], s["tv"], 1, xr, ur)["l"]
        if not np.array_equal(L[0][q], want_L):
            i = int(np.argmax(L[0][q] != want_L))
            raise AssertionError(f"family {fam} case {name} candidate {q} node {i}: first differing quantity L: device {L[0][q][i]!r} oracle {want_L[i]!r} "
                                 f"(largest difference {np.abs(L[0][q] - want_L).max():.3e})")
        assert J[q, 0] == rs.seq_sum(want_L), (fam, name, "J", q)


def _same_trace(got, ref, what):
    """as test_iteration_trace_equals_the_oracles: the decisions exactly, the costs to the last bits"""
    assert got.shape == ref.shape, (what, "trace rows", got.shape, ref.shape)
    for r in range(len(ref)):
        assert np.array_equal(got[r, [0, 2]], ref[r, [0, 2]]), (what, f"trace row {r}: mu / accepted step", got[r].tolist(), ref[r].tolist())
        assert np.allclose(got[r, [1, 3]], ref[r, [1, 3]], rtol=1e-13, atol=0.0), (what, f"trace row {r}: J", got[r].tolist(), ref[r].tolist())


def _same_solution(xs, us, st, ref, what):
    """the bars of test_random_scenario_trees_match_oracle"""
    assert st["iterations"] == ref["iterations"], (what, "iterations", st["iterations"], ref["iterations"])
    assert st["mu"] == ref["mu"], (what, "mu", st["mu"], ref["mu"])
    scale = max(1.0, float(np.abs(ref["xs"]).max()))
    dx = np.abs(xs - ref["xs"]).max(1)
    print(f"{what}: max |xs - oracle| = {dx.max():.3e} (bar {1e-9 * scale:.1e}), |us - oracle| = {np.abs(us - ref['us']).max():.3e}, "
          f"|J - oracle| = {abs(st['J'] - ref['J']):.3e}")
    assert dx.max() < 1e-9 * scale, (what, f"node {int(np.argmax(dx))}: first differing quantity xs", float(dx.max()))
    du = np.abs(us - ref["us"]).max(1)
    assert du.max() < 1e-9 * max(1.0, float(np.abs(ref["us"]).max())), (what, f"node {int(np.argmax(du))}: us", float(du.max()))
    assert abs(st["J"] - ref["J"]) < 1e-9 * max(1.0, abs(ref["J"])), (what, "J", st["J"], ref["J"])


@pytest.mark.parametrize("fam,name", SOLVE_IDS)
def test_contingency_follows_the_oracle(fam, name, hip_predictor):
    """mind_ilqr_contingency with max_iter = 6 against the oracle's warm fit followed by its full fit: iterations, mu, the iteration trace row
    for row, xs / us / J.  On the grids also the plain full fit from zero controls: its first steps are metres long, which is where a
    relevant-agent list that is too short shows."""
    hp = hip_predictor
    c = cc.get(fam, name)
    o = cc.oracle_of(c)
    what = f"family {fam} case {name}"
    xs, us, sw, sf = hp.ilqr_contingency(o["cfg_w"], c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"])
    traces = [hp.ilqr_trace(0, 0), hp.ilqr_trace(0, 1)]
    assert sw[0]["iterations"] == o["warm"]["iterations"] and sw[0]["mu"] == o["warm"]["mu"], (what, "warm fit", sw[0], o["warm"]["iterations"], o["warm"]["mu"])
    _same_trace(traces[0], o["warm"]["trace"], what + " warm fit")
    _same_trace(traces[1], o["full"]["trace"], what + " full fit")
    _same_solution(xs[0], us[0], sf[0], o["full"], what + " full fit")
    if fam == "grids":
        ref = oi.solve(c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], 1, trace=True)
        pxs, pus, pst = hp.ilqr_solve(c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"], 1)
        _same_trace(hp.ilqr_trace(0, 0), ref["trace"], what + " fit from zero controls")
        _same_solution(pxs[0], pus[0], pst[0], ref, what + " fit from zero controls")


def test_crowd_of_128_on_one_and_on_several_workgroups(hip_predictor):
    """the 128-agent case on one workgroup, on four workgroups per tree and in the default form (slots on follower workgroups): bit-identical"""
    hp = hip_predictor
    c = cc.get("crowd", "a128_chain")
    o = cc.oracle_of(c)
    res = {}
    try:
        hp.set_tuning("ilqr_slots", 1)
        res[1] = hp.ilqr_contingency(o["cfg_w"], c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"]) + (hp.ilqr_trace(0, 1),)
        assert hp.ilqr_stats()[2] == 1
        hp.set_tuning("ilqr_multi_min", 8)
        hp.set_tuning("ilqr_wgs", 4)
        res[4] = hp.ilqr_contingency(o["cfg_w"], c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"]) + (hp.ilqr_trace(0, 1),)
        assert hp.ilqr_stats()[2] == 4
    finally:
        hp.set_tuning("ilqr_slots", 10)
        hp.set_tuning("ilqr_multi_min", 192)
        hp.set_tuning("ilqr_wgs", 16)
    res[0] = hp.ilqr_contingency(o["cfg_w"], c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"]) + (hp.ilqr_trace(0, 1),)
    assert hp.ilqr_stats()[2] > 1
    for G in (4, 0):
        for q, a, b in zip(("xs", "us"), res[G][:2], res[1][:2]):
            assert np.array_equal(a[0], b[0]), ("crowd a128_chain", G, q, np.abs(a[0] - b[0]).max())
        assert res[G][2] == res[1][2] and res[G][3] == res[1][3], ("crowd a128_chain", G, "statistics", res[G][2:4], res[1][2:4])
        assert np.array_equal(res[G][4], res[1][4]), ("crowd a128_chain", G, "trace")
