"""GPU: the tree-iLQR kernels at start-state, heading and lane edges (tests/ilqr_state_cases.py; tests/test_ilqr_state_cases_host.py proves on
the oracle what each family reaches and which cases are conditioned well enough for solve-level assertions).  Every comparison and every bar
is one the project already has: evaluation, scoring, gains and rollouts are held to the float64 C oracle and to the plain-Python
restatement bit for bit as in tests/test_gpu_ilqr_cost_edges.py, solves with ``_same_trace`` / ``_same_solution`` of that file.

Every test prints one line ``family name entry max|device - oracle|`` per case; profiles/ilqr_state_edges.txt is that table from an MI355X."""
import numpy as np
import pytest

import ilqr_policy_restate as rs
import ilqr_state_cases as sc
from oracle import ilqr as oi
from test_gpu_ilqr_cost_edges import KEYS, _cfg1, _same_solution, _same_trace, _scene
from test_gpu_ilqr_policy import GAIN_KEYS, _assert_gains_equal, _gains, _rollouts
from test_gpu_ilqr_score import _check_node_costs

pytestmark = pytest.mark.gpu
EVAL_IDS = sc.case_ids()
SOLVE_IDS = sc.solve_ids()
FORM_IDS = [("heading", "mixed"), ("speed", "v0_tv4"), ("limits", "a_under"), ("lanes", "dup_mid")]
KNOBS = ("ilqr_slots", "ilqr_multi_min", "ilqr_wgs", "ilqr_spec_deriv")


def _line(fam, name, entry, worst):
    print(f"{fam} {name} {entry} {worst:.3e}")


@pytest.mark.parametrize("fam,name", EVAL_IDS)
def test_cost_eval_equals_the_oracle(fam, name, hip_predictor):
    """mind_cost_eval in planner mode against oracle.ilqr.node_derivs: l, l_x, l_u, l_xx, l_uu bit for bit at every node's perturbed state of
    the oracle's three-iteration solve and at the edge queries (every bound and one ulp either side, headings k pi / 4 +- 1 ulp, v = +-0)"""
    c = sc.get(fam, name)
    node, x, u, want = sc.eval_points(c)
    got = hip_predictor.cost_eval(c["cfg"], node, x, u, c["flat"], x0=c["x0"], lane=c["lane"], target_vel=c["tv"], use_exo=1)
    keep = np.setdiff1d(np.arange(len(node)), np.asarray(sc.NAN_QUERIES.get(fam, {}).get(name, []), int))
    diff = {k: np.abs(got[k][keep].reshape(len(keep), -1) - want[k][keep].reshape(len(keep), -1)) for k in KEYS}
    worst = max(float(d.max()) for d in diff.values())
    _line(fam, name, "cost_eval", worst)
    for k in KEYS:
        g, w = got[k][keep].reshape(len(keep), -1), want[k][keep].reshape(len(keep), -1)
        if not np.array_equal(g, w):
            q = int(np.argmax((g != w).any(1)))
            raise AssertionError(f"family {fam} case {name} query {keep[q]} node {node[keep[q]]} at state {x[keep[q]].tolist()}: first differing "
                                 f"quantity {k}: device {g[q].tolist()} oracle {w[q].tolist()} (largest difference of the case {worst:.3e})")


@pytest.mark.parametrize("fam,name", EVAL_IDS)
def test_score_trees_states_node_costs_and_sums(fam, name, hip_predictor):
    """mind_ilqr_score_trees on the solver's own controls, zeros and those controls plus noise of scale 1: xs of the first candidate are the
    solver's bits, L is mind_cost_eval's bits and the oracle's, J is what a one-iteration solve reports"""
    hp = hip_predictor
    c = sc.get(fam, name)
    cfg, flat, x0, lane, tv, M = c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], c["M"]
    xs, us, _ = hp.ilqr_solve(cfg, [flat], x0, lane, tv, 1)
    cands = np.stack([us[0], np.zeros((M, 2)), us[0] + np.random.default_rng(17).normal(size=(M, 2))])
    sxs, sL, sJ = hp.ilqr_score(cfg, [flat], x0, lane, tv, 1, cands)
    s = dict(cfg=cfg, flat=flat, x0=x0, lane=lane, tv=tv, M=M, cands=cands, xs=sxs[0], L=sL[0], J=sJ[:, 0], use_exo=1)
    assert np.all(np.isfinite(s["xs"])) and np.all(np.isfinite(s["L"])), (fam, name)
    wants = [oi.node_derivs(cfg, flat, x0, lane, tv, 1, s["xs"][k], cands[k])["l"] for k in range(3)]
    _line(fam, name, "score", max(float(np.abs(s["L"][k] - wants[k]).max()) for k in range(3)))
    if not np.array_equal(s["xs"][0], xs[0]):
        i = int(np.argmax((s["xs"][0] != xs[0]).any(1)))
        raise AssertionError(f"family {fam} case {name} node {i}: first differing quantity xs: score {s['xs'][0][i].tolist()} solver {xs[0][i].tolist()}")
    for k in range(3):
        if not np.array_equal(s["L"][k], wants[k]):
            i = int(np.argmax(s["L"][k] != wants[k]))
            raise AssertionError(f"family {fam} case {name} candidate {k} node {i}: first differing quantity L: device {s['L'][k][i]!r} oracle {wants[k][i]!r} "
                                 f"(largest difference {np.abs(s['L'][k] - wants[k]).max():.3e})")
    _check_node_costs(hp, s)
    cfg1 = _cfg1(c)
    for k, us_c in enumerate(cands):
        one = hp.ilqr_solve(cfg1, [flat], x0, lane, tv, 1, us_init=[us_c])[2][0]["J"]
        ref = oi.solve(cfg1, flat, x0, lane, tv, 1, us_init=us_c)["J"]
        assert s["J"][k] == one, (fam, name, "J", k, s["J"][k], one)
        assert abs(s["J"][k] - ref) < 1e-8 * max(1.0, abs(s["J"][k])), (fam, name, "J", k, s["J"][k], ref)


@pytest.mark.parametrize("fam,name", EVAL_IDS)
def test_gains_equal_the_restatement(fam, name, hip_predictor):
    """mind_ilqr_gains about the oracle's contingency controls: k, K, dV, V_x, V_xx, xs, L bit for bit at mu = 1, 0.5 and 0; a singular Q_uu is
    reported at the node the restatement reports; J is what a one-iteration solve reports"""
    c = sc.get(fam, name)
    s, cfg1 = _scene(c), _cfg1(c)
    us = sc.oracle_of(c)["full"]["us"]
    one = hip_predictor.ilqr_solve(cfg1, [s["flat"]], s["x0"], s["lane"], s["tv"], 1, us_init=[us])[2][0]["J"]
    worst = 0.0
    for mu in (1.0, 0.5, 0.0):
        got = _gains(hip_predictor, s, 1, us, mu, cfg=cfg1)
        want = rs.gains_of(s, 1, us, mu, cfg=cfg1)
        assert got["bad_node"][0] == want["bad"], (fam, name, mu, "singular Q_uu: node", int(got["bad_node"][0]), want["bad"])
        worst = max([worst] + [float(np.abs(got[q][0] - want[q]).max()) for q in GAIN_KEYS])
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
    _line(fam, name, "gains", worst)


@pytest.mark.parametrize("fam,name", EVAL_IDS)
def test_policy_rollouts_equal_the_restatement(fam, name, hip_predictor):
    """mind_ilqr_policy_rollouts as test_perturbed_starts_equal_the_restatement: dx0 = +-(0.3, -0.2, 0.5, 0.02, 0, 0) and zeros, alpha 0 and 1"""
    c = sc.get(fam, name)
    s, cfg1 = _scene(c), _cfg1(c)
    us = sc.oracle_of(c)["full"]["us"]
    g = _gains(hip_predictor, s, 1, us, 1.0, cfg=cfg1)
    d = np.array([0.3, -0.2, 0.5, 0.02, 0.0, 0.0])
    dx0 = np.stack([d, -d, np.zeros(6)] * 2)
    alpha = np.array([0.0] * 3 + [1.0] * 3)
    xs, un, L, J = _rollouts(hip_predictor, s, 1, us, g["k"][0], g["K"][0], alpha, dx0, cfg=cfg1)
    ref = [rs.policy(cfg1, s["flat"]["parent"], s["x0"], g["xs"][0], us, g["k"][0], g["K"][0], alpha[q], dx0[q]) for q in range(6)]
    _line(fam, name, "policy", max(max(float(np.abs(xs[0][q] - ref[q][0]).max()), float(np.abs(un[0][q] - ref[q][1]).max())) for q in range(6)))
    for q in range(6):
        xr, ur = ref[q]
        for what, a, b in (("xs", xs[0][q], xr), ("us", un[0][q], ur)):
            if not np.array_equal(a, b):
                i = int(np.argmax((a != b).any(1)))
                raise AssertionError(f"family {fam} case {name} candidate {q} node {i}: first differing quantity {what}: device {a[i].tolist()} "
                                     f"restatement {b[i].tolist()} (largest difference {np.abs(a - b).max():.3e})")
        want_L = oi.node_derivs(cfg1, s["flat"], s["x0"], s["lane"], s["tv"], 1, xr, ur)["l"]
        if not np.array_equal(L[0][q], want_L):
            i = int(np.argmax(L[0][q] != want_L))
            raise AssertionError(f"family {fam} case {name} candidate {q} node {i}: first differing quantity L: device {L[0][q][i]!r} oracle {want_L[i]!r} "
                                 f"(largest difference {np.abs(L[0][q] - want_L).max():.3e})")
        assert J[q, 0] == rs.seq_sum(want_L), (fam, name, "J", q)


@pytest.mark.parametrize("fam,name", SOLVE_IDS)
def test_contingency_follows_the_oracle(fam, name, hip_predictor):
    """mind_ilqr_contingency against the oracle's warm fit followed by its full fit, and the plain full fit from zero controls: iterations,
    mu, the iteration trace row for row (decisions exact, J at rtol 1e-13), xs / us / J with the bars of the random sweep"""
    hp = hip_predictor
    c = sc.get(fam, name)
    o = sc.oracle_of(c)
    what = f"family {fam} case {name}"
    xs, us, sw, sf = hp.ilqr_contingency(o["cfg_w"], c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"])
    traces = [hp.ilqr_trace(0, 0), hp.ilqr_trace(0, 1)]
    _line(fam, name, "contingency", float(np.abs(xs[0] - o["full"]["xs"]).max()))
    assert sw[0]["iterations"] == o["warm"]["iterations"] and sw[0]["mu"] == o["warm"]["mu"], (what, "warm fit", sw[0], o["warm"]["iterations"], o["warm"]["mu"])
    _same_trace(traces[0], o["warm"]["trace"], what + " warm fit")
    _same_trace(traces[1], o["full"]["trace"], what + " full fit")
    _same_solution(xs[0], us[0], sf[0], o["full"], what + " full fit")
    ref = oi.solve(c["cfg"], c["flat"], c["x0"], c["lane"], c["tv"], 1, trace=True)
    pxs, pus, pst = hp.ilqr_solve(c["cfg"], [c["flat"]], c["x0"], c["lane"], c["tv"], 1)
    _line(fam, name, "plain_fit", float(np.abs(pxs[0] - ref["xs"]).max()))
    _same_trace(hp.ilqr_trace(0, 0), ref["trace"], what + " fit from zero controls")
    _same_solution(pxs[0], pus[0], pst[0], ref, what + " fit from zero controls")


def _run(hp, o, c, flats=None):
    r = hp.ilqr_contingency(o["cfg_w"], c["cfg"], flats or [c["flat"]], c["x0"], c["lane"], c["tv"])
    n = len(flats or [0])
    return r + ([hp.ilqr_trace(t, 0) for t in range(n)], [hp.ilqr_trace(t, 1) for t in range(n)])


@pytest.mark.parametrize("fam,name", FORM_IDS)
def test_launch_forms_give_the_same_bits(fam, name, hip_predictor):
    """the contingency on one workgroup (ilqr_slots = 1), on four workgroups per tree (ilqr_multi_min = 8, ilqr_wgs = 4), without the
    speculative derivative pass (ilqr_spec_deriv = 0) and in the default form: xs, us, statistics and traces bit-identical"""
    hp = hip_predictor
    c = sc.get(fam, name)
    o = sc.oracle_of(c)
    before = {k: hp.get_tuning(k) for k in KNOBS}
    res = {}
    try:
        res["default"] = _run(hp, o, c)
        assert hp.ilqr_stats()[2] > 1
        hp.set_tuning("ilqr_spec_deriv", 0)
        res["no speculation"] = _run(hp, o, c)
        hp.set_tuning("ilqr_spec_deriv", before["ilqr_spec_deriv"])
        hp.set_tuning("ilqr_slots", 1)
        res["one workgroup"] = _run(hp, o, c)
        assert hp.ilqr_stats()[2] == 1
        hp.set_tuning("ilqr_multi_min", 8)
        hp.set_tuning("ilqr_wgs", 4)
        res["four workgroups"] = _run(hp, o, c)
        assert hp.ilqr_stats()[2] == 4
    finally:
        for k, v in before.items():
            hp.set_tuning(k, v)
    one = res["one workgroup"]
    for form, r in res.items():
        for q, a, b in zip(("xs", "us"), r[:2], one[:2]):
            if not np.array_equal(a[0], b[0]):
                i = int(np.argmax((a[0] != b[0]).any(1)))
                raise AssertionError(f"family {fam} case {name} form {form!r} node {i}: first differing quantity {q} (largest difference {np.abs(a[0] - b[0]).max():.3e})")
        assert r[2] == one[2] and r[3] == one[3], (fam, name, form, "statistics", r[2:4], one[2:4])
        assert np.array_equal(r[4][0], one[4][0]) and np.array_equal(r[5][0], one[5][0]), (fam, name, form, "trace")
    _line(fam, name, "launch_forms", float(np.abs(one[0][0] - o["full"]["xs"]).max()))


@pytest.mark.parametrize("host", [("heading", "rot3.0"), ("speed", "v_neg")])
def test_batched_trees_equal_the_single_launches(host, hip_predictor):
    """a launch shares one start state, lane and target speed among its cost trees: the agents of two turned cases and of one speed case,
    batched at a turned case's start and at the reversing start, equal the three single launches bit for bit"""
    hp = hip_predictor
    c = sc.get(*host)
    o = sc.oracle_of(c)
    flats = [sc.get("heading", "rot3.0")["flat"], sc.get("heading", "pi_minus")["flat"], sc.get("speed", "v_neg")["flat"]]
    assert not np.array_equal(flats[0]["mean"], flats[1]["mean"]) and not np.array_equal(flats[1]["mean"], flats[2]["mean"])
    xs, us, sw, sf, tw, tf = _run(hp, o, c, flats)
    for t, flat in enumerate(flats):
        x1, u1, w1, f1, tw1, tf1 = _run(hp, o, c, [flat])
        for q, a, b in (("xs", xs[t], x1[0]), ("us", us[t], u1[0])):
            if not np.array_equal(a, b):
                i = int(np.argmax((a != b).any(1)))
                raise AssertionError(f"family {host[0]} case {host[1]} tree {t} node {i}: first differing quantity {q} (largest difference {np.abs(a - b).max():.3e})")
        assert sw[t] == w1[0] and sf[t] == f1[0], (host, t, "statistics")
        assert np.array_equal(tw[t], tw1[0]) and np.array_equal(tf[t], tf1[0]), (host, t, "trace")
    _line(host[0], host[1], "batched", float(np.abs(xs[host == ("speed", "v_neg") and 2 or 0] - o["full"]["xs"]).max()))
