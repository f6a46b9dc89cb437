"""CPU: the start-state, heading and lane cases of tests/ilqr_state_cases.py reach what they are named for and the oracle is a valid witness
on them, proven on the oracle alone.

Conditioning rule for solve-level assertions: a case is in ``solve_ids()`` only if (a) the oracle built on the shared header mind_trig.h and
the one built on the C library's sin / cos / tan give the same (mu, accepted step) trace rows for the warm fit, the full fit behind it and the plain full fit from zero controls -- the three
fits the GPU test asserts; the last goes beyond what the rule has to cover, and four starts are stiff only there --, and (b) under
x0[2:] *= 1 +- 1e-13 those rows stay the same, xs moves by less than 1e-10 max(1, |xs|max) -- a tenth of the 1e-9 bar the device solve is
held to -- and J by less than 10 x 1e-13 relative.  A case may run with max_iter 4, 3 or 2 to meet it (the largest that does, recorded in
``MAX_ITER``); one that meets it at none is evaluation-only and listed in ``ILL_CONDITIONED``."""
import numpy as np
import pytest

import ilqr_cost_cases as cc
import ilqr_state_cases as sc
from oracle import ilqr as oi

PI4 = np.pi / 4
STEPS = (6, 4, 3, 2)


def _fits(c, cfg, x0):
    """the three fits the GPU test asserts: the warm fit, the full fit behind it, the plain full fit from zero controls"""
    cfg_w = cc.copy_cfg(cfg, w_ego=0.0, w_exo=0.0)
    w = oi.solve(cfg_w, c["flat"], x0, c["lane"], c["tv"], 0, trace=True)
    f = oi.solve(cfg, c["flat"], x0, c["lane"], c["tv"], 1, us_init=w["us"], trace=True)
    p = oi.solve(cfg, c["flat"], x0, c["lane"], c["tv"], 1, trace=True)
    return w, f, p


def _rows(a, b):
    return a["trace"].shape == b["trace"].shape and np.array_equal(a["trace"][:, [0, 2]], b["trace"][:, [0, 2]])


_rule = {}


def rule(c, max_iter):
    """-> (met, rows kept, movement of xs relative to max(1, |xs|max), relative movement of J)"""
    key = (c["family"], c["name"], max_iter)
    if key not in _rule:
        cfg = cc.copy_cfg(c["cfg"], max_iter=max_iter)
        w, f, p = _fits(c, cfg, c["x0"])
        with oi.libm_trig():
            w2, f2, p2 = _fits(c, cfg, c["x0"])
        rows = _rows(w, w2) and _rows(f, f2) and _rows(p, p2)
        dx = dJ = 0.0
        for s in (1.0 + 1e-13, 1.0 - 1e-13):
            xp = c["x0"].copy()
            xp[2:] *= s
            w3, f3, p3 = _fits(c, cfg, xp)
            rows = rows and _rows(w, w3) and _rows(f, f3) and _rows(p, p3)
            for a, b in ((w, w3), (f, f3), (p, p3)):
                dx = max(dx, float(np.abs(a["xs"] - b["xs"]).max() / max(1.0, np.abs(a["xs"]).max())))
                dJ = max(dJ, abs(a["J"] - b["J"]) / abs(a["J"]))
        _rule[key] = (bool(rows and dx < 1e-10 and dJ < 10 * 1e-13), bool(rows), dx, dJ)
    return _rule[key]


@pytest.mark.parametrize("fam,name", sc.case_ids())
def test_oracle_is_finite_on_every_asserted_output(fam, name):
    c = sc.get(fam, name)
    assert c["M"] <= 40 and 4 <= c["flat"]["mean"].shape[1] <= 8
    assert (c["cfg"].grid_res, c["cfg"].grid_w, c["cfg"].grid_h) == (0.4, 256, 256)
    node, x, u, want = sc.eval_points(c)
    assert sc.NAN_QUERIES == {}
    for k, v in want.items():
        assert np.all(np.isfinite(v)), (fam, name, k)
    o = sc.oracle_of(c)                                  # the gains and rollout tests run about the full fit's controls on every case
    for ph in ("warm", "full", "sol3"):
        assert np.all(np.isfinite(o[ph]["xs"])) and np.all(np.isfinite(o[ph]["us"])) and np.isfinite(o[ph]["J"]), (fam, name, ph)
    for ph in ("warm", "full"):
        assert np.all(np.isfinite(o[ph]["trace"])), (fam, name, ph)


@pytest.mark.parametrize("fam,name", sc.solve_ids())
def test_solve_level_cases_meet_the_conditioning_rule(fam, name):
    c = sc.get(fam, name)
    mi = c["cfg"].max_iter
    assert mi == sc.MAX_ITER.get((fam, name), 6) and mi in STEPS
    met, rows, dx, dJ = rule(c, mi)
    print(f"{fam} {name} max_iter {mi}: rows kept {rows}, xs moves {dx:.1e}, J moves {dJ:.1e}")
    assert met, (fam, name, mi, rows, dx, dJ)
    if mi < 6:                                           # the largest that does
        bigger = STEPS[STEPS.index(mi) - 1]
        assert not rule(c, bigger)[0], (fam, name, bigger)


@pytest.mark.parametrize("fam,name", sorted(sc.ILL_CONDITIONED))
def test_evaluation_only_cases_fail_the_rule_at_every_max_iter(fam, name):
    c = sc.get(fam, name)
    assert not c["solve"]
    for mi in STEPS:
        met, rows, dx, dJ = rule(c, mi)
        print(f"{fam} {name} max_iter {mi}: rows kept {rows}, xs moves {dx:.1e}, J moves {dJ:.1e}")
        assert not met, (fam, name, mi)
    for (rows_t, dx_t, dJ_t), mi in zip(sc.ILL_CONDITIONED[(fam, name)], (6, 2)):      # the table is what was measured (to its two digits)
        met, rows, dx, dJ = rule(c, mi)
        assert rows == rows_t and 0.3 * dx_t <= dx <= 3.0 * dx_t and 0.3 * dJ_t <= dJ <= 3.0 * dJ_t, (fam, name, mi, rows, dx, dJ)


def test_caps_on_evaluation_only_cases():
    ids, solve = sc.case_ids(), sc.solve_ids()
    assert set(ids) - set(solve) == set(sc.ILL_CONDITIONED)
    assert len(ids) - len(solve) <= len(ids) / 4, (len(ids), len(solve))
    for fam in sc.FAMILIES:
        assert sum(1 for f, _ in solve if f == fam) >= 2, fam
    assert set(sc.MAX_ITER) <= set(solve) and all(v in (4, 3, 2) for v in sc.MAX_ITER.values())


def _solves():
    return [(c, sc.oracle_of(c)) for c in sc.all_cases() if c["solve"]]


def test_line_search_and_regulariser_paths_are_reached():
    """among the solve-level cases: a full fit with every pass rejected (mu grows by its schedule beyond 1e8), a fit that stops after one
    iteration, accepted step indices of 5 or more"""
    all_rejected, one_iteration, late_steps = [], [], []
    for c, o in _solves():
        key = (c["family"], c["name"])
        tr = o["full"]["trace"]
        if c["cfg"].max_iter == 6 and len(tr) == 6 and np.all(tr[:, 2] == -1):
            assert o["full"]["mu"] > 1e8
            all_rejected.append(key)
        for ph in ("warm", "full"):
            if o[ph]["iterations"] == 1 and len(o[ph]["trace"]) == 1:
                one_iteration.append(key + (ph, int(o[ph]["trace"][0, 2])))
            late_steps += [key + (ph, int(s)) for s in o[ph]["trace"][:, 2] if s >= 5]
    print("every pass rejected:", all_rejected, "\none iteration:", one_iteration, "\nstep index >= 5:", late_steps)
    assert all_rejected and one_iteration and late_steps
    assert any(s[3] >= 7 for s in late_steps)
    assert any(s[3] >= 5 for s in one_iteration)          # ... and one converges in its first iteration at a late step size


def _quadrants(xs):
    return np.rint(xs[:, 3] * 2 / np.pi).astype(int)


def test_heading_reaches_every_quadrant_and_a_mixed_level():
    """rint(theta 2 / pi) != 0 at every node of the warm and the full fit, for each of the four values of k mod 4; iterates that cross +-pi;
    |theta| > 2 pi; x0's heading within 1e-3 of pi / 4 and 3 pi / 4 on both sides; the ``mixed`` case has one tree level on both sides of
    pi / 4 in the full fit"""
    seen = set()
    for c in sc.family("heading"):
        if not c["solve"]:
            continue
        o = sc.oracle_of(c)
        k = np.concatenate([_quadrants(o["warm"]["xs"]), _quadrants(o["full"]["xs"])])
        if np.all(k != 0) and len(set((k % 4).tolist())) == 1:
            seen.add(int(k[0] % 4))
    assert seen == {0, 1, 2, 3}, seen
    get = lambda n: sc.get("heading", n)
    for n, sign in (("pi_minus", 1.0), ("neg_pi_minus", -1.0)):
        th = np.concatenate([sc.oracle_of(get(n))[ph]["xs"][:, 3] for ph in ("warm", "full", "sol3")] + [get(n)["x0"][3:4]])
        assert th.min() < sign * np.pi < th.max(), (n, th.min(), th.max())
    th = sc.oracle_of(get("neg_pi_plus"))["full"]["xs"][:, 3]      # starts 0.08 above -pi and comes within 0.01 of it from above
    assert -np.pi < th.min() < -np.pi + 0.01
    assert np.abs(sc.oracle_of(get("two_pi_plus"))["full"]["xs"][:, 3]).min() > 2 * np.pi
    assert sc.oracle_of(get("near_bound"))["full"]["xs"][:, 3].min() < -9.7 and get("near_bound")["cfg"].state_lower[3] == -10.0
    for n, t, side in (("below_pi4", PI4, -1), ("above_pi4", PI4, 1), ("below_3pi4", 3 * PI4, -1), ("above_3pi4", 3 * PI4, 1)):
        d = get(n)["x0"][3] - t
        assert 0.5e-3 < side * d < 2e-3, (n, d)
    assert get("pi2")["x0"][3] == cc.X0[3] + np.pi / 2
    c = get("mixed")
    assert c["solve"] and not np.array_equal(c["lane"][:, 1], np.full(len(c["lane"]), c["lane"][0, 1]))      # a curved lane
    dep = cc._depth(c["flat"]["parent"])
    th = sc.oracle_of(c)["full"]["xs"][:, 3]
    mixed = [int(l) for l in np.unique(dep) if th[dep == l].min() < PI4 - 1e-4 and th[dep == l].max() > PI4 + 1e-4]
    print("levels on both sides of pi / 4:", mixed)
    assert mixed


def test_rotations_keep_the_lane_only_cost():
    """a check on the case builder: the heading cases (all but ``mixed``, which has its own curved lane) are rigid motions of one base case,
    and the warm fit does not see the agents, so its J agrees with the base case's to 1e-9 relative"""
    base = sc.oracle_of(sc.get("heading", "base"))["warm"]["J"]
    for c in sc.family("heading"):
        if c["name"] == "mixed":
            continue
        J = sc.oracle_of(c)["warm"]["J"]
        print(f"heading {c['name']}: warm-fit J {J!r} (base {base!r}, relative difference {abs(J - base) / base:.1e})")
        assert abs(J - base) <= 1e-9 * base, (c["name"], J, base)
        assert np.array_equal(sc.oracle_of(c)["warm"]["trace"][:, [0, 2]], sc.oracle_of(sc.get("heading", "base"))["warm"]["trace"][:, [0, 2]])


def test_speed_and_limit_cases_reach_the_bounds():
    """among the solve-level cases' iterates: a node with v <= 0, nodes beyond each of the v, a and delta bounds on both sides; the starts are
    what their names say"""
    lo, hi = np.array(list(sc.base()["cfg"].state_lower)), np.array(list(sc.base()["cfg"].state_upper))
    below, above = set(), set()
    for c, o in _solves():
        # (iterate 0 of the warm fit and of the plain fit is the zero-control rollout: their first backward pass runs about it)
        for xs in [cc.zero_control_rollout(c["cfg"], c["flat"]["parent"], c["x0"])] + [o[ph]["xs"] for ph in ("warm", "full", "sol3")]:
            for k in (2, 4, 5):
                if (xs[:, k] < lo[k]).any():
                    below.add(k)
                if (xs[:, k] > hi[k]).any():
                    above.add(k)
    assert below == {2, 4, 5} and above == {2, 4, 5}, (below, above)
    g = lambda f, n: sc.get(f, n)
    assert g("speed", "v0_tv4")["x0"][2] == 0.0 and g("speed", "v0_tv4")["tv"] > 0 and g("speed", "v0_tv0")["tv"] == 0.0
    assert g("speed", "v_neg")["x0"][2] < 0 and g("speed", "v_neg")["solve"]
    assert g("speed", "v_below_ub")["x0"][2] < hi[2] == g("speed", "v_on_ub")["x0"][2] < g("speed", "v_over")["x0"][2] and g("speed", "tv_over")["tv"] > hi[2]
    # standstill: the first node has not moved or turned, whatever the controls (the heading row of the bicycle Jacobian vanishes there)
    for n in ("v0_tv4", "v0_tv0", "v0_tv0_on_lane"):
        x = sc.oracle_of(g("speed", n))["full"]["xs"][0]
        assert x[2] == 0.0 and x[3] == cc.X0[3] and np.array_equal(x[:2], cc.X0[:2]), n
    x = {c["name"]: c["x0"] for c in sc.family("limits")}
    assert x["a_ub"][4] == hi[4] < x["a_over"][4] and x["a_lb"][4] == lo[4] > x["a_under"][4]
    assert x["d_ub"][5] == hi[5] < x["d_over"][5] and x["d_lb"][5] == lo[5] > x["d_under"][5]
    assert x["a_ub"][5] == cc.X0[5] and x["d_ub"][4] == cc.X0[4] and x["a_over_z"][5] == 0.0 and x["d_under_z"][4] == 0.0
    assert (x["a_ub_d_ub"][4], x["a_ub_d_ub"][5]) == (hi[4], hi[5]) and x["a_under_d_under"][4] < lo[4] and x["a_under_d_under"][5] < lo[5]


def test_lane_cases_are_what_they_claim():
    L = sc.base()["lane"]
    ln = {c["name"]: c["lane"] for c in sc.family("lanes")}
    assert len(ln["P2"]) == 2 and np.array_equal(ln["reversed"], L[::-1])
    assert ln["behind"][:, 0].max() < cc.X0[0] - 1.0
    cfg = sc.base()["cfg"]
    assert np.abs(ln["outside"][:, 1] - cc.X0[1]).min() > 0.5 * (cfg.grid_h - 1) * cfg.grid_res + 100.0
    seg = lambda l: np.hypot(*np.diff(l, axis=0).T)
    for n, where in (("dup_start", 0), ("dup_mid", None), ("dup_end", -1)):
        z = np.nonzero(seg(ln[n]) == 0.0)[0]
        assert len(z) == 1 and len(ln[n]) == len(L) + 1
        assert (z[0] == 0) if where == 0 else (z[0] == len(L) - 1) if where == -1 else (0 < z[0] < len(L) - 1)
        # the oracle drops the zero-length segment: the lane field is the one of the lane without the repeat, bit for bit
        q_dup = oi.node_fields(cfg, sc.base()["flat"], cc.X0, ln[n], 0)[0]
        q_ref = oi.node_fields(cfg, sc.base()["flat"], cc.X0, L, 0)[0]
        assert np.all(np.isfinite(q_dup)) and np.array_equal(q_dup, q_ref), n
    s = seg(ln["seg_1e-9"])
    assert 0.0 < s.min() < 2e-9 and np.sum(s < 1e-6) == 1
    # the iterates of the two-point lane, of the lane behind and of the reversed lane are solves of their own (not the base case's)
    base = sc.oracle_of(sc.get("heading", "base"))
    for n in ("P2", "behind", "outside"):
        assert not np.array_equal(sc.oracle_of(sc.get("lanes", n))["warm"]["xs"], base["warm"]["xs"])
    assert (sc.oracle_of(sc.get("lanes", "behind"))["full"]["xs"][:, 2] <= 0.0).any()      # the ego backs up towards it: v crosses 0


def test_queries_sit_on_the_edge_values():
    for fam in sc.FAMILIES:
        c = sc.family(fam)[0]
        qn, qx, qu = c["queries"]
        assert len(qn) == len(qx) == len(qu) == 36 + 51 + 2 and qn.max() < c["M"]
        th = qx[36:87, 3].reshape(17, 3)
        for i, k in enumerate(range(-8, 9)):
            t = k * PI4
            assert th[i, 0] == t and th[i, 1] == np.nextafter(t, -np.inf) and th[i, 2] == np.nextafter(t, np.inf)
        assert qx[87, 2] == 0.0 and not np.signbit(qx[87, 2]) and qx[88, 2] == 0.0 and np.signbit(qx[88, 2])
        assert np.array_equal(qx[:36], cc.bound_states(c["cfg"], c["x0"]))
