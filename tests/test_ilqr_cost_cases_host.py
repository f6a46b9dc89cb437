"""CPU: the cost-edge cases of tests/ilqr_cost_cases.py can catch what they are for, proven on the oracle alone -- the two summation orders
of the exo-agent sum differ in the bits on the crowded cases and the oracle adds in ascending order; a relevant-agent list whose window reach
is a constant 1.0 m misses agents on the coarse grids while the reach 1.5 sqrt(2) res never does; the ties are exact and round both ways, all
nine window placements are visited; the oracle is finite on everything the GPU tests assert."""
import numpy as np
import pytest

import ilqr_cost_cases as cc
import ilqr_policy_restate as rs
from oracle import ilqr as oi

CROWDED = [("crowd", "a40_chain"), ("crowd", "a40_branch"), ("crowd", "a128_chain"), ("far", "x0_4000_-3000")]


def _asserted_cells(c):
    """(node, sx, sy) of the plain 3 x 3 windows about the three-iteration solve's states"""
    xs = cc.oracle_of(c)["sol3"]["xs"]
    cells = []
    for i in range(c["M"]):
        w = cc.window_cells(c, xs[i, 0], xs[i, 1])
        assert w is not None, (c["name"], i)
        cells += [(i, sx, sy) for sx, sy in w]
    return cells


@pytest.mark.parametrize("fam,name", CROWDED)
def test_summation_orders_differ_and_the_oracle_adds_ascending(fam, name):
    c = cc.get(fam, name)
    cfg, flat = c["cfg"], c["flat"]
    assert flat["mean"].shape[1] >= 40
    gx, gy, off = cc.grid_of(c)
    lane_only, ogx, ogy, ooff = oi.node_fields(cfg, flat, c["x0"], c["lane"], 0)
    fields = oi.node_fields(cfg, flat, c["x0"], c["lane"], 1)[0]
    assert np.array_equal(gx, ogx) and np.array_equal(gy, ogy) and np.array_equal(off, ooff)
    differ = 0
    for i, sx, sy in _asserted_cells(c):
        t = cc.exo_terms(c, i, gx[sx], gy[sy])
        asc, strided = cc.sum_ascending(t), cc.sum_strided7(t)
        differ += asc != strided
        m = flat["mean"][i, 0].astype(np.float64)
        ego = np.sqrt((gx[sx] - m[0]) ** 2 + (gy[sy] - m[1]) ** 2) - float(flat["cov"][i, 0] + np.float32(cfg.w_ego_cov_offset))
        ego = ego if ego > 0.0 else 0.0
        want = (lane_only[i, sy, sx] + cfg.w_exo * asc) + cfg.w_ego * ego
        assert fields[i, sy, sx] == want, (name, i, sx, sy, fields[i, sy, sx], want)
    assert differ >= 1, name


def test_crowd_reaches_the_cell_counts_and_list_lengths_it_is_for():
    """single cells are reached by 2, 3, 8, 9 and at least 15 agents; nodes with exactly 15, 16 and 17 agents inside the list radius (the
    capacity of a list and the first two overflows); sigmas are not round numbers"""
    reached, lengths = set(), set()
    for c in cc.family("crowd"):
        assert c["M"] <= 40 and c["flat"]["mean"].shape[1] in (9, 17, 40, 128)
        gx, gy, _ = cc.grid_of(c)
        xs = cc.oracle_of(c)["sol3"]["xs"]
        for i, sx, sy in _asserted_cells(c):
            reached.add(int((cc.exo_terms(c, i, gx[sx], gy[sy]) > 0.0).sum()))
        for i in range(c["M"]):
            lengths.add(int(cc.list_members(c, i, xs[i, 0], xs[i, 1], cc.list_reach(c["cfg"].grid_res)).sum()))
        sg = c["flat"]["cov"][:, 1:].astype(np.float64)
        assert not np.any(sg * 100 == np.round(sg * 100))
    assert {2, 3, 8, 9} <= reached and max(reached) >= 15, sorted(reached)
    assert {15, 16, 17} <= lengths, sorted(lengths)
    assert sorted({c["flat"]["mean"].shape[1] for c in cc.family("crowd")}) == [9, 17, 40, 128]


def _iterates(c, n):
    """iterate 0 = the zero-control rollout, iterate k = the oracle's solve with max_iter = k; accepted[k]: iteration k's step was accepted"""
    its = [rs.rollout(c["cfg"], c["flat"]["parent"], c["x0"], np.zeros((c["M"], 2)))]
    accepted = []
    for k in range(1, n + 1):
        s = oi.solve(cc.copy_cfg(c["cfg"], max_iter=k), c["flat"], c["x0"], c["lane"], c["tv"], 1, trace=True)
        its.append(s["xs"])
        accepted.append(s["iterations"] == k and s["trace"][k - 1, 2] >= 0)
    return its, accepted


_misses = {}


def _list_misses(c, reach):
    """misses of the list rule over the accepted steps of the first five iterations (rejected candidates take larger steps: not counted)"""
    key = c["name"]
    if key not in _misses:
        _misses[key] = _iterates(c, 5)
    its, accepted = _misses[key]
    out = []
    for k, ok in enumerate(accepted):
        if ok:
            out += [(k,) + m for m in cc.list_misses(c, its[k], its[k + 1], reach)]
    return out


@pytest.mark.parametrize("grid", cc.GRIDS)
def test_list_reach_must_scale_with_the_grid(grid):
    res, W, H = grid
    c = cc.get("grids", f"res{res}_{W}x{H}")
    assert c["flat"]["mean"].shape[1] == 40 and (c["cfg"].grid_res, c["cfg"].grid_w, c["cfg"].grid_h) == grid
    assert _list_misses(c, cc.list_reach(res)) == []
    if res in (0.8, 1.0):
        assert cc.list_reach(res) > 1.0
        assert len(_list_misses(c, 1.0)) >= 1                   # the constant that holds at 0.4 m is too short here
    if grid == (0.4, 256, 256):
        assert cc.list_reach(res) < 1.0 and _list_misses(c, 1.0) == []
        assert len(_list_misses(c, 0.0)) >= 1                   # ... and a margin is needed at all


def test_ties_are_exact_round_both_ways_and_every_placement_is_visited():
    tp = cc.tie_points()
    c = cc.family("ties_borders")[0]
    off, res = tp["off"], tp["res"]
    _, _, ooff = cc.grid_of(c)
    assert np.array_equal(off, ooff) and np.array_equal(off, [-6.875, -5.375])
    down = up = 0
    for px, py, kx, ky in tp["ties"]:
        for p, o, k in ((px, off[0], kx), (py, off[1], ky)):
            if k is None:
                continue
            q = (p - o) / res
            assert q == k + 0.5 and q * 2 == 2 * k + 1                      # exact in float64
            r = int(np.rint(q))
            assert r == (k if k % 2 == 0 else k + 1)                        # half to even
            down += r == k
            up += r == k + 1
    assert down >= 4 and up >= 4
    qn, qx, qu = c["queries"]
    seen = {cc.placement(c, *cc.cell_of(c, x[0], x[1])) for x in qx}
    assert seen == {(a, b) for a in range(3) for b in range(3)}
    for px, py, xi, yi in tp["borders"]:
        assert cc.cell_of(c, px, py) == (xi, yi)
    gx, gy, _ = cc.grid_of(c)
    sides = set()
    for px, py in tp["outside"]:
        sides |= {"w" if px < gx[0] else "", "e" if px > gx[-1] else "", "s" if py < gy[0] else "", "n" if py > gy[-1] else ""}
    assert {"w", "e", "s", "n"} <= sides
    # agents really reach the border cells' windows
    for xi, yi in ((0, 0), (tp["W"] - 1, 0), (0, tp["H"] - 1), (tp["W"] - 1, tp["H"] - 1)):
        assert (cc.exo_terms(c, 0, gx[xi], gy[yi]) > 0.0).any(), (xi, yi)


def test_degenerate_inputs_are_what_they_claim():
    cases = {c["name"]: c for c in cc.family("degenerate")}
    c = cases["sigma_sums"]
    off = np.float32(c["cfg"].w_exo_cov_offset)
    s = c["flat"]["cov"][0, 1:5] + off
    assert s[0] < 0 and s[1] == 0 and s[2] == 50.0 and 0 < s[3] < 1e-6
    assert set(np.unique(cases["prob_0_1e-30"]["flat"]["prob"]).tolist()) == {0.0, float(np.float32(1e-30)), 1.0}
    assert cases["cost_offset_0"]["cfg"].w_exo_cost_offset == 0.0
    qn, qx, qu = c["queries"]
    assert len(qx) == 36
    lo, hi = np.array(list(c["cfg"].state_lower)), np.array(list(c["cfg"].state_upper))
    for j, x in enumerate(qx):
        k, b = (j // 3) % 6, (lo, hi)[j // 18][(j // 3) % 6]
        assert x[k] == (b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf))[j % 3]


@pytest.mark.parametrize("fam,name", cc.case_ids())
def test_oracle_is_finite_on_every_asserted_output(fam, name):
    c = cc.get(fam, name)
    node, x, u, want = cc.eval_points(c)
    skip = cc.NAN_QUERIES.get(fam, {}).get(name, [])
    assert len(skip) <= 0.05 * len(node)
    keep = np.setdiff1d(np.arange(len(node)), np.asarray(skip, int))
    for k, v in want.items():
        assert np.all(np.isfinite(v[keep])), (fam, name, k)
    if c["solve"]:
        o = cc.oracle_of(c)
        for ph in ("warm", "full"):
            assert np.all(np.isfinite(o[ph]["xs"])) and np.all(np.isfinite(o[ph]["us"])) and np.isfinite(o[ph]["J"])
            assert np.all(np.isfinite(o[ph]["trace"]))
