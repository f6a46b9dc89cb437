"""Host side of mind_ilqr_score_trees and of the multi-start iLQR.fit -- no GPU needed: the entry point fails cleanly without a context, its
binding matches the header, a plain solve's launch record and tables are what they were before the scoring request existed, and the
multi-start selection picks the lowest finite cost."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mind_amd import _lib
from mind_amd.planners.ilqr import solver as ilqr_solver
from mind_amd.planners.ilqr.dynamics import BicycleDynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE7 = [-1, 0, 1, 1, 2, 3, 4]
SHAPE_THREE = [TREE7, [-1, 0, 1, 2, 3], [-1, 0, 0, 1, 1, 2]]
# mind_debug_ilqr_plan(no knobs, 256 CUs, plain solve) of [TREE7] and of SHAPE_THREE, recorded on the commit before mind_ilqr_score_trees
PLAN_ONE = [
    16, 1, 2, 1, 10, 1, 10, 88, 11, 1, 1, 0, 0, 0, 0, 0, 7, 5, 3, 2, 2, 2, 6, 7, 8, 7, 4, 7, 3, 3, 48, 3, 24, 3, 3, 7, 0, 1, 2, 4, 6, 7, 0, 1, 2,
    3, 4, 5, 6, 0, 1, 3, 4, 5, 6, 6, 6, 1, 2, 3, 4, 5, 6, 0, 0, 2, 5, 7, 0, 1, 2, 4, 6, 3, 5, 0, 1, 3, 0, 1, 2, 0, 2, 1, 0, 0, 2, 1, 0, 2, 3, 0,
    0, 0, 0, 0, 0, 2, 5, 6, 2, 4, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 7, 5, 3, 3, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3, 0, 2, 0, 1, -1, 0, 0,
    0, 2, 5, 2, 4, 1, 0, 0, 0, 5, 7, 3, 5, 1, 0, 0, 0, 2, 5, 7, 0, 2, 7, 0, 1, 2, 4, 6, 3, 5]
PLAN_THREE = [
    16, 3, 2, 1, 10, 1, 10, 88, 11, 1, 1, 0, 0, 0, 0, 0, 7, 5, 3, 2, 2, 2, 6, 7, 8, 7, 4, 7, 3, 3, 48, 3, 24, 3, 3, 7, 0, 1, 2, 4, 6, 7, 0, 1, 2,
    3, 4, 5, 6, 0, 1, 3, 4, 5, 6, 6, 6, 1, 2, 3, 4, 5, 6, 0, 0, 2, 5, 7, 0, 1, 2, 4, 6, 3, 5, 0, 1, 3, 0, 1, 2, 0, 2, 1, 0, 0, 2, 1, 0, 2, 3, 0,
    0, 0, 0, 0, 0, 2, 5, 6, 2, 4, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 7, 5, 3, 3, 0, 6, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3, 0, 2, 0, 1, -1, 0, 0,
    0, 2, 5, 2, 4, 1, 0, 0, 0, 5, 7, 3, 5, 1, 0, 0, 0, 2, 5, 7, 0, 2, 7, 0, 1, 2, 4, 6, 3, 5, 5, 5, 1, 1, 1, 1, 6, 5, 6, 5, 2, 5, 2, 1, 16, 2, 8,
    1, 2, 5, 0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 4, 1, 2, 3, 4, 0, 0, 5, 0, 1, 2, 3, 4, 0, 1, 0, 0, 5, 4, 0, 3, 0, 4, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 1, 0, 5, 0, 1, -1, 0, 0, 0, 5, 0, 5, 0, 1, 2, 3, 4, 6, 3, 5, 3, 2, 3, 4, 6, 7, 6, 6, 6, 4, 5, 80, 4, 40, 5, 4, 6, 0, 1, 3, 6,
    0, 1, 2, 3, 4, 5, 0, 2, 4, 5, 5, 5, 5, 1, 2, 3, 4, 5, 0, 0, 1, 2, 4, 5, 6, 0, 1, 2, 5, 3, 4, 0, 1, 3, 5, 0, 1, 2, 3, 4, 0, 1, 0, 0, 0, 2, 0,
    0, 1, 2, 0, 0, 0, 0, 0, 0, 1, 2, 1, 1, 1, 2, 2, 0, 3, 4, 0, 0, 0, 0, 0, 0, 2, 4, 5, 2, 2, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 5, 3, 3, 3, 0,
    5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 6, 4, 4, 4, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 3, 5, 0, 1, 0, 0, -1, 0, 0, 0, 1, 2, 1, 1, 0, 0, 0, 0, 2,
    4, 2, 5, 0, 0, 0, 0, 4, 5, 3, 3, 1, 0, 0, 0, 5, 6, 4, 4, 1, 0, 0, 0, 1, 2, 4, 5, 6, 0, 1, 4, 6, 0, 1, 2, 5, 3, 4]


def _record(parents):
    lib = _lib.load()
    nn = (C.c_int * len(parents))(*[len(p) for p in parents])
    flat = [v for p in parents for v in p]
    par = (C.c_int32 * len(flat))(*flat)
    n = lib.mind_debug_ilqr_plan(None, None, 0, 256, 0, len(parents), nn, par, None, 0, None)
    out = (C.c_longlong * n)()
    assert lib.mind_debug_ilqr_plan(None, None, 0, 256, 0, len(parents), nn, par, out, n, None) == n
    return list(out)


def test_plain_solve_plan_is_unchanged():
    assert _record([TREE7]) == PLAN_ONE
    assert _record(SHAPE_THREE) == PLAN_THREE


def test_score_without_a_context_fails_cleanly():
    lib = _lib.load()
    us, J = np.zeros((1, 7, 2)), np.zeros((1, 1))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.mind_ilqr_score_trees(None, None, None, None, 1, None, None, 0, 0.0, 0, 1, dp(us), None, None, dp(J)) == _lib.MIND_EINVAL
    assert lib.mind_ilqr_score_trees(None, None, None, None, 0, None, None, 0, 0.0, 0, 0, None, None, None, None) == _lib.MIND_EINVAL
    assert not J.any()


def test_binding_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "mind_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+mind_ilqr_score_trees\s*\(([^)]*)\)", txt)
    assert m, "mind_ilqr_score_trees is not declared in include/mind_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    lib = _lib.load()
    assert len(args) == len(lib.mind_ilqr_score_trees.argtypes) == 15
    assert lib.mind_ilqr_score_trees.restype is C.c_int and "mind_ilqr_score_trees" in _lib.EXPORTS
    for a, t in zip(args, lib.mind_ilqr_score_trees.argtypes):
        if a.startswith("int "):
            assert t is C.c_int, a
        elif a.startswith("double ") and "*" not in a:
            assert t is C.c_double, a
        else:
            assert "*" in a and t not in (C.c_int, C.c_double), a


class _Cost:
    def __init__(self, n):
        self.n = n

    def pack(self):
        return dict(parent=np.arange(-1, self.n - 1, dtype=np.int32), grid=dict(), x0=np.zeros(6))


class _Runtime:
    """stands in for the HIP runtime: candidate c's cost is costs[c]; a fit returns the controls it was started from"""

    def __init__(self, costs):
        self.costs, self.scored, self.fitted = np.asarray(costs, np.float64), [], []

    def ilqr_score(self, cfg, flats, x0, lane, target_vel, use_exo, us_cand, grid=None, **kw):
        assert grid is not None and len(flats) == 1 and cfg.max_iter == 0
        self.scored.append(np.array(us_cand))
        c, m = us_cand.shape[:2]
        return [np.zeros((c, m, 6))], [np.zeros((c, m))], self.costs[:c, None].copy()

    def ilqr_solve_fields(self, cfg, grid, tree, x0, us_init=None):
        self.fitted.append(np.array(us_init))
        return np.zeros((len(us_init), 6)), np.array(us_init), dict(iterations=cfg.max_iter, converged=0, J=1.5, mu=1.0)


def _fit(monkeypatch, costs, n=4):
    rt = _Runtime(costs)
    monkeypatch.setattr(ilqr_solver, "get_runtime", lambda: rt)
    s = ilqr_solver.iLQR(BicycleDynamics(0.2, 2.5))
    cands = np.arange(len(costs) * n * 2, dtype=np.float64).reshape(len(costs), n, 2)
    return rt, s, cands


def test_multi_start_takes_the_lowest_cost_and_the_first_of_equals(monkeypatch):
    rt, s, cands = _fit(monkeypatch, [3.0, 1.0, 2.0, 1.0])
    xs, us = s.fit(cands, _Cost(4), n_iterations=7)
    assert s.start_index == 1 and np.array_equal(s.start_costs, [3.0, 1.0, 2.0, 1.0])
    assert len(rt.scored) == 1 and np.array_equal(rt.scored[0], cands)
    assert len(rt.fitted) == 1 and np.array_equal(rt.fitted[0], cands[1]) and np.array_equal(us, cands[1])
    assert s.N == 4 and s.iterations == 7 and s.J_opt == 1.5


def test_multi_start_skips_non_finite_costs(monkeypatch):
    rt, s, cands = _fit(monkeypatch, [np.nan, np.inf, 5.0, -np.inf, 4.0])
    s.fit(cands, _Cost(4))
    assert s.start_index == 4 and np.array_equal(rt.fitted[0], cands[4])
    rt, s, cands = _fit(monkeypatch, [np.nan, 7.0])
    s.fit(cands, _Cost(4))
    assert s.start_index == 1


def test_multi_start_without_a_finite_candidate_raises(monkeypatch):
    rt, s, cands = _fit(monkeypatch, [np.nan, np.inf, -np.inf])
    with pytest.raises(ValueError, match="no candidate has a finite cost"):
        s.fit(cands, _Cost(4))
    assert not rt.fitted


def test_two_dimensional_start_is_not_scored_and_shapes_are_checked(monkeypatch):
    rt, s, cands = _fit(monkeypatch, [1.0, 2.0])
    s.fit(cands[1], _Cost(4), n_iterations=3)
    assert not rt.scored and np.array_equal(rt.fitted[0], cands[1]) and s.start_index is None and s.start_costs is None
    with pytest.raises(ValueError):
        s.score(cands[:, :3], _Cost(4))
    with pytest.raises(ValueError):
        s.fit(cands, _Cost(5))
