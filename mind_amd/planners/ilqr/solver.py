"""iLQR of the reference (planners/ilqr/solver.py:21-421) on the MI355X: ``fit`` packs the TreeCost and
runs the whole loop -- rollout, tree Riccati sweep, 10-step backtracking line search, Levenberg-Marquardt
schedule, convergence test -- in ONE persistent kernel launch (k_ilqr, generic mode)."""
import numpy as np

from ... import _lib
from ...runtime import get_runtime
from .cost import TreeCost
from .dynamics import BicycleDynamics


class iLQR:
    def __init__(self, dynamics, max_reg=1e10, hessians=False):
        if not isinstance(dynamics, BicycleDynamics):
            raise NotImplementedError("the kernel integrates the kinematic bicycle of trajectory_tree.py:153-177; "
                                      "pass mind_amd.planners.ilqr.dynamics.BicycleDynamics(dt, wheelbase)")
        if hessians or max_reg != 1e10:
            raise NotImplementedError("k_ilqr implements the reference's configuration: max_reg=1e10, hessians=False")
        self.dynamics = dynamics
        self.cost = None
        self.N = None
        self.xs = None
        self.us = None
        self.J_opt = None
        self.iterations = None
        self.converged = None
        self._mu = 1.0
        self.start_index = None
        self.start_costs = None

    def _cfg(self, n_iterations):
        cfg = _lib.IlqrCfg()
        cfg.dt, cfg.wheelbase, cfg.max_iter = float(self.dynamics.dt), float(self.dynamics.wheelbase), int(n_iterations)
        return cfg

    def score(self, us_candidates, cost: TreeCost):
        """Rollout and cost of C candidate control trees, no optimisation (k_ilqr_score, generic mode): us_candidates [C, N, 2] ->
        (xs [C, N, 6], L [C, N], J [C]); J[c] is the J_opt ``fit(us_candidates[c], cost, n_iterations=1)`` reports."""
        uc = np.asarray(us_candidates, np.float64)
        p = cost.pack()
        if uc.ndim != 3 or uc.shape[1:] != (len(p["parent"]), 2):
            raise ValueError(f"us_candidates must be [C, {len(p['parent'])}, 2] for this cost tree, got {uc.shape}")
        xs, L, J = get_runtime().ilqr_score(self._cfg(0), [p], p["x0"], None, 0.0, 0, uc, grid=p["grid"])
        return xs[0], L[0], J[:, 0].copy()

    def fit(self, us_init, cost: TreeCost = None, n_iterations=100):
        """-> (xs [N,6], us [N,2]); node key k of the cost tree <-> row k (solver.py:80-167).  us_init [C, N, 2]: multi-start -- the
        candidates are scored (``score``), the fit runs from the one of lowest finite J (the first of equals); ``start_index`` /
        ``start_costs`` record the choice."""
        self.cost = cost
        us_init = np.asarray(us_init, np.float64)
        if us_init.ndim == 3:
            J = self.score(us_init, cost)[2]
            finite = np.isfinite(J)
            if not finite.any():
                raise ValueError("multi-start fit: no candidate has a finite cost")
            self.start_costs = J
            self.start_index = int(np.argmin(np.where(finite, J, np.inf)))
            us_init = us_init[self.start_index]
        self.N = len(us_init)
        p = cost.pack()
        if len(p["parent"]) != self.N:
            raise ValueError(f"us_init has {self.N} rows, the cost tree {len(p['parent'])} nodes")
        cfg = self._cfg(n_iterations)
        xs, us, st = get_runtime().ilqr_solve_fields(cfg, p["grid"], p, p["x0"], us_init)
        self.xs, self.us = xs, us
        self.J_opt, self._mu = st["J"], st["mu"]
        self.iterations, self.converged = st["iterations"], bool(st["converged"])
        return xs, us
