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
        self._policy = None

    # the reference leaves k, K, dV, V_x, V_xx of its last backward pass on the object (solver.py:51-75); here they are computed on first
    # access after a fit (``policy``) -- about the RETURNED trajectory, one accepted step later than the reference's
    _GAINS = ("k", "K", "dV", "V_x", "V_xx")

    def __getattr__(self, name):
        # before any fit the gains do not exist: AttributeError, so that hasattr() and introspection see a missing attribute.  After a fit
        # the read runs policy(), and a singular Q_uu raises numpy.linalg.LinAlgError from the attribute read, as policy() documents
        if name in iLQR._GAINS and self.__dict__.get("us") is not None and self.__dict__.get("cost") is not None:
            return self.policy()[name]
        raise AttributeError(name)

    def policy(self, mu=None):
        """The feedback policy about the last fit's returned (xs, us): one backward pass on the device (k_ilqr_gains) with ``mu`` (default:
        the fit's final ``_mu``).  -> dict(k [N,2], K [N,2,6], dV [N], V_x [N,6], V_xx [N,6,6], xs [N,6], L [N], J, mu); V_* are the values
        after the node's own update (row N-1 is that node's own: the reference's alias of root key -1 is not reproduced).  The result for the
        default mu also fills the attributes ``k``, ``K``, ``dV``, ``V_x``, ``V_xx`` until the next fit.  Raises numpy.linalg.LinAlgError
        when a Q_uu is singular (the reference's backward pass raises it from numpy.linalg.solve)."""
        if self.us is None or self.cost is None:
            raise RuntimeError("iLQR.policy: no fit has run yet")
        if mu is None and self._policy is not None:
            return self._policy
        m = float(self._mu if mu is None else mu)
        if not np.isfinite(m) or m < 0.0:
            raise ValueError(f"iLQR.policy: mu must be finite and >= 0, got {m}")
        p = self.cost.pack()
        g = get_runtime().ilqr_gains(self._cfg(0), [p], p["x0"], None, 0.0, 0, self.us, m, grid=p["grid"])
        if g["bad_node"][0] >= 0:
            raise np.linalg.LinAlgError(f"Singular matrix: Q_uu of node {int(g['bad_node'][0])}")
        res = {name: g[name][0] for name in ("k", "K", "dV", "V_x", "V_xx", "xs", "L")}
        res["J"], res["mu"] = float(g["J"][0]), m
        if mu is None:
            self._policy = res
        return res

    def rollout_policy(self, alpha, dx0=None):
        """Closed-loop rollouts of the last fit's policy (k_ilqr_policy): alpha [C] (or a number) step sizes, dx0 [C,6] (or [6], or None)
        offsets of the start state; u = us + alpha k + K (x - xs).  -> (xs [C,N,6], us [C,N,2], L [C,N], J [C]), without the leading axis
        when alpha is a number; J is the line search's sequential sum of L."""
        pol = self.policy()
        al = np.asarray(alpha, np.float64)
        single = al.ndim == 0
        al = np.atleast_1d(al)
        if al.ndim != 1 or len(al) < 1:
            raise ValueError(f"alpha must be a number or [C] with C >= 1, got shape {list(al.shape)}")
        d0 = None
        if dx0 is not None:
            d0 = np.asarray(dx0, np.float64)
            if d0.ndim == 1:
                d0 = np.tile(d0, (len(al), 1))
            if d0.shape != (len(al), 6):
                raise ValueError(f"dx0 must be [6] or [{len(al)}, 6], got {list(d0.shape)}")
        p = self.cost.pack()
        xs, us, L, J = get_runtime().ilqr_policy_rollouts(self._cfg(0), [p], p["x0"], None, 0.0, 0, self.us, pol["k"], pol["K"], al, d0,
                                                          grid=p["grid"])
        xs, us, L, J = xs[0], us[0], L[0], J[:, 0].copy()
        return (xs[0], us[0], L[0], float(J[0])) if single else (xs, us, L, J)

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
        self._policy = None
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
