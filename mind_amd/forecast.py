"""Forecast scoring against recorded futures: what the predictor said about the other road users.

The reference runs its scene predictor every planning cycle, hands reg [a,6,60,5] = (x, y, sx, sy, exp rho) in each agent's local frame to
the scenario tree (network.py:545, scenario_tree.py:281-346) and prices every other agent as a disc of radius max(sx, sy) +
``w_exo_cov_offset`` around the predicted mean (trajectory_tree.py:95-102); it never compares a forecast with what the agents went on to do.
A replayed world holds every track's future (``ReplayWorld.agent_state`` / ``is_valid``), so this module measures it -- it is called from
no planning cycle and changes no choice:

* ``ground_truth(world, scene, t_now)``: the recorded futures of a featurised scene's agents in their local frames;
* ``score_scene(gen, world, lcl_smp, agent_obs, t_now)``: featurise, one predictor call, one scoring call -- the forecast never leaves
  the device;
* ``EpisodeForecastScorer(sim)``: scores the root scene of every observation cycle of a ``ClosedLoopSim`` beside the planner.

All numbers come from the device (mind_forecast_score; definitions: mind_amd/csrc/forecast_score.h): per (agent, horizon, mode) ade / fde /
cover / first_out, per (agent, horizon) the arg-minima and brier_fde, per (scene, horizon) the joint rows (one mode index for every agent of
the scene) with miss_rate and the top-scored mode's.  Sample s of a forecast is the state at ``t_now + dt (s + 1)``: the planner appends the
60 samples directly behind the 50 observed frames (scenario_tree.py:346)."""
from types import SimpleNamespace

import numpy as np

DEFAULT_DISC_OFFSET = 2.5       # opt_cfg["w_exo_cov_offset"] of every planning config (configs/planning/_base.py)


def track_indices(world, scene):
    """the world's agent index of every agent of a featurised scene ('AV' is agent 0)"""
    ids = {tid: i for i, tid in enumerate(world.agent_ids)}
    return [0 if tid == "AV" else ids[tid] for tid in scene["TRAJS_TID"]]


def local_frames(scene):
    """(o [2], R [2,2], c [a,2], R_i [a,2,2]) in float64 of a scene's frames: world = ((x R_i^T) + c_i) R^T + o, the transform of
    ScenarioTreeGenerator._to_world with R_i = rot(atan2(vec_i))"""
    o, R = np.asarray(scene["ORIG"], np.float64), np.asarray(scene["ROT"], np.float64)
    c, vecs = np.asarray(scene["TRAJS_CTRS"], np.float64), np.asarray(scene["TRAJS_VECS"], np.float64)
    th = np.arctan2(vecs[:, 1], vecs[:, 0])
    cs, sn = np.cos(th), np.sin(th)
    Ri = np.stack([np.stack([cs, -sn], -1), np.stack([sn, cs], -1)], -2)
    return o, R, c, Ri


def ground_truth(world, scene, t_now, T=60, dt=0.1):
    """The recorded futures of the agents of ``scene`` (what ``ScenarioTreeGenerator.process_data`` returns: ORIG, ROT, TRAJS_CTRS,
    TRAJS_VECS, TRAJS_TID) in their local frames: sample s is the track's ``world.agent_state(i, t_now + dt (s + 1))[:2]`` where
    ``world.is_valid`` says so, taken through the inverse of ``_to_world``, ((p - o) R - c_i) R_i, in float64.  The scene's R is a
    float32 matrix and orthogonal to 1e-8 only, which is micrometres at 100 m: the first factor is the true inverse of R^T, so that the
    forward transform returns the recorded state to float64 rounding.  A sample past the end of the recording is invalid.
    -> gt [a, T, 2] float64 (0 where invalid), valid [a, T] uint8"""
    idx = track_indices(world, scene)
    o, R, c, Ri = local_frames(scene)
    a = len(idx)
    t_end = world.max_step * world.SIM_STEP if hasattr(world, "max_step") else np.inf
    is_valid = getattr(world, "is_valid", None)
    p, valid = np.zeros((a, T, 2)), np.zeros((a, T), np.uint8)
    for s in range(T):
        t = t_now + dt * (s + 1)
        if t > t_end + 1e-9:
            break
        for j, i in enumerate(idx):
            if is_valid is None or is_valid(i, t):
                p[j, s] = np.asarray(world.agent_state(i, t), np.float64)[:2]
                valid[j, s] = 1
    gt = np.matmul(np.matmul(p - o, np.linalg.inv(R.T)) - c[:, None, :], Ri)
    gt[valid == 0] = 0.0
    return gt, valid


def to_world(local, scene):
    """float64 forward transform of local positions [a, T, 2] of a scene's agents: ((x R_i^T) + c_i) R^T + o"""
    o, R, c, Ri = local_frames(scene)
    return np.matmul(np.matmul(np.asarray(local, np.float64), np.transpose(Ri, (0, 2, 1))) + c[:, None, :], R.T) + o


def observation(world, t, ego_state=None):
    """the local semantic map ``ClosedLoopSim._observation`` hands the planner at time t (the recorded ego unless ``ego_state`` is given)"""
    is_valid = getattr(world, "is_valid", None)
    ego = SimpleNamespace(state=world.agent_state(0, t) if ego_state is None else ego_state, type=world.object_type(0), id="AV",
                          timestep=int(round(t / 0.1)))
    exo = [SimpleNamespace(state=world.agent_state(i, t), type=world.object_type(i), id=world.agent_ids[i], timestep=int(round(t / 0.1)))
           for i in range(1, world.n_agents) if is_valid is None or is_valid(i, t)]
    return SimpleNamespace(ego_agent=ego, exo_agents=exo, map_data=world, target_lane=world.target_lane, target_lane_info=world.target_lane_info,
                           target_velocity=world.target_velocity)


class ObservationWindow:
    """The planner's 50-frame sliding Tracks (``MINDPlanner.update_observation``) kept apart from any planner: ``update(lcl_smp)`` per
    observation cycle, ``agent_obs`` is what ``process_data`` takes."""
    native_plan, _native = False, None

    def __init__(self, obs_len=50):
        self.obs_len, self.agent_obs = obs_len, {}

    def update(self, lcl_smp):
        from .planners.mind.planner import MINDPlanner
        MINDPlanner.update_observation(self, lcl_smp)

    def to_object_state(self, agent):
        from .planners.mind.planner import MINDPlanner
        return MINDPlanner.to_object_state(self, agent)


def _cfg(cfg):
    out = dict(horizons=(60,), miss_radius=2.0, disc_scale=1.0, disc_offset=0.0)
    bad = set(cfg) - set(out) - {"scored", "want"}
    if bad:
        raise TypeError(f"unknown scoring option(s) {sorted(bad)}")
    out.update(cfg)
    return out


def score_scene(gen, world, lcl_smp, agent_obs, t_now, dt=0.1, **cfg):
    """Score the predictor's forecast of the scene (``lcl_smp``, ``agent_obs``) at ``t_now`` against ``world``'s recording:
    ``gen.process_data``, one predictor call through ``gen.network`` (a loaded ScenePredNet), ``ground_truth`` and one
    ``forecast_score`` on the device tensors.  ``gen`` needs its target lane set; its ``lane_graph`` / ``lane_feat_in`` are rewritten, so
    hand over a generator of your own, not a planner's.  ``cfg``: horizons, miss_radius, disc_scale, disc_offset, scored, want of
    ``HipPredictor.forecast_score``.  -> its dict, plus ``tids`` (the agents' track ids), ``gt`` and ``valid``"""
    cfg = _cfg(cfg)
    scene = gen.process_data(lcl_smp, agent_obs)
    d, _ = gen.predict_inputs([scene])
    gen.network(d)
    pk = gen.network.last_packed
    reg, cls = pk["reg"], pk["cls"]
    gt, valid = ground_truth(world, scene, t_now, T=int(reg.shape[2]), dt=dt)
    res = pk["rt"].forecast_score(reg, cls, [0, int(reg.shape[0])], gt, valid, **cfg)
    res.update(tids=list(scene["TRAJS_TID"]), gt=gt, valid=valid)
    return res


class EpisodeForecastScorer:
    """Wraps a ClosedLoopSim the way EpisodeAuditor does.  ``step()``: when this simulator step starts an observation cycle (the planner's
    10 Hz trigger, before and after the take-over alike), the scene of that instant is observed into a window of this object's own, and on
    every ``every``-th cycle scored with a PRIVATE ScenarioTreeGenerator that shares the planner's network, config and target lane --
    ``process_data`` writes ``lane_graph`` / ``lane_feat_in`` on its object, and the planner's is not touched; then the simulation
    advances.  The observation is built from ``sim.world`` as ``ClosedLoopSim._observation`` builds it.  ``report()`` tabulates the cycles."""

    def __init__(self, sim, every=1, **cfg):
        from .planners.mind.scenario_tree import ScenarioTreeGenerator
        if "want" in cfg:
            raise TypeError("EpisodeForecastScorer reads every output back: no 'want'")
        self.sim, self.every, self.cfg = sim, max(int(every), 1), _cfg(cfg)
        pl = sim.planner
        self.gen = ScenarioTreeGenerator(pl.device, pl.network, pl.obs_len, pl.scen_tree_gen.pred_len, pl.scen_tree_gen.config)
        self.window = ObservationWindow(pl.obs_len)
        self._lane = None
        self.n_cycles = 0
        self.rows = []

    def _target_lane(self, lcl):
        if self._lane is None:          # (a replayed world hands over the same lane every cycle)
            self._lane = type(self.sim.planner)._resample_target_lane(self.sim.planner, lcl)
        return self._lane

    def step(self):
        sim = self.sim
        t = sim.sim_time
        if sim.last_trigger is None or (t - sim.last_trigger) >= sim.PLAN_STEP:
            if sim.last_trigger is None:
                self.window.agent_obs.clear()
            taking_over = t >= sim.enable_time and not sim.enabled       # (check_enable: this step takes over from the recorded state)
            lcl = observation(sim.world, t, sim.state if sim.enabled else None)
            self.window.update(lcl)
            if self.n_cycles % self.every == 0:
                self.gen.set_target_lane(*self._target_lane(lcl))
                res = score_scene(self.gen, sim.world, lcl, self.window.agent_obs, t, **self.cfg)
                res.update(time=t, planned=bool(sim.enabled or taking_over), step=sim.n_steps)
                self.rows.append(res)
            self.n_cycles += 1
        return sim.step()

    def run(self, n_steps):
        for _ in range(n_steps):
            self.step()
        return self

    SCENE_KEYS = ("s_n_scored", "s_min_ade", "s_min_fde", "s_brier_fde", "s_miss_rate", "s_miss_top", "s_k_ade", "s_k_fde", "s_k_top")

    def report(self):
        """-> dict: times [C], planned [C] (the cycle belongs to a planning step: from the take-over on), n_agents [C]; per cycle and
        horizon [C, n_h] the scene rows s_n_scored, s_min_ade, s_min_fde, s_brier_fde, s_miss_rate, s_miss_top, s_k_ade, s_k_fde, s_k_top,
        and ``cover_frac`` = the share of the scored agents' valid samples inside the disc of the scene's s_k_fde mode; ``mean``: the
        means of the float columns over the cycles that have a value (NaN-free); ``before`` / ``after``: the same dict over the cycles
        before and from the take-over (None when there is none); ``cycles``: the per-cycle result dicts of ``score_scene``"""
        if not self.rows:
            raise RuntimeError("EpisodeForecastScorer.report: no cycle was scored")
        cols = {k: np.stack([r[k][0] for r in self.rows]) for k in self.SCENE_KEYS}
        cols["cover_frac"] = np.stack([_cover_frac(r) for r in self.rows])
        times = np.array([r["time"] for r in self.rows])
        planned = np.array([r["planned"] for r in self.rows], bool)
        n_agents = np.array([len(r["tids"]) for r in self.rows], np.int32)

        def part(idx):
            if len(idx) == 0:
                return None
            out = dict(cycles=idx, times=times[idx], n_agents=n_agents[idx], **{k: v[idx] for k, v in cols.items()})
            out["mean"] = {k: _nanmean0(v[idx]) for k, v in cols.items() if v.dtype == np.float64}
            return out
        out = part(np.arange(len(self.rows)))
        out.update(planned=planned, before=part(np.flatnonzero(~planned)), after=part(np.flatnonzero(planned)), cycles=self.rows)
        return out


def _nanmean0(v):
    """column means over the rows that have a value (NaN where none has)"""
    ok = ~np.isnan(v)
    n = ok.sum(axis=0)
    return np.where(n > 0, np.where(ok, v, 0.0).sum(axis=0) / np.maximum(n, 1), np.nan)


def _cover_frac(r):
    """[n_h]: inside samples / valid samples of the agents with a valid sample, at the scene's s_k_fde mode (NaN without one)"""
    kf, cover, nv = r["s_k_fde"][0], r["cover"], r["n_valid"]
    out = np.full(len(kf), np.nan)
    for h, k in enumerate(kf):
        n = int(nv[:, h].sum())
        if k >= 0 and n > 0:
            out[h] = cover[:, h, k].sum() / n
    return out
