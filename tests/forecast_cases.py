"""Shared by tests/test_forecast_host.py and tests/test_gpu_forecast.py: the seeded forecast batches, the comparison of two result dicts
and the recorded scenes as scoring inputs.  Not a test module."""
import functools

import numpy as np

import forecast_restate as rs

SIZES = (1, 0, 7, 8, 9, 17, 64, 217)              # 323 agents; an empty scene inside the batch
SEED = 5
SHAPES = ((6, 60), (1, 1), (8, 256))
HORIZONS = ((60,), (10, 30, 60), (1,), (1, 2, 3, 60))
ALL = rs.NAMES_A3 + rs.NAMES_A2 + rs.NAMES_S
PATTERNS = 7                                      # validity patterns, dealt to the agents in turn


def horizons_for(T):
    """the horizon sets of the issue cut to what a T-sample forecast admits, and one that ends at T"""
    out = []
    for hz in HORIZONS + ((1, 2, 3, T),):
        h = tuple(sorted({min(v, T) for v in hz}))
        if h not in out:
            out.append(h)
    return out


def validity(rng, A, T):
    """all valid, none valid, only t = 0, only t = T - 1, a track that ends early, one that starts late, ten random holes"""
    v = np.zeros((A, T), np.uint8)
    for a in range(A):
        p = a % PATTERNS
        if p == 0:
            v[a] = 1
        elif p == 2:
            v[a, 0] = 1
        elif p == 3:
            v[a, T - 1] = 1
        elif p == 4:
            v[a, :max(1, int(rng.integers(T // 4, 3 * T // 4 + 1)))] = 1
        elif p == 5:
            v[a, min(T - 1, int(rng.integers(T // 4, 3 * T // 4 + 1))):] = 1
        elif p == 6:
            v[a] = 1
            v[a, rng.choice(T, size=min(10, T // 2), replace=False)] = 0
    return v


@functools.lru_cache(maxsize=None)
def batch(K=6, T=60, seed=SEED, sizes=SIZES):
    """curved constant-speed truths (local frame: from the origin along +x), K modes perturbed in speed and curvature plus 5 cm noise,
    sigma growing with time.  -> dict(reg [A,K,T,5] f32, cls [B,K] f32, actor_off, gt [A,T,2], valid [A,T], scored [A])"""
    rng = np.random.default_rng(seed)
    A, B = int(sum(sizes)), len(sizes)
    tau = 0.1 * (np.arange(T) + 1.0)
    v = rng.uniform(0.5, 15.0, A)
    kap = rng.uniform(0.002, 0.05, A) * rng.choice([-1.0, 1.0], A)

    def arc(v, kap):
        th = kap[..., None] * v[..., None] * tau
        return np.stack([np.sin(th) / kap[..., None], (1.0 - np.cos(th)) / kap[..., None]], -1)
    gt = arc(v, kap)
    vk = v[:, None] * (1.0 + 0.15 * rng.normal(size=(A, K)))
    kk = kap[:, None] + 0.02 * rng.normal(size=(A, K))
    kk = np.where(np.abs(kk) < 1e-3, 1e-3, kk)
    xy = arc(vk, kk) + 0.05 * rng.normal(size=(A, K, T, 2))
    sig = (0.2 + 0.25 * tau)[None, None, :, None] * rng.uniform(0.6, 1.4, (A, K, 1, 2))
    rho = np.exp(0.1 * rng.normal(size=(A, K, T, 1)))
    reg = np.concatenate([xy, sig, rho], -1).astype(np.float32)
    logit = rng.normal(size=(B, K))
    cls = (np.exp(logit) / np.exp(logit).sum(1, keepdims=True)).astype(np.float32)
    valid = validity(rng, A, T)
    scored = (rng.uniform(size=A) < 0.8).astype(np.uint8)
    out = dict(reg=reg, cls=cls, actor_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), gt=gt, valid=valid, scored=scored)
    for a in out.values():
        a.setflags(write=False)
    return out


def same(got, want, names=None, where=""):
    """bitwise equality of two result dicts over ``names`` (None = every output of the C-ABI); NaN == NaN"""
    for k in (ALL if names is None else names):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (where, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float64:
            assert np.array_equal(np.isnan(g), np.isnan(w)), (where, k, "NaN pattern")
            m = ~np.isnan(g)
            assert np.array_equal(g[m].view(np.uint64), w[m].view(np.uint64)), (where, k, float(np.abs(g[m] - w[m]).max()) if m.any() else 0.0)
        else:
            assert np.array_equal(g, w), (where, k, np.argwhere(g != w)[:4].tolist())


def agent_rows(res, lo, hi):
    """the per-agent outputs of agents lo..hi of a result"""
    return {k: res[k][lo:hi] for k in rs.NAMES_A3 + rs.NAMES_A2}


def window_at(world, t_now, plan_step=0.1 - 1e-4, sim_step=0.02):
    """(lcl_smp, agent_obs) of a replayed world at the observation cycle in force at ``t_now``: the simulator's clock (repeated additions of
    sim_step) and trigger rule up to there.  -> lcl_smp, agent_obs, the trigger's time"""
    from mind_amd import forecast
    win, t, last, lcl, t_obs = forecast.ObservationWindow(), 0.0, None, None, None
    while t <= t_now + 1e-9:
        if last is None or (t - last) >= plan_step:
            last = t
            lcl, t_obs = forecast.observation(world, t), t
            win.update(lcl)
        t += sim_step
    return lcl, win.agent_obs, t_obs


@functools.lru_cache(maxsize=None)
def recorded_scene(name, t_now=4.0):
    """(world, scene, gt, valid, t) of a recorded demo scene featurised by the host featuriser at the take-over"""
    import torch
    from mind_amd import forecast
    from mind_amd.planners.mind.configs.planning._base import ScenTreeCfg
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.planners.mind.scenario_tree import ScenarioTreeGenerator
    from mind_amd.scene_io import ReplayWorld, scene_fixture_path
    w = ReplayWorld.from_scene_file(scene_fixture_path(name))
    lcl, obs, t = window_at(w, t_now)
    gen = ScenarioTreeGenerator(torch.device("cpu"), None, 50, 50, ScenTreeCfg())
    gen.set_target_lane(*MINDPlanner._resample_target_lane(None, lcl))
    scene = gen.process_data(lcl, obs)
    gt, valid = forecast.ground_truth(w, scene, t)
    return w, scene, gt, valid, t
