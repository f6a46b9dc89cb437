"""CPU: forecast scoring by the library's HOST entry (mind_debug_forecast_score, mind_amd/csrc/forecast_score.h on the CPU) against the numpy
restatement (tests/forecast_restate.py) bit for bit, against an independent vectorised evaluation to 1e-12, on hand cases with exact
numbers, on the four recorded scenes (frames and time convention of mind_amd.forecast.ground_truth) and over its error codes."""
import ctypes as C

import numpy as np
import pytest

import forecast_cases as fc
import forecast_restate as rs
from mind_amd import _lib, forecast

CFG = dict(miss_radius=2.0, disc_scale=1.0, disc_offset=0.5)


def _host(b, scored=None, horizons=(60,), **kw):
    return _lib.forecast_score_host(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], scored, horizons, **dict(CFG, **kw))


@pytest.mark.parametrize("K,T", fc.SHAPES)
def test_restatement_is_the_host_entry_bit_for_bit(K, T):
    b = fc.batch(K, T)
    assert b["reg"].shape == (323, K, T, 5) and np.diff(b["actor_off"]).tolist() == list(fc.SIZES)
    for hz in fc.horizons_for(T):
        for scored in (None, b["scored"]):
            want = rs.score(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], scored, hz, **CFG)
            fc.same(_host(b, scored, hz), want, where=(K, T, hz, scored is None))
    # every validity pattern is in the batch and does what it says
    r = _host(b, None, (T,))
    nv, last = r["n_valid"][:fc.PATTERNS, 0], r["last"][:fc.PATTERNS, 0]
    assert nv[0] == T and nv[1] == 0 and last[1] == -1 and (nv[2], last[2]) == (1, 0) and (nv[3], last[3]) == (1, T - 1)
    assert np.all(np.isnan(r["ade"][1])) and np.all(r["cover"][1] == 0) and np.all(r["first_out"][1] == -1) and r["k_ade"][1, 0] == -1
    if T > 20:
        assert 0 < nv[4] < T and last[4] == nv[4] - 1 and 0 < nv[5] < T and last[5] == T - 1 and nv[6] == T - 10
    assert r["s_n_scored"][1, 0] == 0 and np.isnan(r["s_miss_rate"][1, 0]) and r["s_k_fde"][1, 0] == -1        # the empty scene


def _gap2(v):
    """smallest gap between the best and the second-best finite value along the last axis (inf where fewer than two are finite)"""
    s = np.sort(np.where(np.isfinite(v), v, np.inf), axis=-1)
    if s.shape[-1] < 2:
        return np.inf
    with np.errstate(invalid="ignore"):
        g = s[..., 1] - s[..., 0]
    return float(np.nanmin(np.where(np.isfinite(g), g, np.inf)))


def _vectorised(b, scored, hz, miss_radius, disc_scale, disc_offset):
    """the same quantities by other means: np.linalg.norm, np.mean over masked selections, np.argmin"""
    reg, gt, valid, off = b["reg"].astype(np.float64), b["gt"], b["valid"] != 0, b["actor_off"]
    A, K, T = reg.shape[:3]
    d = np.linalg.norm(reg[..., :2] - gt[:, None], axis=-1)
    inside = d <= disc_scale * np.maximum(reg[..., 2], reg[..., 3]) + disc_offset
    o = dict(ade=np.full((A, len(hz), K), np.nan), fde=np.full((A, len(hz), K), np.nan), cover=np.zeros((A, len(hz), K), np.int32),
             first_out=np.full((A, len(hz), K), -1, np.int32), n_valid=np.zeros((A, len(hz)), np.int32), last=np.full((A, len(hz)), -1, np.int32))
    for a in range(A):
        for h, e in enumerate(hz):
            t = np.flatnonzero(valid[a, :e])
            o["n_valid"][a, h] = len(t)
            if len(t):
                o["last"][a, h] = t[-1]
                o["ade"][a, h], o["fde"][a, h] = d[a][:, t].mean(axis=1), d[a][:, t[-1]]
                o["cover"][a, h] = inside[a][:, t].sum(axis=1)
                for k in range(K):
                    out = t[~inside[a, k, t]]
                    o["first_out"][a, h, k] = out[0] if len(out) else -1
    has = o["n_valid"] > 0
    for m in ("ade", "fde"):
        o["k_" + m] = np.where(has, np.argmin(np.where(has[..., None], o[m], 0.0), axis=-1), -1).astype(np.int32)
    scene_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    kf = np.maximum(o["k_fde"], 0)
    pa = b["cls"].astype(np.float64)[scene_of[:, None], kf]
    o["brier_fde"] = np.where(has, np.take_along_axis(o["fde"], kf[..., None], -1)[..., 0] + (1 - pa) ** 2, np.nan)
    B, H = len(off) - 1, len(hz)
    o.update(s_n_scored=np.zeros((B, H), np.int32), s_ade=np.full((B, H, K), np.nan), s_fde=np.full((B, H, K), np.nan),
             s_k_ade=np.full((B, H), -1, np.int32), s_k_fde=np.full((B, H), -1, np.int32), s_k_top=np.zeros((B, H), np.int32),
             s_brier_fde=np.full((B, H), np.nan), s_miss_rate=np.full((B, H), np.nan), s_miss_top=np.full((B, H), np.nan))
    sc = np.ones(A, bool) if scored is None else scored != 0
    for s in range(B):
        o["s_k_top"][s] = int(np.argmax(b["cls"][s]))
        for h in range(H):
            rows = np.flatnonzero(sc[off[s]:off[s + 1]] & has[off[s]:off[s + 1], h]) + off[s]
            o["s_n_scored"][s, h] = len(rows)
            if len(rows):
                o["s_ade"][s, h], o["s_fde"][s, h] = o["ade"][rows, h].mean(axis=0), o["fde"][rows, h].mean(axis=0)
                ka, kf = int(np.argmin(o["s_ade"][s, h])), int(np.argmin(o["s_fde"][s, h]))
                o["s_k_ade"][s, h], o["s_k_fde"][s, h] = ka, kf
                o["s_brier_fde"][s, h] = o["s_fde"][s, h, kf] + (1 - float(b["cls"][s, kf])) ** 2
                o["s_miss_rate"][s, h] = np.mean(o["fde"][rows, h, kf] > miss_radius)
                o["s_miss_top"][s, h] = np.mean(o["fde"][rows, h, o["s_k_top"][s, h]] > miss_radius)
    return o, d, inside


@pytest.mark.parametrize("K,T", [s for s in fc.SHAPES if s[0] > 1])
def test_independent_vectorised_evaluation(K, T):
    """values to 1e-12 relative (sums of <= 256 terms of one sign in float64: <= 256 x 2^-53), indices and counts exactly -- after the guard
    that no decision of the restatement sits on an edge: every gap >= 1e-7"""
    b = fc.batch(K, T)
    for hz in fc.horizons_for(T):
        for scored in (None, b["scored"]):
            want = rs.score(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], scored, hz, **CFG)
            got, d, inside = _vectorised(b, scored, hz, **CFG)
            d_rs, _ = rs.samples(b["reg"], b["gt"], CFG["disc_scale"], CFG["disc_offset"])
            r = CFG["disc_scale"] * np.fmax(b["reg"][..., 2], b["reg"][..., 3]).astype(np.float64) + CFG["disc_offset"]
            ok = (b["valid"] != 0)[:, None, :] & np.ones_like(inside)
            gaps = dict(agent_ade=_gap2(want["ade"]), agent_fde=_gap2(want["fde"]), scene_ade=_gap2(want["s_ade"]), scene_fde=_gap2(want["s_fde"]),
                        miss=float(np.nanmin(np.abs(want["fde"] - CFG["miss_radius"]))), disc=float(np.abs(d_rs - r)[ok].min()))
            print((K, T), hz, scored is None, {k: f"{v:.1e}" for k, v in gaps.items()})
            assert all(v >= 1e-7 for v in gaps.values()), gaps
            for k in fc.ALL:
                if want[k].dtype == np.float64:
                    assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
                    m = ~np.isnan(want[k])
                    assert np.all(np.abs(got[k][m] - want[k][m]) <= 1e-12 * np.abs(want[k][m])), (k, hz)
                else:
                    assert np.array_equal(got[k], want[k]), (k, hz)


def _one(xy, gt, sig=(1.0, 1.0), cls=None, valid=None, K=6, T=1, scored=None, actor_off=None, **kw):
    """A agents whose K modes all forecast ``xy`` [A, (K,) T, 2] with sigma ``sig``"""
    gt = np.asarray(gt, np.float64).reshape(-1, T, 2)
    A = gt.shape[0]
    reg = np.zeros((A, K, T, 5), np.float32)
    reg[..., :2] = np.asarray(xy, np.float32).reshape(A, -1, T, 2)
    reg[..., 2], reg[..., 3], reg[..., 4] = sig[0], sig[1], 1.0
    off = np.array([0, A], np.int32) if actor_off is None else np.asarray(actor_off, np.int32)
    cls = np.full((len(off) - 1, K), 1.0 / K, np.float32) if cls is None else np.asarray(cls, np.float32).reshape(len(off) - 1, K)
    valid = np.ones((A, T), np.uint8) if valid is None else np.asarray(valid, np.uint8).reshape(A, T)
    b = dict(reg=reg, cls=cls, actor_off=off, gt=gt, valid=valid)
    return b, _lib.forecast_score_host(reg, cls, off, gt, valid, scored, kw.pop("horizons", (T,)), **dict(CFG, **kw))


def test_hand_cases_on_exact_numbers():
    # forecast (0, 0), truth (3, 4), sigma 2.5, offset 2.5: d = 5.0 = r, inside
    _, r = _one([[0.0, 0.0]], [[3.0, 4.0]], sig=(2.5, 1.0), disc_offset=2.5, miss_radius=5.0)
    assert np.all(r["ade"] == 5.0) and np.all(r["fde"] == 5.0) and np.all(r["cover"] == 1) and np.all(r["first_out"] == -1)
    assert r["s_miss_rate"][0, 0] == 0.0 and r["s_miss_top"][0, 0] == 0.0                      # fde == miss_radius: not a miss
    _, r = _one([[0.0, 0.0]], [[3.0, 4.0]], sig=(1.0, 2.5), disc_offset=2.5 - 2.0 ** -50, miss_radius=np.nextafter(5.0, 0.0))
    assert np.all(r["cover"] == 0) and np.all(r["first_out"] == 0) and r["s_miss_rate"][0, 0] == 1.0 and r["s_miss_top"][0, 0] == 1.0
    # six identical modes: every arg-min is 0; brier = fde + (1 - 1/6)^2 in the header's order
    assert r["k_ade"][0, 0] == 0 and r["k_fde"][0, 0] == 0 and r["s_k_ade"][0, 0] == 0 and r["s_k_fde"][0, 0] == 0 and r["s_k_top"][0, 0] == 0
    q = 1.0 - np.float64(np.float32(1.0 / 6))
    assert r["brier_fde"][0, 0] == 5.0 + q * q and r["s_brier_fde"][0, 0] == 5.0 + q * q and r["min_fde"][0, 0] == 5.0 and r["s_min_ade"][0, 0] == 5.0
    # two equal maxima of cls: the lower k
    _, r = _one([[0.0, 0.0]], [[3.0, 4.0]], cls=[0.1, 0.3, 0.05, 0.3, 0.2, 0.05])
    assert r["s_k_top"][0, 0] == 1
    # the top mode is the only one that misses
    xy = np.zeros((1, 6, 1, 2))
    xy[0, 1] = (3.0, 4.0 + 2.5)
    _, r = _one(xy, [[3.0, 4.0]], cls=[0.1, 0.3, 0.05, 0.3, 0.2, 0.05], miss_radius=6.0)
    assert r["k_fde"][0, 0] == 1 and r["fde"][0, 0, 1] == 2.5 and r["s_miss_rate"][0, 0] == 0.0 and r["s_miss_top"][0, 0] == 0.0
    _, r = _one(xy, [[3.0, 4.0]], cls=[0.4, 0.3, 0.05, 0.3, 0.2, 0.05], miss_radius=4.0)
    assert r["s_k_top"][0, 0] == 0 and r["s_k_fde"][0, 0] == 1 and r["s_miss_rate"][0, 0] == 0.0 and r["s_miss_top"][0, 0] == 1.0


def test_nan_forecasts():
    T, hz = 8, (2, 4, 8)
    g = np.random.default_rng(3)
    gt = np.cumsum(g.uniform(0.5, 1.0, (2, T, 2)), axis=1)
    xy = gt[:, None] + g.normal(scale=0.3, size=(2, 6, T, 2))
    xy[0, 2, 3, 0] = np.nan                                  # mode 2 of agent 0, sample 3: inside horizons 4 and 8 only
    b, r = _one(xy, gt, T=T, horizons=hz)
    assert np.isfinite(r["ade"][0, 0, 2]) and np.isfinite(r["fde"][0, 0, 2])
    assert np.isnan(r["ade"][0, 1:, 2]).all() and np.isnan(r["fde"][0, 1, 2]) and np.isfinite(r["fde"][0, 2, 2])      # (fde is one sample's d)
    assert r["first_out"][0, 0, 2] in (-1, 0, 1) and r["first_out"][0, 1, 2] <= 3 and np.all(r["k_ade"][0, 1:] != 2) and r["k_fde"][0, 1] != 2
    assert np.isnan(r["s_ade"][0, 1:, 2]).all() and np.all(r["s_k_ade"][0, 1:] != 2) and np.isfinite(r["s_ade"][0, 0, 2])
    assert np.all(np.isfinite(np.delete(r["ade"], 2, axis=2)))
    fc.same(r, rs.score(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], None, hz, **CFG))
    # first_out names the NaN sample when everything before it is inside
    _, r2 = _one(xy, gt, T=T, horizons=hz, disc_offset=50.0)
    assert r2["first_out"][0, :, 2].tolist() == [-1, 3, 3] and r2["cover"][0, :, 2].tolist() == [2, 3, 7]
    # all modes NaN (and +inf): k = -1, brier NaN; the other agent keeps the scene row alive, but its means are NaN
    xy[0, :, 0, 1] = np.nan
    b, r = _one(xy, gt, T=T, horizons=hz)
    assert np.all(r["k_ade"][0] == -1) and np.all(r["k_fde"][0, 1:] == r["k_fde"][0, 1:]) and r["k_fde"][0, 0] >= 0
    assert np.isnan(r["brier_fde"][0]).sum() == 0 and np.isnan(r["min_ade"][0]).all()
    assert np.all(r["s_k_ade"][0] == -1) and np.isnan(r["s_ade"]).all() and r["s_n_scored"][0].tolist() == [2, 2, 2]
    xy[0, :, :, 0] = np.inf
    b, r = _one(xy, gt, T=T, horizons=hz)
    assert np.all(r["k_ade"][0] == -1) and np.all(r["k_fde"][0] == -1) and np.isnan(r["brier_fde"][0]).all() and np.all(r["k_fde"][1] >= 0)
    assert np.all(r["s_k_fde"][0] == -1) and np.isnan(r["s_brier_fde"]).all() and np.isnan(r["s_miss_rate"]).all() and not np.isnan(r["s_miss_top"]).any()
    fc.same(r, rs.score(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], None, hz, **CFG))


def test_scored_flags_and_empty_scenes():
    b = fc.batch()
    off = b["actor_off"]
    full, part = _host(b, None), _host(b, b["scored"])
    fc.same(part, full, names=rs.NAMES_A3 + rs.NAMES_A2)                   # an unscored agent keeps its own rows
    assert np.all(part["s_n_scored"] <= full["s_n_scored"]) and part["s_n_scored"].sum() < full["s_n_scored"].sum()
    # one agent taken out of a scene: the scene row is the one of the scene without it
    a = int(off[3])                                                        # first agent of the 8-agent scene: all samples valid
    sc = np.ones(323, np.uint8)
    sc[a] = 0
    keep = np.ones(323, bool)
    keep[a] = False
    cut = dict(reg=b["reg"][keep], cls=b["cls"], actor_off=np.where(np.arange(9) > 3, off - 1, off).astype(np.int32), gt=b["gt"][keep], valid=b["valid"][keep])
    fc.same(_host(b, sc), _host(cut, None), names=rs.NAMES_S)
    assert full["s_n_scored"][1, 0] == 0 and full["s_k_ade"][1, 0] == -1 and np.isnan(full["s_ade"][1]).all() and np.isnan(full["s_brier_fde"][1, 0])
    assert full["s_k_top"][1, 0] == int(np.argmax(b["cls"][1])) and np.isnan(full["s_miss_top"][1, 0])
    # A == 0 and no scene at all: successful no-ops
    e = _lib.forecast_score_host(np.zeros((0, 6, 60, 5), np.float32), np.zeros((2, 6), np.float32), [0, 0, 0], np.zeros((0, 60, 2)), np.zeros((0, 60), np.uint8))
    assert e["ade"].shape == (0, 1, 6) and e["s_ade"].shape == (2, 1, 6)
    e = _lib.forecast_score_host(np.zeros((0, 6, 60, 5), np.float32), np.zeros((0, 6), np.float32), [0], np.zeros((0, 60, 2)), np.zeros((0, 60), np.uint8))
    assert e["s_n_scored"].shape == (0, 1)


@pytest.mark.parametrize("name", ["demo_1", "demo_2", "demo_3", "demo_4"])
def test_ground_truth_on_the_recorded_scenes(name):
    w, scene, gt, valid, t = fc.recorded_scene(name)
    a = len(scene["TRAJS_TID"])
    assert gt.shape == (a, 60, 2) and valid.shape == (a, 60) and gt.dtype == np.float64 and abs(t - 4.0) < 1e-9 and a > 1
    idx = forecast.track_indices(w, scene)
    assert idx[0] == 0 and len(set(idx)) == a
    # the float64 forward transform returns the world states to 1e-9 m (coordinates < 1e4 m, a handful of float64 operations)
    back = forecast.to_world(gt, scene)
    n = 0
    for j, i in enumerate(idx):
        for s in range(60):
            ts = t + 0.1 * (s + 1)
            assert bool(valid[j, s]) == bool(w.is_valid(i, ts))
            if valid[j, s]:
                p = w.agent_state(i, ts)[:2]
                assert np.abs(p).max() < 1e4 and np.abs(back[j, s] - p).max() < 1e-9
                n += 1
    assert n > 60
    # the time convention, by a self-forecast: reg = float32(gt) scores ade <= sqrt(2) 2^-24 max|gt| on every fully valid moving agent, the
    # same forecast one sample late more than 100 x that on every agent faster than 1 m/s (an off-by-one step is >= 0.1 m)
    full = np.flatnonzero(valid.all(axis=1))
    step = np.linalg.norm(np.diff(gt, axis=1), axis=-1)
    moving = [j for j in full if step[j].min() > 0.1 * 1.0]                # faster than 1 m/s at every sample
    assert moving, "no fully valid moving agent"
    reg = np.zeros((a, 6, 60, 5), np.float32)
    reg[..., :2], reg[..., 2:] = gt[:, None].astype(np.float32), 1.0
    cls = np.full((1, 6), 1.0 / 6, np.float32)
    bound = np.sqrt(2.0) * 2.0 ** -24 * np.abs(gt[moving]).max()
    r = _lib.forecast_score_host(reg, cls, [0, a], gt, valid)
    assert np.all(r["ade"][moving, 0] <= bound), (r["ade"][moving, 0].max(), bound)
    late = reg.copy()
    late[:, :, 1:, :2] = reg[:, :, :-1, :2]
    r1 = _lib.forecast_score_host(late, cls, [0, a], gt, valid)
    assert np.all(r1["ade"][moving, 0] > 100 * bound) and np.all(r1["ade"][moving, 0] > 0.09), r1["ade"][moving, 0].min()
    print(name, "agents", a, "moving", len(moving), "self ade", float(r["ade"][moving, 0].max()), "bound", bound, "late ade", float(r1["ade"][moving, 0].min()))


def test_error_codes():
    lib = _lib.load()
    b = fc.batch()
    K, T = 6, 60

    def call(reg=b["reg"], cls=b["cls"], actor_off=b["actor_off"], gt=b["gt"], valid=b["valid"], horizons=(10, 60), K=K, T=T, n_h=None, null=(), want=("ade",),
             n_scenes=None, **kw):
        cfg, B, off, g, v, sc, out, res, keep = _lib.forecast_args(6, 60, actor_off, gt, valid, None, horizons, **dict(CFG, **kw), want=want)
        cfg.K, cfg.T = K, T
        if n_h is not None:
            cfg.n_h = n_h
        r, c = np.ascontiguousarray(reg, np.float32), np.ascontiguousarray(cls, np.float32)
        args = dict(cfg=C.byref(cfg), off=off, reg=C.c_void_p(r.ctypes.data), cls=C.c_void_p(c.ctypes.data), gt=g, valid=v, out=C.byref(out))
        if "horizon" in null:
            cfg.horizon = None
        for n in null:
            if n in args:
                args[n] = None
        rc = lib.mind_debug_forecast_score(args["cfg"], B if n_scenes is None else n_scenes, args["off"], args["reg"], args["cls"], args["gt"], args["valid"],
                                           None, args["out"])
        return rc, res
    rc, res = call()
    assert rc == _lib.MIND_OK and np.isfinite(res["ade"][0]).all()
    bad_off, nan_gt, inf_gt = b["actor_off"].copy(), b["gt"].copy(), b["gt"].copy()
    bad_off[3], bad_off[4] = bad_off[4], bad_off[3]
    nan_gt[0, 7, 1], inf_gt[4, 0, 0] = np.nan, np.inf                     # agents 0 and 4: sample valid
    assert b["valid"][0, 7] and b["valid"][4, 0] and not b["valid"][1, 7]
    off1 = b["actor_off"].copy()
    off1[0] = 1
    for bad in (dict(null=("cfg",)), dict(null=("out",)), dict(null=("horizon",)), dict(null=("off",)), dict(null=("reg",)), dict(null=("cls",)),
                dict(null=("gt",)), dict(null=("valid",)), dict(want=()), dict(K=0), dict(K=9), dict(T=0), dict(T=257), dict(n_h=0), dict(n_h=5),
                dict(horizons=(0, 60)), dict(horizons=(10, 61)), dict(horizons=(10, 10)), dict(horizons=(30, 10)), dict(miss_radius=-1.0),
                dict(miss_radius=np.nan), dict(disc_scale=np.inf), dict(disc_scale=-0.5), dict(disc_offset=np.nan), dict(disc_offset=-2.5),
                dict(actor_off=bad_off), dict(actor_off=off1), dict(gt=nan_gt), dict(gt=inf_gt), dict(n_scenes=-1)):
        rc, res = call(**bad)
        assert rc == _lib.MIND_EINVAL, bad
        assert all(np.all(v == 0) for v in res.values()), bad                 # nothing was written
    # more than 2^20 agents: refused on the offsets alone
    big = np.array([0, (1 << 20) + 1], np.int32)
    cfg, B, off, g, v, sc, out, res, keep = _lib.forecast_args(6, 60, [0, 0], np.zeros((0, 60, 2)), np.zeros((0, 60), np.uint8), None, (60,), **CFG, want=("ade",))
    one = np.zeros(8, np.float32)
    rc = lib.mind_debug_forecast_score(C.byref(cfg), 1, big.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), g, v, None,
                                       C.byref(out))
    assert rc == _lib.MIND_EINVAL
    # a non-finite gt at an INVALID sample is nobody's business
    ok_gt = b["gt"].copy()
    ok_gt[1, 7] = np.nan
    rc, res = call(gt=ok_gt)
    assert rc == _lib.MIND_OK and np.array_equal(res["ade"], call()[1]["ade"], equal_nan=True)
    # no scene: a successful no-op that writes nothing
    rc, res = call(n_scenes=0)
    assert rc == _lib.MIND_OK and np.all(res["ade"] == 0)
    with pytest.raises(ValueError):
        _lib.forecast_score_host(b["reg"], b["cls"], b["actor_off"], b["gt"][:, :30], b["valid"])
    with pytest.raises(ValueError):
        _lib.forecast_score_host(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], horizons=(61,))
