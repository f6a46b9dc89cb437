"""numpy restatement of mind_amd/csrc/forecast_score.h, operation for operation (float64 after the float32 inputs are widened, no fused
multiply-add: numpy evaluates every operator on its own).  Sums are taken with np.cumsum, which adds sequentially along its axis; a sample
that does not count enters as +0.0, which leaves a running sum of non-negative terms (and a NaN or inf one) unchanged.  np.sum / np.mean
add pairwise and are not used.  Not a test module."""
import numpy as np

NAMES_A3 = ("ade", "fde", "cover", "first_out")
NAMES_A2 = ("n_valid", "last", "k_ade", "k_fde", "brier_fde")
NAMES_S = ("s_n_scored", "s_ade", "s_fde", "s_k_ade", "s_k_fde", "s_k_top", "s_brier_fde", "s_miss_rate", "s_miss_top")


def samples(reg, gt, disc_scale, disc_offset):
    """fs_sample over [A, K, T]: d float64, inside bool"""
    x, y = reg[..., 0].astype(np.float64), reg[..., 1].astype(np.float64)
    dx, dy = x - gt[:, None, :, 0], y - gt[:, None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt(dx * dx + dy * dy)
        r = np.float64(disc_scale) * np.fmax(reg[..., 2], reg[..., 3]).astype(np.float64) + np.float64(disc_offset)
        inside = d <= r
    return d, inside


def argmin_c(v):
    """`best = +inf, k = -1; for k ascending: if (v < best) take it` along the last axis"""
    best, kb = np.full(v.shape[:-1], np.inf), np.full(v.shape[:-1], -1, np.int32)
    for k in range(v.shape[-1]):
        with np.errstate(invalid="ignore"):
            m = v[..., k] < best
        best, kb = np.where(m, v[..., k], best), np.where(m, np.int32(k), kb)
    return kb


def argmax_c(cls):
    best, kb = np.full(cls.shape[:-1], -np.inf, np.float32), np.full(cls.shape[:-1], -1, np.int32)
    for k in range(cls.shape[-1]):
        with np.errstate(invalid="ignore"):
            m = cls[..., k] > best
        best, kb = np.where(m, cls[..., k], best), np.where(m, np.int32(k), kb)
    return kb


def brier(fde, p):
    q = 1.0 - p.astype(np.float64)
    return fde + q * q


def _pick(v, k):
    """v[..., k] with NaN for k == -1"""
    g = np.take_along_axis(v, np.maximum(k, 0)[..., None].astype(np.int64), axis=-1)[..., 0]
    return np.where(k >= 0, g, np.nan)


def score(reg, cls, actor_off, gt, valid, scored=None, horizons=(60,), miss_radius=2.0, disc_scale=1.0, disc_offset=0.0):
    """every output of mind_forecast_score, by the header's rules"""
    reg, cls = np.asarray(reg, np.float32), np.asarray(cls, np.float32)
    A, K, T = reg.shape[:3]
    B, H = len(actor_off) - 1, len(horizons)
    d, inside = samples(reg, gt, disc_scale, disc_offset)
    ok = (np.asarray(valid) != 0)[:, None, :] & np.ones((1, K, 1), bool)              # [A, K, T]
    with np.errstate(invalid="ignore"):
        run_sum = np.cumsum(np.where(ok, d, 0.0), axis=2)
    run_n = np.cumsum(ok, axis=2).astype(np.int32)
    run_cover = np.cumsum(ok & inside, axis=2).astype(np.int32)
    tt = np.arange(T)
    run_last = np.maximum.accumulate(np.where(ok, tt, -1), axis=2).astype(np.int32)
    out_t = np.where(ok & ~inside, tt, T)                                             # first valid sample not inside: a running minimum
    run_first = np.minimum.accumulate(out_t, axis=2)
    run_first = np.where(run_first == T, -1, run_first).astype(np.int32)
    o = dict(ade=np.zeros((A, H, K)), fde=np.zeros((A, H, K)), cover=np.zeros((A, H, K), np.int32), first_out=np.zeros((A, H, K), np.int32),
             n_valid=np.zeros((A, H), np.int32), last=np.zeros((A, H), np.int32))
    for h, hz in enumerate(horizons):
        e = hz - 1
        n, last = run_n[:, :, e], run_last[:, :, e]
        with np.errstate(invalid="ignore", divide="ignore"):
            o["ade"][:, h] = np.where(n > 0, run_sum[:, :, e] / np.where(n > 0, n, 1).astype(np.float64), np.nan)
        o["fde"][:, h] = np.where(n > 0, np.take_along_axis(d, np.maximum(last, 0)[..., None].astype(np.int64), axis=2)[..., 0], np.nan)
        o["cover"][:, h], o["first_out"][:, h] = run_cover[:, :, e], run_first[:, :, e]
        o["n_valid"][:, h], o["last"][:, h] = n[:, 0], last[:, 0]
    o["k_ade"], o["k_fde"] = argmin_c(o["ade"]), argmin_c(o["fde"])
    scene_of = np.repeat(np.arange(B), np.diff(actor_off))
    p = np.take_along_axis(cls[scene_of][:, None, :] * np.ones((1, H, 1), np.float32), np.maximum(o["k_fde"], 0)[..., None].astype(np.int64), axis=2)[..., 0]
    with np.errstate(invalid="ignore"):
        o["brier_fde"] = np.where(o["k_fde"] >= 0, brier(_pick(o["fde"], o["k_fde"]), p), np.nan)
    # the scene rows: agents in index order, sequential sums from 0.0
    o.update(s_n_scored=np.zeros((B, H), np.int32), s_ade=np.full((B, H, K), np.nan), s_fde=np.full((B, H, K), np.nan), s_k_top=np.zeros((B, H), np.int32),
             s_miss_rate=np.full((B, H), np.nan), s_miss_top=np.full((B, H), np.nan))
    sc = np.ones(A, bool) if scored is None else np.asarray(scored) != 0
    miss = np.zeros((B, H, K), np.int32)
    for b in range(B):
        for h in range(H):
            rows = np.array([a for a in range(actor_off[b], actor_off[b + 1]) if sc[a] and o["n_valid"][a, h] > 0], np.int64)
            n = len(rows)
            o["s_n_scored"][b, h] = n
            if n:
                zero = np.zeros((1, K))
                with np.errstate(invalid="ignore"):
                    o["s_ade"][b, h] = np.cumsum(np.concatenate([zero, o["ade"][rows, h]]), axis=0)[-1] / np.float64(n)
                    o["s_fde"][b, h] = np.cumsum(np.concatenate([zero, o["fde"][rows, h]]), axis=0)[-1] / np.float64(n)
                    miss[b, h] = (o["fde"][rows, h] > np.float64(miss_radius)).sum(axis=0)
    o["s_k_ade"], o["s_k_fde"] = argmin_c(o["s_ade"]), argmin_c(o["s_fde"])
    o["s_k_top"][:] = argmax_c(cls)[:, None]
    ps = np.take_along_axis(cls[:, None, :] * np.ones((1, H, 1), np.float32), np.maximum(o["s_k_fde"], 0)[..., None].astype(np.int64), axis=2)[..., 0]
    with np.errstate(invalid="ignore"):
        o["s_brier_fde"] = np.where(o["s_k_fde"] >= 0, brier(_pick(o["s_fde"], o["s_k_fde"]), ps), np.nan)
    n = o["s_n_scored"]
    for key, k in (("s_miss_rate", o["s_k_fde"]), ("s_miss_top", o["s_k_top"])):
        m = np.take_along_axis(miss, np.maximum(k, 0)[..., None].astype(np.int64), axis=2)[..., 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            o[key] = np.where((n > 0) & (k >= 0), m.astype(np.float64) / np.where(n > 0, n, 1).astype(np.float64), np.nan)
    return o
