"""float64 restatement of SceneDecoder's curve step (planners/mind/networks/network.py:449-481, :514-534, :545) for the decoder-aux tests,
the error bound those tests hold the device to, and a numpy emulation of the device's fp32 chain (used on the CPU to check the bound itself).

The bound.  Every linear output is o = sum_c t_c p_c over n <= 8 terms, with t_c an fp32-rounded table entry (relative error u = 2^-24), p_c
a control point or an fp32 difference of two (u), accumulated by n fused multiply-adds (one rounding each) and, for the two derivatives,
divided by 6 (u): |o_dev - o_64| <= gamma_{n+3} S with S = sum_c |t_c| |p_c| and gamma_k = k u / (1 - k u) < 11 u for k = 11 -- rounded up to
16 u.  The three exp outputs carry that as an error of the argument, i.e. as a relative error of the result, plus expf's own (4 u covers the
2-ulp class of the device's expf with room): rel <= 16 u S + 4 u."""
import math

import numpy as np

U = 2.0 ** -24
GRID = np.linspace(0.0, 1.0, 60, endpoint=True)


def tables64(basis, ts):
    """network.py:449-481 in float64 at the times ts (fractions of the horizon): (T [n,8], Tp [n,7])"""
    ts = np.asarray(ts, np.float64)
    if basis == "bezier":
        T = [math.comb(7, i) * (1.0 - ts) ** (7 - i) * ts ** i for i in range(8)]
        Tp = [7 * math.comb(6, i) * (1.0 - ts) ** (6 - i) * ts ** i for i in range(7)]
    else:
        assert basis == "monomial", basis
        T = [ts ** i for i in range(8)]
        Tp = [(i + 1) * (ts ** i) for i in range(7)]
    return np.array(T).T, np.array(Tp).T


def _vel_terms(P, basis):
    """what Tp multiplies for the positions: diff under Bezier (network.py:519), P[1:] under monomial (:530)"""
    return np.diff(P, axis=-2) if basis == "bezier" else P[..., 1:, :]


def curves64(param, basis, ts):
    """param [..., 8, 5] -> dict of float64 (value, S) pairs: reg_lin [..., n, 5] (positions and the exp ARGUMENTS), vel [..., n, 2],
    cov_vel [..., n, 3]; S = sum_c |t_c| |p_c| of the same shape (after the division by 6 for the two derivatives)"""
    p = np.asarray(param, np.float64)
    T, Tp = tables64(basis, ts)
    dv, dc = _vel_terms(p[..., :2], basis), np.diff(p[..., 2:], axis=-2)       # cov_vel: diff under both bases (:523 / :534)
    mm = lambda M, X: np.einsum("tc,...cd->...td", M, X)
    return {"reg_lin": (mm(T, p), mm(np.abs(T), np.abs(p))),
            "vel": (mm(Tp, dv) / 6.0, mm(np.abs(Tp), np.abs(dv)) / 6.0),
            "cov_vel": (mm(Tp, dc) / 6.0, mm(np.abs(Tp), np.abs(dc)) / 6.0)}


def reference64(param, basis, ts):
    """the reference's outputs in float64: reg [..., n, 5] = (x, y, exp sx, exp sy, exp rho), vel, cov_vel"""
    c = curves64(param, basis, ts)
    reg = c["reg_lin"][0].copy()
    reg[..., 2:] = np.exp(reg[..., 2:])
    return reg, c["vel"][0], c["cov_vel"][0]


def bound_violations(param, basis, ts, reg=None, vel=None, cov_vel=None):
    """worst (error / bound) per output over everything given, > 1 = outside the bound; dict name -> float"""
    c = curves64(param, basis, ts)
    worst = {}

    def lin(name, dev, val, S):
        err, lim = np.abs(np.asarray(dev, np.float64) - val), 16 * U * S
        assert np.isfinite(err).all(), name
        worst[name] = float(np.max(np.where(err == 0, 0.0, err / np.maximum(lim, 1e-300))))

    if reg is not None:
        val, S = c["reg_lin"]
        lin("pos", reg[..., :2], val[..., :2], S[..., :2])
        e64 = np.exp(val[..., 2:])
        rel, lim = np.abs(np.asarray(reg[..., 2:], np.float64) - e64) / e64, 16 * U * S[..., 2:] + 4 * U
        assert np.isfinite(rel).all()
        worst["cov"] = float(np.max(rel / lim))
    if vel is not None:
        lin("vel", vel, *c["vel"])
    if cov_vel is not None:
        lin("cov_vel", cov_vel, *c["cov_vel"])
    return worst


def emulate_fp32(param, basis, T32, Tp32):
    """the device's chain in numpy: fp32 tables, fmaf over the control points in order (the product of two fp32 is exact in float64; the sum is
    rounded once to float64 and once to fp32 -- a double rounding the device does not have, within the bound's slack), fp32 difference, expf as
    float32(exp(float64)), / 6 in fp32.  -> reg, vel, cov_vel float32"""
    p = np.asarray(param, np.float32)
    f32 = np.float32

    def contract(M, X):      # M [n, C] fp32, X [..., C, D] fp32 -> [..., n, D]
        acc = np.zeros(X.shape[:-2] + (M.shape[0], X.shape[-1]), np.float32)
        for c in range(M.shape[1]):
            acc = (M[:, c].astype(np.float64)[:, None] * X[..., c, :].astype(np.float64)[..., None, :] + acc.astype(np.float64)).astype(f32)
        return acc

    lin = contract(T32, p)
    reg = lin.copy()
    reg[..., 2:] = np.exp(lin[..., 2:].astype(np.float64)).astype(f32)
    dv = (p[..., 1:, :2] - p[..., :-1, :2]).astype(f32) if basis == "bezier" else p[..., 1:, :2]
    dc = (p[..., 1:, 2:] - p[..., :-1, 2:]).astype(f32)
    return reg, (contract(Tp32, dv) / f32(6.0)).astype(f32), (contract(Tp32, dc) / f32(6.0)).astype(f32)
