"""Shared by tests/test_ttc_host.py and tests/test_gpu_ttc.py: the time-to-collision audit evaluated through the library's HOST entry
(mind_debug_box_ttc, all pairs of a trace in one call) and reduced by the restatement's rules (tests/ttc_geom_restate.py).  The kernel forms
the ego's velocity as v (cos yaw, sin yaw) with the library's own sin / cos, so the host text is handed that trig: mind_trig.h as the C
oracle compiles it (``oracle_sincos``; tests/test_gpu_ilqr.py holds the device to those bits).  Not a test module."""
import ctypes as C

import numpy as np

import ttc_geom_restate as ts
from mind_amd import _lib, audit

EGO_BOX = audit.BOXES["VEHICLE"]
HORIZON, BOUND = audit.DEFAULT_TTC_HORIZON, audit.DEFAULT_TTC_BOUND
KEYS = ("step_ttc", "step_track", "ego_min", "ego_step", "ego_track", "ego_hits", "ego_first")


def lib_trig(yaw):
    """(cos, sin) of an array of angles by mind_trig.h on the host"""
    from oracle import ilqr as oi
    f = oi.lib().oracle_sincos
    f.restype = None
    yaw = np.asarray(yaw, np.float64)
    c, s = np.zeros(yaw.shape), np.zeros(yaw.shape)
    sv, cv = C.c_double(), C.c_double()
    for i, v in enumerate(yaw.ravel()):
        f(C.c_double(float(v)), C.byref(sv), C.byref(cv))
        s.ravel()[i], c.ravel()[i] = sv.value, cv.value
    return c, s


def numpy_trig(yaw):
    return np.cos(yaw), np.sin(yaw)


def host_steps(ego, exo, valid, boxes, ego_box=EGO_BOX, horizon=HORIZON, trig=lib_trig):
    """step_ttc [S] / step_track [S] of one ego trace [S, 4] = (x, y, v, yaw), pairs through the host entry.  A non-zero center_offset moves
    the ego's centre by hand (the kernel subtracts it from the offset: equal to rounding, not bit for bit)"""
    S, n = valid.shape
    ttc, track = np.full(S, np.inf), np.full(S, -1, np.int32)
    ss, jj = np.nonzero(valid[:, 1:])
    jj = jj + 1
    if len(ss):
        ca, sa = trig(ego[:, 3])
        off = ego_box[2] if len(ego_box) == 3 else 0.0
        cx, cy = (ego[:, 0] + off * ca, ego[:, 1] + off * sa) if off != 0.0 else (ego[:, 0], ego[:, 1])
        m = len(ss)
        A = np.stack([cx[ss], cy[ss], ego[ss, 3], np.full(m, ego_box[0]), np.full(m, ego_box[1]), ego[ss, 2] * ca[ss], ego[ss, 2] * sa[ss]], 1)
        B = np.stack([exo[ss, jj, 0], exo[ss, jj, 1], exo[ss, jj, 2], boxes[jj, 0], boxes[jj, 1], exo[ss, jj, 3], exo[ss, jj, 4]], 1)
        cb, sb = trig(B[:, 2])
        t = _lib.box_ttc(A, B, np.stack([ca[ss], sa[ss], cb, sb], 1))
        lo = np.searchsorted(ss, np.arange(S + 1))          # (np.nonzero: steps ascending, tracks ascending within a step)
        for s in range(S):
            ttc[s], track[s] = ts.reduce_tracks(t[lo[s]:lo[s + 1]], jj[lo[s]:lo[s + 1]], horizon)
    return ttc, track


def host_ttc(egos, exo, valid, boxes, ego_box=EGO_BOX, horizon=HORIZON, bound=BOUND, trig=lib_trig):
    """what HipPredictor.audit_ttc returns, from the host entry + the restatement's reductions; egos [E, S, 4]"""
    E, S = egos.shape[:2]
    out = dict(step_ttc=np.zeros((E, S)), step_track=np.zeros((E, S), np.int32), ego_min=np.zeros(E), ego_step=np.zeros(E, np.int32),
               ego_track=np.zeros(E, np.int32), ego_hits=np.zeros(E, np.int32), ego_first=np.zeros(E, np.int32))
    for e in range(E):
        out["step_ttc"][e], out["step_track"][e] = host_steps(egos[e], exo, valid, boxes, ego_box, horizon, trig)
        for k, v in zip(KEYS[2:], ts.reduce_ego(out["step_ttc"][e], out["step_track"][e], bound)):
            out[k][e] = v
    return out


def same(got, want, what=""):
    assert set(got) == set(want) == set(KEYS), (what, sorted(got))
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), (what, k, got[k], w)
