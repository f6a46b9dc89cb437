"""CPU: the geometry of the time-to-collision audit (mind_amd/csrc/ttc_geom.h through the host entry mind_debug_box_ttc) against its numpy
restatement (tests/ttc_geom_restate.py) bit for bit, exact cases at yaw = 0, an independent check through the clearance geometry
(mind_debug_box_clearance with both boxes moved to the reported time), the library's own sin / cos against numpy's, the four recorded scenes,
and what of the device entry and of mind_amd/audit.py needs no device: argument errors and shape checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_cases as ac
import ttc_cases as tc
import ttc_geom_restate as ts
from mind_amd import _lib, audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf


def _random_pairs(n, seed):
    """rectangles a, b as (x, y, yaw, L, W, vx, vy) at AV2-size coordinates, positions and boxes as tests/test_audit_host.py draws them
    (offsets up to +-300 m, yaw in +-7, a fifth of the pairs near each other); a drives at 0-15 m/s along its heading, b's velocity is a's
    plus a relative velocity of 0-20 m/s in a random direction"""
    g = np.random.default_rng(seed)
    a = np.stack([g.uniform(-6000, 6000, n), g.uniform(-6000, 6000, n), g.uniform(-7, 7, n), g.uniform(0.3, 8, n), g.uniform(0.3, 3, n)], 1)
    off = g.uniform(-300, 300, (n, 2))
    off[::5] = g.uniform(-6, 6, (len(off[::5]), 2))
    b = np.stack([a[:, 0] + off[:, 0], a[:, 1] + off[:, 1], g.uniform(-7, 7, n), g.uniform(0.3, 8, n), g.uniform(0.3, 3, n)], 1)
    va = g.uniform(0, 15, n)[:, None] * np.stack([np.cos(a[:, 2]), np.sin(a[:, 2])], 1)
    w, ang = g.uniform(0, 20, n), g.uniform(-np.pi, np.pi, n)
    # half of the far pairs close in on each other to within a few metres of the centre line, so that many of them meet
    aim = np.arctan2(-off[:, 1], -off[:, 0]) + g.uniform(-0.03, 0.03, n)
    ang = np.where((np.arange(n) % 5 != 0) & (np.arange(n) % 2 == 0), aim, ang)
    vb = va + w[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    return np.concatenate([a, va], 1), np.concatenate([b, vb], 1)


def _trig(a, b):
    return np.stack([np.cos(a[:, 2]), np.sin(a[:, 2]), np.cos(b[:, 2]), np.sin(b[:, 2])], 1)


@pytest.fixture(scope="module")
def pairs():
    a, b = _random_pairs(2000, 21)
    tg = _trig(a, b)
    return a, b, tg, _lib.box_ttc(a, b, tg)


# 4 x 2 boxes at yaw = 0, a at rest at the origin: (b, expected)
EXACT = [((10, 0, 0, 4, 2, -2, 0), 3.0),            # closing at 2 m/s over the 10 - 4 m between the facing edges
         ((10, 0, 0, 4, 2, 2, 0), INF),             # the same pair receding
         ((10, 2, 0, 4, 2, -2, 0), INF),            # 2 m across: the long edges slide along each other (q == 0 on that axis, |p| == R)
         ((3, 0.5, 0, 4, 2, -2, 1), 0.0),           # overlapping now
         ((3, 3, 0, 4, 2, 1, -1), INF),             # the corners graze at t = 1 (dx = 4, dy = 2): the x shadows part as the y shadows meet
         ((10, 0, 0, 4, 2, 0, 0), INF),             # no relative velocity, separated
         ((10, 1.5, 0, 4, 2, -2, 0), 3.0)]          # half a metre of lateral overlap is an overlap


def test_host_entry_is_the_restatement_bit_for_bit(pairs):
    a, b, tg, got = pairs
    want = ts.pairs(a, b, tg)
    assert np.array_equal(got, want), np.abs(got - want)[np.isfinite(want)].max()
    n_inf, n_zero, n_pos = int(np.isinf(got).sum()), int((got == 0.0).sum()), int((np.isfinite(got) & (got > 0)).sum())
    print(f"{len(got)} pairs: {n_inf} never meet, {n_zero} overlap now, {n_pos} meet later (soonest {got[got > 0].min():.3f} s, latest {got[np.isfinite(got)].max():.1f} s)")
    assert n_inf > 100 and n_zero > 20 and n_pos > 100 and not np.isnan(got).any() and np.all(got >= 0.0)
    # the exact cases through both, and two point boxes
    ea = np.array([(0, 0, 0, 4, 2, 0, 0)] * len(EXACT), np.float64)
    eb = np.array([c[0] for c in EXACT], np.float64)
    et = np.array([(1, 0, 1, 0)] * len(EXACT), np.float64)
    assert np.array_equal(_lib.box_ttc(ea, eb, et), ts.pairs(ea, eb, et))
    pa, pb = a.copy(), b.copy()
    pa[:, 3:5] = pb[:, 3:5] = 0.0
    pb[0, :2], pb[0, 5:] = pa[0, :2] + (3.0, 0.0), pa[0, 5:] + (-1.0, 0.0)          # head on
    assert np.all(_lib.box_ttc(pa, pb, tg) == INF) and np.all(ts.pairs(pa[:50], pb[:50], tg[:50]) == INF)


def test_exact_cases_at_yaw_zero():
    A = (0, 0, 0, 4, 2, 0, 0)
    for B, want in EXACT:
        for trig in ([(1, 0, 1, 0)], None):          # (the trig header at 0 is exactly (1, 0))
            got = _lib.box_ttc([A], [B], trig)[0]
            assert got == want, (B, got, want)
    # a common velocity changes nothing: only the relative one is read
    for B, want in EXACT:
        B2 = B[:5] + (B[5] + 7.5, B[6] - 2.25)
        assert _lib.box_ttc([A[:5] + (7.5, -2.25)], [B2])[0] == want
    # the pair the other way round, and a pair crossing at right angles: b (6 x 0.5, trig (0, 1) exactly) comes down on a from 9 m
    assert _lib.box_ttc([EXACT[0][0]], [A])[0] == 3.0
    assert _lib.box_ttc([A], [(0, 9, np.pi / 2, 6, 0.5, 0, -4)], [(1, 0, 0, 1)])[0] == (9.0 - 1.0 - 3.0) / 4.0


def _moved(x, t):
    """boxes (x, y, yaw, L, W, vx, vy) at time t as the rows (x, y, yaw, L, W) of mind_debug_box_clearance"""
    out = x[:, :5].copy()
    out[:, 0] += x[:, 5] * t
    out[:, 1] += x[:, 6] * t
    return out


def test_reported_time_is_the_first_contact_by_the_clearance_geometry(pairs):
    """independent of the closed form: bg_rect_rect (mind_debug_box_clearance, kind 1) of both boxes moved to time t.  At the reported time
    the boxes touch, before it they never overlap, and a pair reported as never meeting does not overlap at 64 times within 3 s.  The bar
    is the 1e-9 m tests/test_audit_host.py::test_own_trig_against_numpy holds this geometry to; the moved world coordinates stay below
    1e5 m here (asserted), where one rounding is 7e-12 m."""
    a, b, tg, ttc = pairs
    fin = np.isfinite(ttc) & (ttc > 0.0)
    assert fin.sum() > 100
    t = ttc[fin]
    assert max(np.abs(_moved(a[fin], t)[:, :2]).max(), np.abs(_moved(b[fin], t)[:, :2]).max()) < 1e5
    at = _lib.box_clearance(1, _moved(a[fin], t), _moved(b[fin], t), tg[fin])
    print(f"{fin.sum()} contacts: max |clearance at ttc| = {np.abs(at).max():.3e} m")
    assert np.abs(at).max() <= 1e-9
    low = INF
    for k in range(32):
        tk = t * (k / 32.0)
        low = min(low, float(_lib.box_clearance(1, _moved(a[fin], tk), _moved(b[fin], tk), tg[fin]).min()))
    never = np.isinf(ttc)
    for tk in np.linspace(0.0, 3.0, 64):
        low = min(low, float(_lib.box_clearance(1, _moved(a[never], tk), _moved(b[never], tk), tg[never]).min()))
    print(f"least clearance before contact / of {never.sum()} pairs that never meet: {low:.3e} m")
    assert low >= -1e-9
    # overlapping now is what the clearance geometry calls a hit (to the same bar: the two sets may differ in a boundary case's last ulp)
    now = _lib.box_clearance(1, a[:, :5], b[:, :5], tg)
    assert np.all(now[ttc == 0.0] < 1e-9) and np.all(now[ttc > 0.0] > -1e-9)


def test_own_trig_against_numpy(pairs):
    """trig = NULL (mind_trig.h on the host) against the restatement fed numpy's cos / sin: both are within an ulp, every later operation is
    the same IEEE operation, and a time is a length over a speed -- so the same 1e-9 m, in seconds x the pair's relative speed (an upper
    bound of the closing speed along any axis)"""
    a, b, tg, want = pairs
    got = _lib.box_ttc(a, b)
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    speed = np.hypot(b[fin, 5] - a[fin, 5], b[fin, 6] - a[fin, 6])
    worst = float((np.abs(got[fin] - want[fin]) * speed).max())
    print(f"max |own trig - numpy trig| x relative speed = {worst:.3e} m")
    assert worst <= 1e-9


@pytest.mark.parametrize("name", ["demo_1", "demo_2", "demo_3", "demo_4"])
def test_recorded_scenes(name):
    w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
    ttc, track = tc.host_steps(ego, exo, valid, boxes, tc.EGO_BOX, 3.0)
    assert len(ttc) == int(w.max_step) + 1 == 546
    # every tenth step once more, pair by pair through the restatement on the same trig
    sub = np.arange(0, len(ttc), 10)
    ca, sa = tc.lib_trig(ego[:, 3])
    for s in sub:
        jj = np.flatnonzero(valid[s, 1:]) + 1
        cb, sb = tc.lib_trig(exo[s, jj, 2])
        pt = [ts.rect_rect_ttc(exo[s, j, 0] - ego[s, 0], exo[s, j, 1] - ego[s, 1], exo[s, j, 3] - ego[s, 2] * ca[s], exo[s, j, 4] - ego[s, 2] * sa[s], ca[s], sa[s],
                               tc.EGO_BOX[0], tc.EGO_BOX[1], cb[i], sb[i], boxes[j, 0], boxes[j, 1]) for i, j in enumerate(jj)]
        assert ts.reduce_tracks(pt, jj, 3.0) == (ttc[s], track[s]), s
    mn, step, trk, hits, first = ts.reduce_ego(ttc, track, tc.BOUND)
    fin = np.isfinite(ttc)
    print(f"{name}: {fin.sum()} of {len(ttc)} steps within 3 s of a collision at constant velocity, {int((ttc == 0).sum())} at 0.0; min {mn:.3f} s at step {step} "
          f"with track {trk}; {hits} steps below {tc.BOUND} s, first {first}")
    assert fin.any() and (~fin).any() and np.all(ttc[fin] <= 3.0) and np.all(ttc >= 0.0)
    assert np.all(track[fin] >= 1) and np.all(track[~fin] == -1) and track[step] == trk
    if name == "demo_1":          # the recorded ego overlaps one track's nominal box for a long stretch (tests/test_audit_host.py)
        assert (ttc == 0.0).any() and mn == 0.0 and hits > 0 and first >= 0 and ttc[first] < tc.BOUND and np.all(ttc[:first] >= tc.BOUND)
        clear, _ = ac.host_episode_steps(ego, exo, valid, boxes)
        assert np.all(clear[ttc == 0.0] < 1e-9) and np.all(clear[ttc > 0.0] > -1e-9)
    else:
        assert not (ttc == 0.0).any() and hits == 0 and first == -1 and mn >= tc.BOUND and np.isfinite(mn)
    # a longer horizon only adds finite steps and moves none
    far, ftrack = tc.host_steps(ego, exo, valid, boxes, tc.EGO_BOX, 8.0)
    assert np.array_equal(far[fin], ttc[fin]) and np.array_equal(ftrack[fin], track[fin]) and np.all(far[~fin] > 3.0)


# ---- error surface --------------------------------------------------------------------------------------------------------------------

def test_entries_fail_cleanly_without_a_context():
    lib = _lib.load()
    box, cfg = _lib.AuditBox(4.5, 2.0, 0.0), _lib.AuditTtcCfg(3.0, 0.95, 0)
    assert lib.mind_audit_ttc(None, C.byref(box), C.byref(cfg), 1, 1, 1, None, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_ttc(-1, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_ttc(1, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_box_ttc(0, None, None, None, None) == _lib.MIND_OK
    assert _lib.box_ttc(np.zeros((0, 7)), np.zeros((0, 7))).shape == (0,)
    with pytest.raises(ValueError):
        _lib.box_ttc(np.zeros((2, 7)), np.zeros((1, 7)))
    with pytest.raises(ValueError):
        _lib.box_ttc(np.zeros((2, 7)), np.zeros((2, 7)), np.zeros((1, 4)))


@pytest.mark.parametrize("name,n_args", [("mind_audit_ttc", 11), ("mind_debug_box_ttc", 5)])
def test_binding_matches_header(name, n_args):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mind_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
    assert m, f"{name} is not declared in include/mind_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    fn = getattr(_lib.load(), name)
    assert len(args) == len(fn.argtypes) == n_args and fn.restype is C.c_int and name in _lib.EXPORTS
    for a, t in zip(args, fn.argtypes):
        assert ("*" in a) == (t is C.c_void_p or hasattr(t, "contents")), (a, t)
    assert C.sizeof(_lib.AuditTtcCfg) == 24 and C.sizeof(_lib.AuditTtcOut) == 56
    assert [f[0] for f in _lib.AuditTtcCfg._fields_] == ["horizon", "bound", "lanes"]
    m = re.search(r"typedef struct \{([^}]*)\} mind_audit_ttc_out;", txt)
    assert re.findall(r"\*\s*(\w+)", m.group(1)) == [f[0] for f in _lib.AuditTtcOut._fields_] == list(tc.KEYS)


def test_predictor_method_checks_its_arguments():
    """HipPredictor.audit_ttc rejects bad shapes and settings before any library call (no context is needed to get that far)"""
    from mind_amd.predictor import HipPredictor
    hp = HipPredictor.__new__(HipPredictor)
    S, n = 5, 3
    ok = dict(ego_states=np.zeros((S, 4)), exo=np.zeros((S, n, 5)), valid=np.zeros((S, n), np.uint8), boxes=np.ones((n, 2)), ego_box=(4.5, 2.0))
    for key, bad, msg in (("ego_states", np.zeros((S, 3)), "ego_states"), ("exo", np.zeros((S + 1, n, 5)), "exo must be"),
                          ("valid", np.zeros((S, n + 1), np.uint8), "valid must be"), ("boxes", np.ones((n, 3)), "valid must be"),
                          ("boxes", -np.ones((n, 2)), "boxes must be"), ("ego_box", (1.0,), "ego_box"), ("horizon", 0.0, "horizon"),
                          ("horizon", np.inf, "horizon"), ("horizon", np.nan, "horizon"), ("bound", -0.1, "bound"), ("bound", np.nan, "bound"),
                          ("lanes", 3, "lanes"), ("lanes", -1, "lanes")):
        with pytest.raises(ValueError, match=msg):
            hp.audit_ttc(**dict(ok, **{key: bad}))


class _Runtime:
    """stands in for HipPredictor: records the calls, answers with arrays of the right shapes"""

    def __init__(self):
        self.calls = []

    def audit_ttc(self, ego, exo, valid, boxes, ego_box, horizon, bound):
        self.calls.append((ego, exo, valid, boxes, ego_box, horizon, bound))
        E, S = ego.shape[:2]
        ttc = np.tile(np.array([INF, 0.5, 1.0, 0.25, INF])[:S], (E, 1))
        return dict(step_ttc=ttc, step_track=np.where(np.isfinite(ttc), 2, -1).astype(np.int32), ego_min=np.full(E, 0.25), ego_step=np.full(E, 3, np.int32),
                    ego_track=np.full(E, 2, np.int32), ego_hits=np.full(E, 2, np.int32), ego_first=np.ones(E, np.int32))


def test_episode_ttc_auditor_records_and_reports_once():
    class World:
        n_agents, agent_ids = 3, ["AV", "a", "b"]

        def agent_state(self, i, t):
            return np.array([10.0 * i + t, float(i), 1.0, 0.0])

        def object_type(self, i):
            return ("vehicle", "pedestrian", "bus")[i]

        def is_valid(self, i, t):
            return not (i == 2 and t == 0.0)

    class Sim:
        def __init__(self):
            self.world, self.sim_time, self.enabled, self.state, self.n = World(), 0.0, False, np.array([-1.0, -1.0, 0.0, 0.0]), 0

        def step(self):
            self.sim_time += 0.02
            self.n += 1
            self.enabled = self.n >= 3
            return False

    rt, sim = _Runtime(), Sim()
    au = audit.EpisodeTtcAuditor(sim, runtime=rt).run(5)
    assert sim.n == 5 and not rt.calls and au.step.__func__ is audit.EpisodeAuditor.step
    rep = au.report()
    assert len(rt.calls) == 1
    ego, exo, valid, boxes, box, horizon, bound = rt.calls[0]
    assert ego.shape == (1, 5, 4) and exo.shape == (5, 3, 5) and valid.shape == (5, 3) and box == (4.5, 2.0) and (horizon, bound) == (3.0, 0.95)
    assert np.array_equal(rep["times"], ac.sim_times(5)) and rep["enabled"].tolist() == [False, False, False, True, True]
    assert exo[1, 1, 3] == 1.0 and exo[1, 1, 4] == 0.0 and valid[:, 2].tolist() == [0, 1, 1, 1, 1]          # the tracks' velocities are tabulated
    assert set(rep) == {"times", "enabled", "step_ttc", "step_track", "ego_min", "ego_step", "ego_track", "ego_hits", "ego_first", "before", "after"}
    # the split at the take-over: steps 0..2 before (inf, 0.5, 1.0), 3..4 after (0.25, inf); a hit is ttc < 0.95
    b, a = rep["before"], rep["after"]
    assert b["steps"].tolist() == [0, 1, 2] and (b["ego_min"], b["ego_step"], b["ego_track"], b["ego_hits"], b["ego_first"]) == (0.5, 1, 2, 1, 1)
    assert a["steps"].tolist() == [3, 4] and (a["ego_min"], a["ego_step"], a["ego_track"], a["ego_hits"], a["ego_first"]) == (0.25, 3, 2, 1, 3)
    assert (rep["ego_min"], rep["ego_step"], rep["ego_hits"], rep["ego_first"]) == (0.25, 3, 2, 1)
    # another bound moves the parts' hits with it; the bar of the other auditors stays 0.0
    au2 = audit.EpisodeTtcAuditor(Sim(), ego_box=(5.0, 2.2, 1.4), horizon=5.0, bound=1.0, runtime=rt).run(5)
    rep2 = au2.report()
    assert rt.calls[1][4:] == ((5.0, 2.2, 1.4), 5.0, 1.0) and rep2["before"]["ego_hits"] == 1 and rep2["after"]["ego_hits"] == 1
    au3 = audit.EpisodeTtcAuditor(Sim(), bound=1.5, runtime=rt).run(5)
    assert au3.report()["before"]["ego_hits"] == 2
    per = dict(step_clear=np.array([0.5, -1.0]), step_track=np.array([1, 2], np.int32))
    assert audit._part(per, np.arange(2), "step_clear", "track", nan_step=False)["ego_hits"] == 1
    with pytest.raises(RuntimeError):
        audit.EpisodeTtcAuditor(Sim(), runtime=rt).report()
