"""GPU: the time-to-collision audit on the device (mind_audit_ttc / k_audit_ttc<1>, k_audit_ttc<2>, mind_amd/audit.py) against the library's HOST
evaluation of the same header (mind_debug_box_ttc, pair by pair, handed mind_trig.h's sin / cos) reduced by the restatement's rules
(tests/ttc_geom_restate.py, tests/ttc_cases.py): every output bit for bit, in both lane layouts and under the library's own choice.  The
minimum over the tracks is taken on the lexicographic order (ttc, track), which is associative and commutative, so the cross-lane fold of
the track-lane layout owes the sequential scan every bit."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import audit_cases as ac
import ilqr_policy_restate as pr
import ttc_cases as tc
from mind_amd import _lib, audit
from mind_amd.predictor import IlqrCall
from oracle import ilqr as oi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LAYOUTS = (1, 2, 0)          # thread per ego, lanes over tracks, the library's rule
TCH = 64                     # tracks per LDS staging turn = lanes of a wavefront (AU_TCH)


def _all_layouts(hp, egos, exo, valid, boxes, box=tc.EGO_BOX, horizon=tc.HORIZON, bound=tc.BOUND, want=None, what=""):
    """the call in every layout, each held to the host text (or to `want`) -> the last result"""
    if want is None:
        want = tc.host_ttc(egos if egos.ndim == 3 else egos[None], exo, valid, boxes, box, horizon, bound)
    for lanes in LAYOUTS:
        got = hp.audit_ttc(egos, exo, valid, boxes, box, horizon, bound, lanes)
        tc.same(got, want, (what, "lanes", lanes))
    return got


@pytest.mark.parametrize("name,n", [("demo_1", 40), ("demo_3", 16)])
def test_device_is_the_host_text(hip_predictor, name, n):
    w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
    assert ego.shape == (546, 4) and exo.shape == (546, n, 5)
    one = _all_layouts(hip_predictor, ego, exo, valid, boxes, what=name)
    fin = np.isfinite(one["step_ttc"][0])
    assert fin.any() and (~fin).any() and np.all(one["step_track"][0][~fin] == -1) and np.all(one["step_track"][0][fin] >= 1)
    if name == "demo_1":
        assert one["ego_min"][0] == 0.0 and one["ego_hits"][0] > 0 and one["step_track"][0, one["ego_step"][0]] == one["ego_track"][0] >= 1
    else:
        assert one["ego_hits"][0] == 0 and one["ego_first"][0] == -1 and tc.BOUND <= one["ego_min"][0] <= tc.HORIZON
    egos = np.stack([ego, ego + np.array([1.5, -0.75, 0, 0]), ego + np.array([-3.0, 2.0, 0.5, 0])])
    three = _all_layouts(hip_predictor, egos, exo, valid, boxes, what=name + " x 3")
    assert np.array_equal(three["step_ttc"][0], one["step_ttc"][0])
    # a step on which every track is invalid; and more egos than one workgroup of the thread-per-ego layout takes
    v2 = valid.copy()
    v2[10] = 0
    many = np.stack([ego[:40] + np.array([0.01 * k, 0, 0.02 * k, 0]) for k in range(65)])
    got = _all_layouts(hip_predictor, many, exo[:40], v2[:40], boxes, what=name + " x 65")
    assert np.all(got["step_ttc"][:, 10] == np.inf) and np.all(got["step_track"][:, 10] == -1)


def test_layouts_agree_where_the_library_rule_changes_sides(hip_predictor):
    """61 traces x 546 steps = 33 306 rows, past the 2^15 rows up to which the library's rule takes the track lanes: all three calls agree
    byte for byte, and the first and the last trace are the host text"""
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_3")
    egos = np.stack([ego + np.array([0.05 * k, -0.02 * k, 0.01 * k, 0]) for k in range(61)])
    assert egos.shape[0] * egos.shape[1] > 1 << 15
    got = [hip_predictor.audit_ttc(egos, exo, valid, boxes, tc.EGO_BOX, lanes=lanes) for lanes in LAYOUTS]
    for g in got[1:]:
        assert _bytes(g) == _bytes(got[0])
    want = tc.host_ttc(egos[[0, 60]], exo, valid, boxes)
    tc.same({k: v[[0, 60]] for k, v in got[2].items()}, want)
    assert np.isfinite(got[2]["step_ttc"]).any()


def _synth(n, S, seed):
    """S steps of n tracks about an ego near the origin: positions within 60 m, any heading, speeds up to 15 m/s, validity 0.8"""
    g = np.random.default_rng(seed)
    exo = np.zeros((S, n, 5))
    exo[:, :, 0], exo[:, :, 1], exo[:, :, 2] = g.uniform(-60, 60, (S, n)), g.uniform(-60, 60, (S, n)), g.uniform(-7, 7, (S, n))
    sp = g.uniform(0, 15, (S, n))
    exo[:, :, 3], exo[:, :, 4] = sp * np.cos(exo[:, :, 2]), sp * np.sin(exo[:, :, 2])
    valid = (g.uniform(size=(S, n)) < 0.8).astype(np.uint8)
    boxes = np.stack([g.uniform(0.5, 7, n), g.uniform(0.5, 2.5, n)], 1)
    egos = np.stack([g.uniform(-3, 3, (2, S)), g.uniform(-3, 3, (2, S)), g.uniform(0, 12, (2, S)), g.uniform(-3, 3, (2, S))], 2)
    return egos, exo, valid, boxes


def test_edges(hip_predictor):
    hp = hip_predictor
    # S = 1, n = 1: the ego alone
    for lanes in LAYOUTS:
        r = hp.audit_ttc(np.zeros((1, 4)), np.zeros((1, 1, 5)), np.zeros((1, 1), np.uint8), np.ones((1, 2)), tc.EGO_BOX, lanes=lanes)
        assert r["step_ttc"][0, 0] == np.inf and r["step_track"][0, 0] == -1 and r["ego_min"][0] == np.inf
        assert (r["ego_step"][0], r["ego_track"][0], r["ego_hits"][0], r["ego_first"][0]) == (0, -1, 0, -1)
    # track counts about the staging turn and the wavefront: exactly one turn of 64 tracks beside the ego's row, one more, two turns and two
    # more.  On step 0 the last track sits on the first ego (ttc 0.0): the turn that holds one or two tracks decides
    for n in (TCH + 1, TCH + 2, 2 * TCH + 3):
        egos, exo, valid, boxes = _synth(n, 3, n)
        exo[0, n - 1, :2], valid[0, n - 1] = egos[0, 0, :2], 1
        got = _all_layouts(hp, egos, exo, valid, boxes, horizon=8.0, what=("synth", n))
        assert got["step_ttc"][0, 0] == 0.0 and got["step_track"][0, 0] == n - 1
        assert (np.isfinite(got["step_ttc"]) & (got["step_ttc"] > 0.0)).sum() >= 3
    # two tracks mirrored in the ego's axis, in different staging turns and different lanes: equal ttc, the lower is named.  The ego drives
    # along x at 4 m/s; the two come in from the sides at 2 m/s and meet its flanks after exactly 2 s; every other track of the step
    # shares the ego's velocity (no relative motion: never)
    n, S = 2 * TCH + 3, 3
    egos, exo, valid, boxes = _synth(n, S, 5)
    ego = np.zeros((S, 4))
    ego[:, 2] = 4.0
    exo[1, :, 0], exo[1, :, 1], exo[1, :, 3], exo[1, :, 4] = np.linspace(-60, 60, n), 30.0, 4.0, 0.0
    exo[1, 70], exo[1, 129], boxes[70], boxes[129] = (12, 6, 0, 0, -2), (12, -6, 0, 0, 2), (4, 2), (4, 2)
    valid[1, 70] = valid[1, 129] = 1
    assert (70 - 1) // TCH != (129 - 1) // TCH and (70 - 1) % TCH != (129 - 1) % TCH
    got = _all_layouts(hp, ego, exo, valid, boxes, horizon=8.0, what="mirrored")
    assert got["step_ttc"][0, 1] == 2.0 and got["step_track"][0, 1] == 70
    alone = valid.copy()
    alone[1, 70] = 0
    assert _all_layouts(hp, ego, exo, alone, boxes, horizon=8.0, what="mirrored, the upper alone")["step_track"][0, 1] == 129
    # the horizon: a minimum above it is +inf / -1, one equal to it is reported
    only = np.zeros_like(valid)
    only[1, 70] = only[1, 129] = 1
    for horizon, want in ((1.5, (np.inf, -1)), (2.0, (2.0, 70)), (np.nextafter(2.0, 0.0), (np.inf, -1))):
        got = _all_layouts(hp, ego, exo, only, boxes, horizon=horizon, what=("horizon", horizon))
        assert (got["step_ttc"][0, 1], got["step_track"][0, 1]) == want
        assert np.all(got["step_ttc"][0, [0, 2]] == np.inf) and got["ego_step"][0] == (1 if want[1] > 0 else 0) and got["ego_track"][0] == want[1]
    # the bound is strict: a step at exactly `bound` is no hit
    for bound, hits, first in ((2.0, 0, -1), (np.nextafter(2.0, 3.0), 1, 1), (0.0, 0, -1)):
        got = _all_layouts(hp, ego, exo, only, boxes, horizon=3.0, bound=bound, what=("bound", bound))
        assert (got["ego_min"][0], got["ego_step"][0], got["ego_track"][0], got["ego_hits"][0], got["ego_first"][0]) == (2.0, 1, 70, hits, first)


def test_centre_offset_moves_the_contact_time_as_the_shifted_box_says(hip_predictor):
    hp = hip_predictor
    # exact: the ego drives along x at 4 m/s towards a 4 x 2 box at rest 12 m ahead; its own 4.5 m box carried 1.5 m forward meets it 1.5 / 4 s sooner
    ego, exo, valid, boxes = np.array([[0.0, 0, 4, 0]]), np.zeros((1, 2, 5)), np.array([[0, 1]], np.uint8), np.array([[1, 1], [4, 2.0]])
    exo[0, 1, 0] = 12.0
    for lanes in LAYOUTS:
        assert hp.audit_ttc(ego, exo, valid, boxes, (4.5, 2.0), lanes=lanes)["step_ttc"][0, 0] == (12.0 - 2.0 - 2.25) / 4.0
        assert hp.audit_ttc(ego, exo, valid, boxes, (4.5, 2.0, 1.5), lanes=lanes)["step_ttc"][0, 0] == (12.0 - 1.5 - 2.0 - 2.25) / 4.0
    # the recorded demo_1 trace: center_offset o at state (x, y, yaw) is the box of offset 0 at (x + o cos yaw, y + o sin yaw), to the rounding
    # of the moved centre (1e-12 m at these coordinates): the host text of the box moved by hand, to 1e-9 m in seconds x relative speed
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_1")
    o = 1.4
    want, wtrack = tc.host_steps(ego, exo, valid, boxes, tc.EGO_BOX + (o,))
    base = tc.host_steps(ego, exo, valid, boxes, tc.EGO_BOX)[0]
    assert not np.array_equal(want, base)
    for lanes in LAYOUTS:
        got = hp.audit_ttc(ego, exo, valid, boxes, tc.EGO_BOX + (o,), lanes=lanes)
        assert np.array_equal(got["step_track"][0], wtrack) and np.array_equal(np.isinf(got["step_ttc"][0]), np.isinf(want))
        fin = np.isfinite(want)
        j = wtrack[fin]
        speed = np.hypot(exo[fin, j, 3] - ego[fin, 2] * np.cos(ego[fin, 3]), exo[fin, j, 4] - ego[fin, 2] * np.sin(ego[fin, 3]))
        assert (np.abs(got["step_ttc"][0][fin] - want[fin]) * speed).max() <= 1e-9


def _bytes(res):
    return {k: (a.dtype.str, a.shape, a.tobytes()) for k, a in res.items()}


def test_scratch_is_shared_with_the_clearance_audit(hip_predictor):
    """mind_audit_ttc runs on the scratch buffer of the other audits: interleaved with mind_audit_episode on one context, every call behind
    a call that left other bytes in the buffer -- the call without a track beside the ego's row, which skips the scene's upload, right
    behind the largest -- each returns what it returns on a fresh context, bit for bit"""
    from mind_amd.predictor import HipPredictor
    egos, exo, valid, boxes = _synth(TCH + 2, 3, 9)
    box = (4.5, 2.0, 1.2)
    calls = dict(ttc=lambda hp: hp.audit_ttc(egos, exo, valid, boxes, box, 8.0, 2.0, 2),
                 ttc_egos=lambda hp: hp.audit_ttc(egos, exo, valid, boxes, box, 8.0, 2.0, 1),
                 ttc_alone=lambda hp: hp.audit_ttc(egos, exo[:, :1], valid[:, :1], boxes[:1], box),
                 episode=lambda hp: hp.audit_episode(egos, exo, valid, boxes, box),
                 episode_alone=lambda hp: hp.audit_episode(egos, exo[:, :1], valid[:, :1], boxes[:1], box))
    want = {}
    for name in ("ttc", "ttc_alone", "episode", "episode_alone"):
        fresh = HipPredictor(0)
        try:
            want[name] = _bytes(calls[name](fresh))
        finally:
            fresh.close()
    want["ttc_egos"] = want["ttc"]                                        # (the layout changes no result)
    assert want["ttc"] != want["ttc_alone"] and want["episode"] != want["episode_alone"]
    for step, name in enumerate(("episode", "ttc", "ttc_alone", "episode", "ttc_egos", "episode_alone", "ttc", "episode")):
        got = _bytes(calls[name](hip_predictor))
        assert got == want[name], (step, name)


def _make(scene):
    sys.path.insert(0, ROOT)
    from bench import BRANCHING_WEIGHTS, WORKLOADS
    from mind_amd.closed_loop import ClosedLoopSim
    from mind_amd.planners.mind.planner import MINDPlanner
    from mind_amd.scene_io import ReplayWorld, scene_fixture_path
    cfg = os.path.join(ROOT, "mind_amd", "planners", "mind", "configs", "synthetic.json")
    wkw = dict(WORKLOADS[scene])
    w = ReplayWorld.from_scene_file(scene_fixture_path(wkw["scene"]))
    cfg = dict(json.load(open(cfg)), planning_config="planners.mind.configs.planning." + wkw["scene"], ckpt_path=BRANCHING_WEIGHTS)
    pl = MINDPlanner(cfg)
    pl.traj_tree_opt.speculative = False
    return pl, ClosedLoopSim(w, pl, native=None)


def test_closed_loop_auditor():
    pl, sim = _make("demo_2")
    assert sim._native is not None
    au = audit.EpisodeTtcAuditor(sim)
    while sim.n_plans < 10:
        au.step()
    S = len(au.times)
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_2")
    states = np.stack(au.states)
    # the defaults, under which no step of this stretch of demo_2 is within the horizon, and a longer look-ahead with a bar above its
    # least time: the same recorded run reported by a second auditor
    far = audit.EpisodeTtcAuditor(sim, horizon=8.0, bound=4.5)
    far.states, far.enabled, far.times = au.states, au.enabled, au.times
    for a, horizon, bound in ((au, tc.HORIZON, tc.BOUND), (far, 8.0, 4.5)):
        rep = a.report()
        assert len(rep["times"]) == S == sim.n_steps and rep["enabled"].sum() > 0 and not rep["enabled"][0]
        # before the take-over the ego is the recording: the recorded scene's values, by the host text
        nb = int((~rep["enabled"]).sum())
        assert rep["times"].tolist() == times[:S] and rep["before"]["steps"].tolist() == list(range(nb))
        rec = tc.host_ttc(ego[None, :nb], exo[:nb], valid[:nb], boxes, tc.EGO_BOX, horizon, bound)
        assert np.array_equal(rep["before"]["step_ttc"], rec["step_ttc"][0]) and np.array_equal(rep["before"]["step_track"], rec["step_track"][0])
        for k in tc.KEYS[2:]:
            assert rep["before"][k] == rec[k][0], k
        # the whole report: the recorded states through the host text
        assert np.array_equal(states[:nb], ego[:nb]) and not np.array_equal(states[nb + 5:], ego[nb + 5:S])
        want = tc.host_ttc(states[None], exo[:S], valid[:S], boxes, tc.EGO_BOX, horizon, bound)
        assert np.array_equal(rep["step_ttc"], want["step_ttc"][0]) and np.array_equal(rep["step_track"], want["step_track"][0])
        for k in tc.KEYS[2:]:
            assert rep[k] == want[k][0], k
        after = rep["after"]
        assert after["steps"][0] == nb and after["ego_min"] == rep["step_ttc"][nb:].min() and after["ego_hits"] == int((rep["step_ttc"][nb:] < bound).sum())
        print(f"demo_2, {S} steps, take-over at {nb}, horizon {horizon} s: {int(np.isfinite(rep['step_ttc']).sum())} steps within it; min ttc before "
              f"{rep['before']['ego_min']:.3f} s, after {after['ego_min']:.3f} s at step {after['ego_step']} (track {after['ego_track']}), {after['ego_hits']} steps below {bound} s")
    assert np.isfinite(rep["step_ttc"][:nb]).any() and np.isfinite(rep["step_ttc"][nb:]).any() and rep["before"]["ego_hits"] > 0


def test_error_codes(hip_predictor):
    hp = hip_predictor
    S, n = 4, 3
    box = _lib.AuditBox(4.5, 2.0, 0.0)
    eo = _lib.AuditTtcOut()
    st = np.full((1, S), -7.0)
    eo.step_ttc = st.ctypes.data_as(C.POINTER(C.c_double))
    ego, exo, valid, boxes = np.zeros((1, S, 4)), np.ones((S, n, 5)), np.ones((S, n), np.uint8), np.ones((n, 2))
    exo[:, :, 0] = 30.0
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    cfg_of = lambda h=3.0, b=0.95, l=0: _lib.AuditTtcCfg(h, b, l)

    def call(box=box, cfg=cfg_of(), n_ego=1, S=S, n=n, ego=ego, exo=exo, valid=valid, boxes=boxes, out=eo):
        rc = hp.lib.mind_audit_ttc(hp.ctx, C.byref(box) if box is not None else None, C.byref(cfg) if cfg is not None else None, n_ego, S, n, dp(ego), dp(exo),
                                   None if valid is None else valid.ctypes.data_as(C.POINTER(C.c_uint8)), dp(boxes), None if out is None else C.byref(out))
        return rc, (hp.lib.mind_last_error_string(hp.ctx) or b"").decode()
    nan_ego, nan_v, nan_exo, nan_vx, nan_vy, inv = ego.copy(), ego.copy(), exo.copy(), exo.copy(), exo.copy(), valid.copy()
    nan_ego[0, 2, 3], nan_v[0, 1, 2], nan_exo[1, 2, 0], nan_vx[1, 2, 3], nan_vy[1, 2, 4] = np.nan, np.inf, np.inf, np.nan, -np.inf
    for bad in (dict(box=None), dict(cfg=None), dict(out=None), dict(out=_lib.AuditTtcOut()), dict(n_ego=-1), dict(S=-1), dict(n=0), dict(ego=None), dict(exo=None),
                dict(valid=None), dict(boxes=None), dict(boxes=-boxes), dict(boxes=boxes * np.nan), dict(ego=nan_ego), dict(ego=nan_v), dict(exo=nan_exo),
                dict(exo=nan_vx), dict(exo=nan_vy), dict(box=_lib.AuditBox(4.5, -2.0, 0.0)), dict(box=_lib.AuditBox(4.5, 2.0, np.nan)), dict(n_ego=(1 << 22) // S + 1),
                dict(cfg=cfg_of(h=0.0)), dict(cfg=cfg_of(h=-1.0)), dict(cfg=cfg_of(h=np.nan)), dict(cfg=cfg_of(h=np.inf)), dict(cfg=cfg_of(b=-0.5)),
                dict(cfg=cfg_of(b=np.nan)), dict(cfg=cfg_of(b=np.inf)), dict(cfg=cfg_of(l=3)), dict(cfg=cfg_of(l=-1))):
        rc, msg = call(**bad)
        assert rc == _lib.MIND_EINVAL and msg.startswith("mind_audit_ttc"), (bad, rc, msg)
    assert np.all(st == -7.0)                                       # nothing was written
    inv[1, 2] = 0                                                   # an invalid row may hold anything
    for e in (nan_exo, nan_vx, nan_vy):
        assert call(exo=e, valid=inv)[0] == _lib.MIND_OK and np.all(st == np.inf)
    assert call(cfg=cfg_of(b=0.0))[0] == _lib.MIND_OK
    st[:] = -7.0
    assert call(n_ego=0)[0] == _lib.MIND_OK and call(S=0)[0] == _lib.MIND_OK and np.all(st == -7.0)          # successful no-ops
    with pytest.raises(ValueError, match="lanes"):
        hp.audit_ttc(ego, exo, valid, boxes, tc.EGO_BOX, lanes=4)
    # while a begun tree-iLQR call is pending: MIND_ESTATE, and that call then finishes with its usual result
    s = pr.scene("lead", 4)
    cfg_w, cfg_f = oi.default_cfg(max_iter=100), oi.default_cfg(max_iter=100)
    cfg_w.w_ego = cfg_w.w_exo = 0.0
    ref = hp.ilqr_contingency(cfg_w, cfg_f, [s["flat"]], s["x0"], s["lane"], s["tv"])
    pending = IlqrCall(hp.lib, cfg_w, [s["flat"]], s["x0"], s["lane"], s["tv"], cfg_full=cfg_f)
    pending.begin(hp)
    try:
        rc, msg = call()
        assert rc == _lib.MIND_ESTATE and "has not been finished" in msg and np.all(st == -7.0)
        with pytest.raises(_lib.MindError):
            hp.audit_ttc(ego, exo, valid, boxes, tc.EGO_BOX)
    finally:
        xs2, us2, sw, sf = pending.wait().finish()
    assert np.array_equal(xs2[0], ref[0][0]) and np.array_equal(us2[0], ref[1][0]) and sw == ref[2] and sf == ref[3]
    assert call()[0] == _lib.MIND_OK and np.all(st == np.inf)
