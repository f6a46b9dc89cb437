"""CPU: the observation windows of mind_planner_* (include/mind_hip.h) against MINDPlanner.update_observation.

mind_planner_observe / _reset / _export touch no device, so a planner created with a NULL context keeps windows on a machine without a GPU.
A scripted sequence of frames -- tracks that appear late, vanish for a few frames and return, vanish for good, more than 50 frames, a
reset in the middle -- must leave the library with the windows `MINDPlanner.update_observation` keeps in `agent_obs[...]._arr` for the
same frames: value for value, in the same track order."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from mind_amd import _lib
from mind_amd.planners.mind.planner import MINDPlanner
from mind_amd.planners.mind.utils import _TYPE_SLOT, _name

TYPES = ["vehicle", "pedestrian", "bus", "cyclist", "something_else"]


def _null_planner(lib, ego_type="vehicle"):
    cw, cf = _lib.IlqrCfg(), _lib.IlqrCfg()
    d = _lib.PlannerDesc()
    d.time_ahead, d.min_vel, d.dist_thres, d.max_depth, d.max_rounds, d.pred_len, d.prob_floor = 3.0, 0.5, 2.0, 5, 16, 60, 0.0
    d.cfg_warm, d.cfg_full, d.speculative, d.ego_type_slot = C.addressof(cw), C.addressof(cf), 0, _TYPE_SLOT.get(_name(ego_type), 6)
    h = C.c_void_p()
    assert lib.mind_planner_create(None, C.byref(d), C.byref(h)) == 0
    return h


def _python_planner():
    pl = object.__new__(MINDPlanner)
    pl.agent_obs, pl.obs_len = {}, 50
    return pl


def _frames(n_frames, seed):
    """frame f -> (ego state, [(id, type, state)]): a scripted cast.  "late" appears at frame 7, "blink" vanishes for frames 12..15 and
    returns, "gone" vanishes for good after frame 20, "steady" is always there, "late2" appears at frame 60 (after the windows have slid),
    and the order in which a frame lists its agents changes from frame to frame"""
    rng = np.random.default_rng(seed)
    cast = {"steady": 0, "blink": 1, "gone": 2, "late": 3, "late2": 4, 1007: 0}

    def there(name, f):
        return {"steady": True, "blink": not (12 <= f <= 15), "gone": f <= 20, "late": f >= 7, "late2": f >= 60, 1007: f % 9 != 4}[name]

    out = []
    for f in range(n_frames):
        ego = rng.normal(size=4) * (10.0, 10.0, 3.0, 1.0)
        exo = [(name, TYPES[t], rng.normal(size=4) * (30.0, 30.0, 4.0, 2.0)) for name, t in cast.items() if there(name, f)]
        if f % 2:
            exo.reverse()
        if f % 5 == 3:
            exo = exo[1:] + exo[:1]
        out.append((ego, exo))
    return out


def _lcl(frame, f):
    ego, exo = frame
    return SimpleNamespace(ego_agent=SimpleNamespace(state=ego, type="vehicle", id="AV", timestep=f),
                           exo_agents=[SimpleNamespace(state=s, type=t, id=i, timestep=f) for i, t, s in exo])


def _push(lib, h, pl, lcl, keys, ids):
    """the frame through mind_planner_observe, marshalled with the planner's own to_object_state"""
    row = lambda a: (lambda o: (o.position[0], o.position[1], o.heading, o.velocity[0], o.velocity[1]))(pl.to_object_state(a))
    ego = np.array(row(lcl.ego_agent), np.float64)
    k, s, r = [], [], []
    for a in lcl.exo_agents:
        if a.id not in keys:
            keys[a.id] = 1000 + 17 * len(ids)         # (any integers: the caller chooses)
            ids[keys[a.id]] = a.id
        k.append(keys[a.id]); s.append(_TYPE_SLOT.get(_name(a.type), 6)); r.append(row(a))
    n = len(k)
    ka, sa, ra = np.array(k, np.int64), np.array(s, np.int32), np.array(r, np.float64).reshape(n, 5)
    return lib.mind_planner_observe(h, lcl.ego_agent.timestep, ego.ctypes.data, n, ka.ctypes.data, sa.ctypes.data, ra.ctypes.data)


def _export(lib, h, cap=16):
    n = C.c_int(0)
    key, count, rows = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros((cap, 50, 7))
    assert lib.mind_planner_export(h, cap, C.byref(n), key.ctypes.data, count.ctypes.data, rows.ctypes.data) == 0
    return [(int(key[s]), rows[s, :count[s]].copy()) for s in range(n.value)]


def _assert_same_windows(lib, h, pl, ids, where):
    got = _export(lib, h)
    want = list(pl.agent_obs.items())
    assert [("AV" if k == _lib.PLANNER_EGO_KEY else ids[k]) for k, _ in got] == [tid for tid, _ in want], where
    for (k, rows), (tid, tr) in zip(got, want):
        assert rows.shape[0] == len(tr.object_states) == len(tr._arr), (where, tid)
        assert np.array_equal(rows[:, :6], tr._arr), (where, tid)
        assert [int(t) for t in rows[:, 6]] == [s.timestep for s in tr.object_states], (where, tid)
        assert [bool(o) for o in rows[:, 0]] == [s.observed for s in tr.object_states], (where, tid)


def test_windows_equal_update_observation():
    lib = _lib.load()
    h, pl = _null_planner(lib), _python_planner()
    keys, ids = {}, {}
    try:
        assert _export(lib, h) == []                       # no frame yet: no track, not even the ego's
        frames = _frames(75, seed=3)
        for f, frame in enumerate(frames):
            lcl = _lcl(frame, f)
            pl.update_observation(lcl)
            assert _push(lib, h, pl, lcl, keys, ids) == 0
            if f in (0, 6, 7, 11, 13, 16, 21, 30, 49, 50, 51, 60, 74):
                _assert_same_windows(lib, h, pl, ids, f)
        assert max(len(rows) for _, rows in _export(lib, h)) == 50 and len(_export(lib, h)) == 7
        # a reset in the middle (ClosedLoopSim._start_episode clears agent_obs): the next episode's tracks join in ITS order
        assert lib.mind_planner_reset(h) == 0
        pl.agent_obs.clear()
        assert _export(lib, h) == []
        for f, frame in enumerate(_frames(58, seed=4)[5:]):
            lcl = _lcl(frame, f)
            pl.update_observation(lcl)
            assert _push(lib, h, pl, lcl, keys, ids) == 0
        _assert_same_windows(lib, h, pl, ids, "after the reset")
    finally:
        lib.mind_planner_destroy(h)


def test_exported_windows_rebuild_agent_obs():
    """the hand-back path (NativePlan.export_windows / NativeLoop.hand_back) without a device: the library's exported windows, rebuilt into
    an empty planner's agent_obs by native_cycle.rebuild_agent_obs, are the Tracks update_observation holds for the same frames -- and
    stay so when both planners carry on in Python across the array mirror's compaction (a wrong _i / _n / _buf shows there)"""
    from mind_amd.native_cycle import rebuild_agent_obs
    from mind_amd.planners.mind.planner import TrackCategory
    lib = _lib.load()
    h, pl, rebuilt = _null_planner(lib), _python_planner(), _python_planner()
    keys, ids, types = {}, {}, {}
    try:
        frames = _frames(75, seed=3)
        for f, frame in enumerate(frames):
            lcl = _lcl(frame, f)
            types.update((a.id, a.type) for a in lcl.exo_agents)
            pl.update_observation(lcl)
            assert _push(lib, h, pl, lcl, keys, ids) == 0
        cap, n = 16, C.c_int(0)
        key, count, rows = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros((cap, 50, 7))
        assert lib.mind_planner_export(h, cap, C.byref(n), key.ctypes.data, count.ctypes.data, rows.ctypes.data) == 0
    finally:
        lib.mind_planner_destroy(h)
    rebuild_agent_obs(rebuilt, n.value, key, count, rows, lambda k: ("AV", "vehicle", TrackCategory.FOCAL_TRACK) if k == _lib.PLANNER_EGO_KEY else
                      (ids[k], types[ids[k]], TrackCategory.TRACK_FRAGMENT))

    def assert_same(where):
        assert list(rebuilt.agent_obs) == list(pl.agent_obs) and len(pl.agent_obs) == 7, where
        for tid, want in pl.agent_obs.items():
            got = rebuilt.agent_obs[tid]
            assert got.track_id == want.track_id == tid and got.object_type == want.object_type and got.category == want.category, (where, tid)
            assert len(got.object_states) == len(want.object_states), (where, tid)
            for a, b in zip(got.object_states, want.object_states):
                assert (a.observed, a.timestep, tuple(a.position), a.heading, tuple(a.velocity)) == \
                       (b.observed, b.timestep, tuple(b.position), b.heading, tuple(b.velocity)), (where, tid)
                assert type(a.observed) is bool and type(a.timestep) is int, (where, tid)
            assert got._arr.shape == want._arr.shape and np.array_equal(got._arr, want._arr), (where, tid)

    assert_same("rebuilt")
    assert max(len(t.object_states) for t in pl.agent_obs.values()) == 50
    compacted = {id(p): set() for p in (pl, rebuilt)}
    for f, frame in enumerate(_frames(170, seed=7)):
        lcl = _lcl(frame, 75 + f)
        for p in (pl, rebuilt):
            before = {tid: t._i for tid, t in p.agent_obs.items()}
            p.update_observation(lcl)
            compacted[id(p)].update(tid for tid, i in before.items() if p.agent_obs[tid]._i <= i)
        assert_same(75 + f)
    # both planners' mirrors were compacted on the way (at 4 * obs_len appends, so at different frames for the two); "late2", 15 frames old
    # at the export, does not get there in either
    assert all(c == set(pl.agent_obs) - {"late2"} for c in compacted.values()), compacted


def test_float32_states_are_the_callers_business():
    """a float32 recording: the caller's to_object_state evaluates numpy's float32 cosine; the library stores what it is given"""
    lib = _lib.load()
    h, pl = _null_planner(lib), _python_planner()
    keys, ids = {}, {}
    try:
        for f, (ego, exo) in enumerate(_frames(20, seed=5)):
            lcl = _lcl((ego.astype(np.float32), [(i, t, s.astype(np.float32)) for i, t, s in exo]), f)
            pl.update_observation(lcl)
            assert _push(lib, h, pl, lcl, keys, ids) == 0
        _assert_same_windows(lib, h, pl, ids, "float32")
    finally:
        lib.mind_planner_destroy(h)


def test_argument_errors():
    lib = _lib.load()
    E, S = _lib.MIND_EINVAL, _lib.MIND_ESTATE
    h = C.c_void_p()
    assert lib.mind_planner_create(None, None, C.byref(h)) == E
    d = _lib.PlannerDesc()
    assert lib.mind_planner_create(None, C.byref(d), C.byref(h)) == E          # no solver configuration, no rounds
    h = _null_planner(lib)
    try:
        ego, k, s, r = np.zeros(5), np.array([5, 6], np.int64), np.zeros(2, np.int32), np.zeros((2, 5))
        obs = lambda *a: lib.mind_planner_observe(*a)
        assert obs(None, 0, ego.ctypes.data, 0, None, None, None) == E
        assert obs(h, 0, None, 0, None, None, None) == E
        assert obs(h, 0, ego.ctypes.data, -1, k.ctypes.data, s.ctypes.data, r.ctypes.data) == E
        assert obs(h, 0, ego.ctypes.data, 2, None, s.ctypes.data, r.ctypes.data) == E
        assert obs(h, 0, ego.ctypes.data, 2, k.ctypes.data, None, r.ctypes.data) == E
        assert obs(h, 0, ego.ctypes.data, 2, k.ctypes.data, s.ctypes.data, None) == E
        dup = np.array([5, 5], np.int64)
        assert obs(h, 0, ego.ctypes.data, 2, dup.ctypes.data, s.ctypes.data, r.ctypes.data) == E
        own = np.array([5, _lib.PLANNER_EGO_KEY], np.int64)
        assert obs(h, 0, ego.ctypes.data, 2, own.ctypes.data, s.ctypes.data, r.ctypes.data) == E
        bad_slot = np.array([0, 7], np.int32)
        assert obs(h, 0, ego.ctypes.data, 2, k.ctypes.data, bad_slot.ctypes.data, r.ctypes.data) == E
        assert _export(lib, h) == []                       # a refused frame changes nothing
        assert obs(h, 0, ego.ctypes.data, 2, k.ctypes.data, s.ctypes.data, r.ctypes.data) == 0
        assert obs(h, 1, ego.ctypes.data, 0, None, None, None) == 0           # an empty frame is a frame
        assert [len(rows) for _, rows in _export(lib, h)] == [2, 2, 2]
        n = C.c_int(0)
        assert lib.mind_planner_export(h, 2, C.byref(n), k.ctypes.data, s.ctypes.data, r.ctypes.data) == E and n.value == 3      # cap too small
        assert lib.mind_planner_export(h, 4, None, None, None, None) == E
        assert lib.mind_planner_reset(None) == E
        # every call that needs the device: MIND_ESTATE on a planner without a context
        out = _lib.PlannerOut()
        st, ct = np.zeros(4), np.zeros(2)
        assert lib.mind_planner_plan(h, st.ctypes.data, ct.ctypes.data, C.byref(out)) == S
        assert lib.mind_planner_plan(h, None, ct.ctypes.data, C.byref(out)) == E
        lane = np.zeros((12, 2))
        assert lib.mind_planner_set_lanes(h, 1, np.zeros((1, 11, 2)).ctypes.data, np.zeros((1, 6), np.int32).ctypes.data) == S
        assert lib.mind_planner_set_target_lane(h, 12, lane.astype(np.float32).ctypes.data, np.zeros((12, 12), np.float32).ctypes.data) == S
        assert lib.mind_planner_set_solve_lane(h, 12, lane.ctypes.data, 5.0) == S
        assert lib.mind_planner_set_eval_lane(h, 12, lane.ctypes.data, 0) == S
        po, ptr = _lib.AimePlanOut(), [C.c_void_p() for _ in range(6)]
        assert lib.mind_planner_last_plan(h, C.byref(po), *[C.byref(p) for p in ptr], None) == S
        # ... and the windows are still there
        assert [len(rows) for _, rows in _export(lib, h)] == [2, 2, 2]
    finally:
        assert lib.mind_planner_destroy(h) == 0


def test_native_plan_is_off_by_default():
    assert MINDPlanner.native_plan_default is False


def test_dropin_install_switches_it_on_for_the_planners_it_aliases():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import mind_amd.dropin as d\n"
            "d.install()\n"
            "from planners.mind.planner import MINDPlanner\n"
            "assert MINDPlanner.native_plan_default is False\n"
            "d.install(native_plan=True)\n"
            "from planners.mind.planner import MINDPlanner as M2\n"
            "assert M2.native_plan_default is True\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=root))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
