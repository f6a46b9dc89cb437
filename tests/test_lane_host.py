"""CPU: the lane geometry (mind_amd/csrc/lane_geom.h) through the library's host entry mind_debug_lane_project -- against its numpy
restatement bit for bit, against an independent vectorised witness (world coordinates, the projected point, argmin), closed forms, the edge
cases the header pins, the recorded AV on the four recorded maps -- the header alone under the address and undefined-behaviour sanitizers,
and the Python layer above it (audit.Lanes)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import audit_cases as ac
import lane_cases as lc
import lane_geom_restate as lr
from mind_amd import _lib, audit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (seed, lane sizes, origin): every decision of the 60 boxes of a case stays >= 1e-6 from its edge (asserted below)
SEEDED = [(1, (2,), (0.0, 0.0)), (2, (17,), (6500.0, 900.0)), (3, (40, 25), (-300.0, 1200.0)), (4, (9, 31, 14), (3000.0, 1500.0)),
          (7, (64, 65, 5), (7200.0, 250.0))]
BOX_OFF = (4.5, 2.0, 1.4)
PT = (0.0, 0.0)                     # a box of no size and no offset: the pose itself
DBL = ("lat", "s", "along", "across")
STRAIGHT = [(0.0, 0.0), (8.0, 0.0), (16.0, 0.0)]
ELL = [(0.0, 0.0), (8.0, 0.0), (8.0, 8.0)]


def _trig(b):
    with np.errstate(invalid="ignore"):
        return np.stack([np.cos(b[:, 2]), np.sin(b[:, 2])], 1)


def _proj(boxes, lanes, box=lc.EGO_BOX, cos_flow=lc.COS_FLOW, bound=lc.BOUND, trig=True):
    b = np.asarray(boxes, np.float64).reshape(-1, 3)
    if not isinstance(lanes, audit.Lanes):
        lanes = audit.Lanes.from_polylines(lanes)
    tg = None if trig is False else (_trig(b) if trig is True else trig)
    return _lib.lane_project(b, box, lanes.verts, lanes.lane_off, cos_flow, bound, tg)


def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=want[k].dtype == np.float64), (k, got[k], want[k])


@pytest.fixture(scope="module")
def seeded():
    out = []
    for seed, sizes, origin in SEEDED:
        lanes = lc.synth_lanes(seed, sizes, origin)
        out.append((lanes, lc.boxes_about(lanes, 60, seed + 100)))
    return out


def test_host_entry_is_the_restatement(seeded):
    """bit for bit, (cos, sin) from numpy handed to both; also with a box carried forward of its reference point, and with the restatement
    walking the segments backwards (the minimum over (d2, g) does not depend on the order)"""
    for lanes, b in seeded:
        for box in (lc.EGO_BOX, BOX_OFF):
            got = _proj(b, lanes, box)
            _same(got, lr.project(b, box, lanes.verts, lanes.lane_off, lc.COS_FLOW, lc.BOUND))
        _same(got, lr.project(b, box, lanes.verts, lanes.lane_off, lc.COS_FLOW, lc.BOUND, order=lambda n: range(n - 1, -1, -1)))
        hit = got["margin"] < 0
        assert hit.any() and (~hit).any() and (got["lane"][1] < 0).any() and (got["edge"][0] != got["edge"][1]).any()    # every branch is exercised
    d1 = lc.demo_lanes("demo_1")
    ego = ac.recorded_scene("demo_1")[2]
    b = ego[::25][:, [0, 1, 3]]
    got = _proj(b, d1)
    _same(got, lr.project(b, lc.EGO_BOX, d1.verts, d1.lane_off, lc.COS_FLOW, lc.BOUND))
    # the library's own sin / cos differs from numpy's by an ulp at most: the same decisions, the numbers to 1e-12
    own = _proj(b, d1, trig=False)
    assert all(np.array_equal(own[k], got[k]) for k in ("lane", "edge")) and all(np.abs(own[k] - got[k]).max() < 1e-12 for k in DBL + ("margin",))


def test_independent_witness(seeded):
    """Every double equals an independent evaluation to 1e-9, the road test's bar for the same kind of comparison: coordinates are <= 1e4 m,
    an ulp there is 1.8e-12 m, and the two formulations (offsets from the box centre against world coordinates; cross product over length
    against the projected point) differ by a few roundings of offsets.  First the cases keep every decision >= 1e-6 from its edge: the
    nearest segment against the next with another nearest point (segments meeting in the nearest vertex tie exactly; the header names the
    lower), every segment's cosine against the threshold, the winners' cross products against 0 (the sign of lat)."""
    for lanes, b in seeded:
        for box in (lc.EGO_BOX, BOX_OFF):
            wt = lr.witness(b, box, lanes.verts, lanes.lane_off, lc.COS_FLOW)
            assert wt["gap"] >= 1e-6, wt["gap"]
            got = _proj(b, lanes, box)
            for k in DBL:
                fin = np.isfinite(wt[k])
                assert np.array_equal(fin, np.isfinite(got[k])) and np.abs(got[k][fin] - wt[k][fin]).max() <= 1e-9, k
                assert np.array_equal(got[k][~fin], wt[k][~fin], equal_nan=True), k          # (+inf / NaN where there is no segment)
            assert np.array_equal(got["lane"], wt["lane"])
            for q in range(2):
                g = got["edge"][q] + lanes.lane_off[np.maximum(got["lane"][q], 0)]
                assert all((got["lane"][q, i] < 0 and not wt["segs"][q][i]) or g[i] == min(wt["segs"][q][i]) for i in range(len(b)))
            assert np.array_equal(got["margin"], lc.BOUND - np.abs(got["lat"][1]))


def test_closed_forms():
    """a straight lane along +x and an L-shaped one, segment lengths powers of two: every number is exact"""
    r = _proj([[5.0, 2.0, 0.0], [13.0, -1.5, 0.0]], [STRAIGHT])
    for q in range(2):
        assert r["lat"][q].tolist() == [2.0, -1.5] and r["s"][q].tolist() == [5.0, 13.0] and r["along"][q].tolist() == [1.0, 1.0]
        assert r["across"][q].tolist() == [0.0, 0.0] and r["lane"][q].tolist() == [0, 0] and r["edge"][q].tolist() == [0, 1]
    assert r["margin"].tolist() == [3.0, 3.5]
    # heading across the lane (cos, sin handed over exactly): the nearest segment of all is found, none goes the box's way
    r = _proj([[13.0, -1.5, 0.0]], [STRAIGHT], trig=np.array([[0.0, 1.0]]))
    assert (r["lat"][0, 0], r["s"][0, 0], r["along"][0, 0], r["across"][0, 0]) == (-1.5, 13.0, 0.0, 1.0)          # (pointing left of the lane)
    # the L: at (6, 3) the second leg, northbound, is nearer (2 m; the pose is to its west: left of travel) than the first (3 m)
    r = _proj([[6.0, 3.0, 0.0]], [ELL])
    assert (r["lat"][0, 0], r["s"][0, 0], r["along"][0, 0], r["across"][0, 0], r["edge"][0, 0]) == (2.0, 11.0, 0.0, -1.0, 1)
    assert (r["lat"][1, 0], r["s"][1, 0], r["along"][1, 0], r["across"][1, 0], r["edge"][1, 0]) == (3.0, 6.0, 1.0, 0.0, 0)     # heading east: the first leg
    assert r["margin"][0] == 2.0
    # the same lanes and poses rotated by 0.7 rad and carried thousands of metres away: to 1e-11 (an ulp of the coordinates is 9e-13)
    th, org = 0.7, np.array([6534.73, -3912.09])
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    far = _proj([np.concatenate([np.array([6.0, 3.0]) @ R.T + org, [th]])], [np.asarray(ELL) @ R.T + org])
    assert all(np.abs(far[k] - r[k]).max() <= 1e-11 for k in DBL) and np.array_equal(far["edge"], r["edge"])
    # a box carried 1.4 m forward of its reference point: the pose at the moved centre
    assert _proj([[3.6, 2.0, 0.0]], [STRAIGHT], BOX_OFF)["s"][0, 0] == 5.0


def test_edge_cases():
    p = lambda lanes, boxes, **kw: _proj(boxes, lanes, PT, **kw)
    # exactly on a segment: cr == 0, lat = +0.0
    r = p([STRAIGHT], [[4.0, 0.0, 0.0]])
    assert r["lat"][0, 0] == 0.0 and not np.signbit(r["lat"][0, 0]) and r["s"][0, 0] == 4.0 and r["margin"][0] == 5.0
    # before the first vertex: s = 0; beyond the last: s = the lane's length; the sign of lat is the side of the end segment's line
    r = p([STRAIGHT], [[-3.0, 1.0, 0.0], [-3.0, -1.0, 0.0], [19.0, 2.0, 0.0], [19.0, -2.0, 0.0]])
    assert r["s"][0].tolist() == [0.0, 0.0, 16.0, 16.0] and r["edge"][0].tolist() == [0, 0, 1, 1]
    assert np.array_equal(r["lat"][0], np.array([1.0, -1.0, 1.0, -1.0]) * np.sqrt([10.0, 10.0, 13.0, 13.0]))
    # two segments tie at their shared vertex: the lower one wins
    r = p([ELL], [[10.0, -2.0, 0.0]])
    assert (r["lat"][0, 0], r["s"][0, 0], r["edge"][0, 0], r["along"][0, 0]) == (-np.sqrt(8.0), 8.0, 0, 1.0)
    # ... also across lanes: two lanes on the same vertices, the lower lane is named
    r = p([ELL, ELL], [[10.0, -2.0, 0.0], [6.0, 3.0, 0.0]])
    assert r["lane"][0].tolist() == [0, 0] and r["edge"][0].tolist() == [0, 1]
    # a duplicated vertex is skipped: the same numbers, the edge indices moved by it, the arc length unchanged
    dup = [(0.0, 0.0), (8.0, 0.0), (8.0, 0.0), (8.0, 8.0), (8.0, 8.0)]
    pts = [[6.0, 3.0, 0.0], [10.0, -2.0, 0.0], [9.0, 9.0, 1.0], [3.0, -1.0, 0.0]]
    r, base = p([dup], pts), p([ELL], pts)
    assert all(np.array_equal(r[k], base[k]) for k in DBL + ("margin", "lane"))
    assert r["edge"][0].tolist() == [2, 0, 2, 0] and base["edge"][0].tolist() == [1, 0, 1, 0]
    # a lane of duplicated vertices only has no segment at all
    r = p([[(1.0, 1.0), (1.0, 1.0)]], [[0.0, 0.0, 0.0]])
    assert r["lat"][:, 0].tolist() == [np.inf, np.inf] and r["lane"][:, 0].tolist() == [-1, -1] and r["margin"][0] == -np.inf
    # the phantom segment: the line from lane 0's last vertex (8, 0) to lane 1's first (8, 8) passes through the pose (8, 3) -- the distance
    # is the real segments', 3 m to the end of lane 0
    r = p([[(0.0, 0.0), (8.0, 0.0)], [(8.0, 8.0), (16.0, 8.0)]], [[8.0, 3.0, 0.0], [8.0, 6.0, 0.0]])
    assert r["lat"][0].tolist() == [3.0, -2.0] and r["lane"][0].tolist() == [0, 1] and r["edge"][0].tolist() == [0, 0] and r["s"][0].tolist() == [8.0, 0.0]
    # along exactly equal to cos_flow counts: E = (3, 4), heading +x, the threshold 3.0 / 5.0; one ulp more and it does not
    lane34 = [[(0.0, 0.0), (3.0, 4.0)]]
    r = p(lane34, [[1.0, 0.0, 0.0]], cos_flow=3.0 / 5.0)
    assert r["along"][1, 0] == 3.0 / 5.0 and r["lane"][1, 0] == 0 and np.isfinite(r["margin"][0])
    r = p(lane34, [[1.0, 0.0, 0.0]], cos_flow=np.nextafter(3.0 / 5.0, 1.0))
    assert r["lane"][1, 0] == -1 and r["lane"][0, 0] == 0
    # no with-flow segment: +inf / -1 / NaN and a margin of -inf, while `any` is reported
    r = p([STRAIGHT], [[5.0, 2.0, np.pi]])
    assert r["lat"][1, 0] == np.inf and r["lane"][1, 0] == -1 and r["edge"][1, 0] == -1 and r["margin"][0] == -np.inf and r["margin"][0] < 0
    assert all(np.isnan(r[k][1, 0]) for k in ("s", "along", "across"))
    assert (r["lat"][0, 0], r["s"][0, 0], r["lane"][0, 0]) == (2.0, 5.0, 0) and abs(r["along"][0, 0] + 1.0) < 1e-15
    # cos_flow = -1 admits every segment: the two rows agree
    r = p([STRAIGHT], [[5.0, 2.0, 0.0]], cos_flow=-1.0, trig=np.array([[-1.0, 0.0]]))
    assert all(np.array_equal(r[k][0], r[k][1]) for k in lr.KEYS)
    # exactly at the bound: margin 0.0 and no hit; one ulp beyond: a hit
    r = p([STRAIGHT], [[5.0, 5.0, 0.0], [5.0, np.nextafter(5.0, 6.0), 0.0]])
    assert r["margin"][0] == 0.0 and not r["margin"][0] < 0 and r["margin"][1] < 0
    # a NaN pose: every double NaN, every index -1, the neighbours untouched
    r = _proj([[5.0, 2.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [13.0, -1.5, 0.0]], [STRAIGHT])
    assert all(np.isnan(r[k][:, 1:4]).all() for k in DBL) and np.isnan(r["margin"][1:4]).all()
    assert np.all(r["lane"][:, 1:4] == -1) and np.all(r["edge"][:, 1:4] == -1) and r["lat"][0, [0, 4]].tolist() == [2.0, -1.5]


@pytest.mark.parametrize("name", ["demo_1", "demo_2", "demo_3", "demo_4"])
def test_recorded_av_keeps_its_lane(name):
    """the recorded AV at every simulator step of the four scenes, against every semantic lane of the map (angle pi / 4, bound 5 m): no hit;
    and against its target lane: along the flow, and the progress the recording made.  The pinned figures are what the restatement gives
    (a subsample of it is compared bit for bit below); a prototype of the same rules gave the same to the digits shown."""
    w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
    lanes = lc.demo_lanes(name)
    assert (lanes.n_lanes, len(lanes.verts)) == {"demo_1": (21, 1395), "demo_2": (15, 747), "demo_3": (9, 288), "demo_4": (16, 999)}[name]
    assert lanes.n_lanes == len(w.smp.semantic_lanes) and np.array_equal(lanes.lane(1), np.asarray(w.smp.semantic_lanes[1], np.float64))
    b = ego[:, [0, 1, 3]]
    got = _proj(b, lanes, trig=False)
    assert len(ego) == 546 and not np.any(got["margin"] < 0.0) and np.all(np.isfinite(got["margin"])) and np.all(got["lane"] >= 0)
    worst = np.abs(got["lat"][1]).max()
    assert abs(worst - {"demo_1": 0.457, "demo_2": 1.391, "demo_3": 1.271, "demo_4": 0.883}[name]) < 0.006, worst
    sub = slice(3, None, 25)
    _same(_proj(b[sub], lanes), lr.project(b[sub], lc.EGO_BOX, lanes.verts, lanes.lane_off, lc.COS_FLOW, lc.BOUND))
    rest = lr.project(b[[int(np.argmax(np.abs(got["lat"][1])))]], lc.EGO_BOX, lanes.verts, lanes.lane_off, lc.COS_FLOW, lc.BOUND)
    assert abs(abs(rest["lat"][1, 0]) - worst) < 1e-12
    wt = lr.witness(b[::5], lc.EGO_BOX, lanes.verts, lanes.lane_off, lc.COS_FLOW)
    assert all(np.abs(wt[k] - got[k][:, ::5]).max() <= 1e-9 for k in ("lat", "s"))
    # the target lane
    tl = audit.Lanes.from_target_lane(w.target_lane)
    tg = _proj(b, tl, trig=False)
    assert tl.n_lanes == 1 and np.all(tg["lane"] == 0) and tg["along"][0].min() >= 0.93 and not np.any(tg["margin"] < 0)
    prog, back = lr.progress_ego(tg["lane"][0], tg["s"][0])
    assert (prog, back) == audit.lane_progress(tg["lane"][0], tg["s"][0])
    assert abs(prog - {"demo_1": 8.35, "demo_2": 34.08, "demo_3": 76.68, "demo_4": 50.74}[name]) < 0.01, prog
    if name in ("demo_1", "demo_2"):        # nearly at rest, the recorded trace steps backwards by less than a millimetre a step
        assert -0.01 < back <= 0.0, back
    else:
        assert back == 0.0
    print(name, "largest |lat| with the flow", worst, "at step", int(np.argmax(np.abs(got["lat"][1]))), "| target lane: least along", tg["along"][0].min(),
          "progress", prog, "back", back)


def test_arc_length_at_the_lanes_ends():
    """the arc length the library forms, seen through s beyond the lanes' far ends, is the sequential sum of the segment lengths: to 1e-11
    (the last segment's length comes from offsets, an ulp of these coordinates is 9e-13; bit for bit is the restatement's test above)"""
    lanes = lc.synth_lanes(9, (33, 7, 12), (6500.0, 900.0))
    cum = lr.cum_of(lanes.verts, lanes.lane_off)
    ends = lanes.lane_off[1:] - 1
    d = lanes.verts[ends] - lanes.verts[ends - 1]
    b = np.concatenate([lanes.verts[ends] + 0.5 * d, np.arctan2(d[:, 1], d[:, 0])[:, None]], 1)       # half a segment beyond every lane's end
    r = _proj(b, lanes, PT)
    assert np.abs(r["s"][0] - cum[ends]).max() <= 1e-11 and np.all(cum[ends] > 20.0) and r["lane"][0].tolist() == [0, 1, 2] and np.array_equal(r["edge"][0], np.diff(lanes.lane_off) - 2)


def test_header_alone_under_the_sanitizers(tmp_path, seeded):
    """lane_geom.h's whole walk in a stand-alone program with its own main, built by the host compiler with the address and
    undefined-behaviour sanitizers and run as a process of its own over the edge cases and a seeded family: no report, and the library's
    numbers bit for bit"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "lane_geom_walk")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "mind_amd", "csrc"), os.path.join(ROOT, "tests", "lane_geom_walk.cpp"), "-o", exe])
    dup = [(0.0, 0.0), (8.0, 0.0), (8.0, 0.0), (8.0, 8.0), (8.0, 8.0)]
    edge_b = np.array([[4.0, 0.0, 0.0], [-3.0, 1.0, 0.0], [19.0, -2.0, 0.0], [10.0, -2.0, 0.0], [6.0, 3.0, 0.0], [8.0, 3.0, 0.0], [5.0, 2.0, np.pi], [9.0, 9.0, 1.0]])
    cases = [(audit.Lanes.from_polylines(l), edge_b, cf) for l, cf in (([STRAIGHT], lc.COS_FLOW), ([ELL, dup], lc.COS_FLOW), ([[(1.0, 1.0), (1.0, 1.0)]], -1.0),
                                                                        ([[(0.0, 0.0), (8.0, 0.0)], [(8.0, 8.0), (16.0, 8.0)]], lc.COS_FLOW),
                                                                        ([[(0.0, 0.0), (3.0, 4.0)]], 3.0 / 5.0))]
    cases += [(seeded[3][0], seeded[3][1], lc.COS_FLOW), (seeded[0][0], seeded[0][1], lc.COS_FLOW)]
    hx = lambda v: " ".join(float(x).hex() for x in np.ravel(v))
    for lanes, b, cf in cases:
        tg = _trig(b)
        text = f"{lanes.n_lanes} {' '.join(map(str, lanes.lane_off.tolist()))}\n{hx(lanes.verts)}\n{hx([cf, lc.BOUND, 1.4])} {len(b)}\n"
        text += "\n".join(hx([b[i, 0], b[i, 1], tg[i, 0], tg[i, 1]]) for i in range(len(b))) + "\n"
        run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
        rows = [ln.split() for ln in run.stdout.splitlines()]
        assert len(rows) == len(b)
        want = _proj(b, lanes, BOX_OFF, cos_flow=cf)
        for i, r in enumerate(rows):
            f = [float.fromhex(x) if j not in (5, 6, 11, 12) else int(x) for j, x in enumerate(r)]
            mine = [want["margin"][i]] + [want[k][q, i] for q in range(2) for k in lr.KEYS]
            assert np.array_equal(np.array(f, np.float64), np.array(mine, np.float64), equal_nan=True), (i, f, mine)


def test_lanes_class():
    w = ac.recorded_scene("demo_3")[0]
    lanes = audit.Lanes.from_semantic_map(w.smp)
    assert lanes.verts.dtype == np.float64 and lanes.lane_off.dtype == np.int32 and lanes.lane_off[0] == 0 and lanes.lane_off[-1] == len(lanes.verts)
    assert all(np.array_equal(lanes.lane(i), np.asarray(w.smp.semantic_lanes[k], np.float64)) for i, k in enumerate(sorted(w.smp.semantic_lanes)))
    three = audit.Lanes.from_polylines([np.zeros((2, 3)) + [[0.0], [1.0]], STRAIGHT])            # (z is dropped)
    assert three.lane_off.tolist() == [0, 2, 5] and three.verts.shape == (5, 2)
    assert audit._lanes(w.smp).n_lanes == lanes.n_lanes and audit._lanes([STRAIGHT]).n_lanes == 1 and audit._lanes(lanes) is lanes
    for bad in (lambda: audit.Lanes(lanes.verts, [0, 1, len(lanes.verts)]), lambda: audit.Lanes(lanes.verts, [1, len(lanes.verts)]),
                lambda: audit.Lanes(lanes.verts, [0, 5]), lambda: audit.Lanes.from_polylines([]), lambda: audit.Lanes.from_polylines([np.zeros((3, 4))]),
                lambda: audit.Lanes([[0.0, np.nan], [1.0, 1.0]], [0, 2]), lambda: audit._cos_flow(-0.1), lambda: audit._cos_flow(4.0)):
        with pytest.raises(ValueError):
            bad()
    assert audit.DEFAULT_LANE_ANGLE == np.pi / 4.0 and audit.DEFAULT_LANE_BOUND == 5.0
    assert audit.lane_progress([0, 0, 1, 1, -1, -1, 1], [1.0, 3.0, 7.0, 6.5, np.nan, np.nan, 9.0]) == (1.5, -0.5)


def test_error_codes_of_the_host_entry():
    lib = _lib.load()
    lanes = audit.Lanes.from_polylines([STRAIGHT, ELL, [(0.0, 5.0), (9.0, 5.0)]])         # lane_off [0, 3, 6, 8]
    boxes = np.array([[5.0, 2.0, 0.0], [6.0, 3.0, 0.3]])
    lat, ln = np.full((2, 2), -7.0), np.full((2, 2), -7, np.int32)
    mg = np.full(2, -7.0)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    good = _lib.AuditLaneCfg(lc.COS_FLOW, 5.0, 0)

    def call(n=2, boxes=boxes, box=_lib.AuditBox(4.5, 2.0, 0.0), cfg=good, verts=lanes.verts, off=lanes.lane_off, P=3, lat=lat, lane=ln, margin=mg):
        off = None if off is None else np.ascontiguousarray(off, np.int32)
        return lib.mind_debug_lane_project(n, dp(boxes), None if box is None else C.byref(box), None if cfg is None else C.byref(cfg), dp(verts), ip(off), P,
                                           None, dp(lat), None, None, None, ip(lane), None, dp(margin))
    nan_v = lanes.verts.copy()
    nan_v[5, 1] = np.nan
    inf_v = lanes.verts.copy()
    inf_v[0, 0] = -np.inf
    cfg = lambda *a: _lib.AuditLaneCfg(*a)
    for bad in (dict(n=-1), dict(boxes=None), dict(box=None), dict(cfg=None), dict(verts=None), dict(off=None), dict(P=0), dict(P=-1), dict(P=(1 << 16) + 1),
                dict(lat=None, lane=None, margin=None), dict(box=_lib.AuditBox(-4.5, 2.0, 0.0)), dict(box=_lib.AuditBox(4.5, np.nan, 0.0)),
                dict(box=_lib.AuditBox(4.5, 2.0, np.inf)), dict(off=[1, 3, 6, 8]), dict(off=[0, 1, 6, 8]), dict(off=[0, 3, 3, 8]), dict(off=[0, 6, 3, 8]),
                dict(verts=nan_v), dict(verts=inf_v), dict(cfg=cfg(1.0000001, 5.0, 0)), dict(cfg=cfg(-1.5, 5.0, 0)),
                dict(cfg=cfg(np.nan, 5.0, 0)), dict(cfg=cfg(0.5, 0.0, 0)), dict(cfg=cfg(0.5, -1.0, 0)), dict(cfg=cfg(0.5, np.inf, 0)), dict(cfg=cfg(0.5, np.nan, 0)),
                dict(cfg=cfg(0.5, 5.0, 3)), dict(cfg=cfg(0.5, 5.0, -1))):
        assert call(**bad) == _lib.MIND_EINVAL, bad
    assert np.all(lat == -7.0) and np.all(ln == -7) and np.all(mg == -7.0)                  # nothing was written
    assert call(n=0) == _lib.MIND_OK and np.all(lat == -7.0)
    # (the C entries take V from lane_off's last entry, so "lane_off does not end at V" is the Python layer's to refuse: below)
    assert call(lane=None, margin=None) == _lib.MIND_OK and lat[:, 0].tolist() == [2.0, 2.0] and np.all(ln == -7) and np.all(mg == -7.0)
    assert call(P=1, off=[0, 3], lat=None, lane=None) == _lib.MIND_OK and mg[0] == 3.0
    assert call(cfg=cfg(-1.0, 5.0, 2), lat=None, margin=None) == _lib.MIND_OK and ln[:, 0].tolist() == [0, 0]
    # the Python binding raises on the same
    for bad in (lambda: _lib.lane_project(boxes, lc.EGO_BOX, lanes.verts, [0, 1, 6, 8], 0.5, 5.0), lambda: _lib.lane_project(boxes, lc.EGO_BOX, lanes.verts, [0, 3, 6, 7], 0.5, 5.0),
                lambda: _lib.lane_project(boxes, (4.5, -2.0), lanes.verts, lanes.lane_off, 0.5, 5.0), lambda: _lib.lane_project(boxes, lc.EGO_BOX, nan_v, lanes.lane_off, 0.5, 5.0),
                lambda: _lib.lane_project(boxes, lc.EGO_BOX, lanes.verts, lanes.lane_off, 1.5, 5.0), lambda: _lib.lane_project(boxes, lc.EGO_BOX, lanes.verts, lanes.lane_off, 0.5, 0.0),
                lambda: _lib.lane_project(boxes, lc.EGO_BOX, lanes.verts, lanes.lane_off, 0.5, 5.0, trig=np.ones((3, 2))), lambda: _lib.lane_cfg(0.5, 5.0, 3),
                lambda: _lib.lane_cfg(np.nan, 5.0), lambda: _lib.lane_cfg(0.5, np.inf)):
        with pytest.raises(ValueError):
            bad()
