"""CPU: the road geometry (mind_amd/csrc/road_geom.h) through the library's host entry mind_debug_road_margin -- against its numpy
restatement bit for bit, against an independent vectorised witness (world coordinates, projection form, matplotlib's point-in-polygon),
closed forms, the edge cases the header pins, the four recorded maps and the recorded AV on them -- and the Python layer above it
(av2_lite.StaticMap.drivable_areas, audit.Road)."""
import ctypes as C
import os

import numpy as np
import pytest

import audit_cases as ac
import road_cases as rc
import road_geom_restate as rr
from mind_amd import _lib, audit, av2_lite, scene_io

# (seed, ring sizes, origin): seeds chosen so that every decision of the 60 boxes of a case stays >= 1e-6 m from its edge (asserted below)
SEEDED = [(1, (3,), (0.0, 0.0)), (5, (17,), (6500.0, 900.0)), (3, (40, 25), (-300.0, 1200.0)), (4, (9, 31, 14), (3000.0, 1500.0)),
          (7, (64, 65), (7200.0, 250.0))]
BOX_OFF = (4.5, 2.0, 1.4)


def _trig(b):
    with np.errstate(invalid="ignore"):
        return np.stack([np.cos(b[:, 2]), np.sin(b[:, 2])], 1)


def _margin(boxes, road, box=rc.EGO_BOX, trig=True):
    b = np.asarray(boxes, np.float64).reshape(-1, 3)
    return _lib.road_margin(b, box, road.verts, road.poly_off, _trig(b) if trig else None)


@pytest.fixture(scope="module")
def seeded():
    out = []
    for seed, sizes, origin in SEEDED:
        road = rc.synth_road(seed, sizes, origin)
        out.append((road, rc.boxes_about(road, 60, seed + 100)))
    return out


def test_host_entry_is_the_restatement(seeded):
    """bit for bit, (cos, sin) from numpy handed to both; also with a box carried forward of its reference point"""
    on = 0
    for road, b in seeded:
        for box in (rc.EGO_BOX, BOX_OFF):
            got, want = _margin(b, road, box), rr.margins(b, box, road.verts, road.poly_off)
            for k in ("margin", "corner", "ring", "edge"):
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, box)
        on += int((got["margin"] >= 0).sum())
        assert 0 < (got["margin"] < 0).sum() < len(b)                # both sides of the boundary are exercised
    assert on >= 40
    d1 = rc.demo_road("demo_1")
    w, times, ego, exo, valid, boxes = ac.recorded_scene("demo_1")
    b = ego[::25][:, [0, 1, 3]]
    got, want = _margin(b, d1), rr.margins(b, rc.EGO_BOX, d1.verts, d1.poly_off)
    assert all(np.array_equal(got[k], want[k]) for k in got)
    # the library's own sin / cos differs from numpy's by an ulp at most: the same decisions, the margin to 1e-12
    own = _margin(b, d1, trig=False)
    assert np.abs(own["margin"] - got["margin"]).max() < 1e-12 and all(np.array_equal(own[k], got[k]) for k in ("corner", "ring", "edge"))


def test_independent_witness(seeded):
    """Inside / outside equals matplotlib's contains_points and the margin an independent evaluation to 1e-9 m.  The bound is derived:
    coordinates are <= 1e4 m, an ulp there is 1.8e-12 m, and the two formulations (offsets from the box centre against world coordinates;
    cross product over length against the projected point) differ by a few roundings of offsets -- three orders below the bound.  First
    the cases keep every decision >= 1e-6 m from its edge: the distance of every corner to every ring's boundary (so inside / outside
    and hit / no hit), the limiting corner against the second, the deciding ring against the next, the nearest edge against the next
    edge with another nearest point (two edges meeting in the nearest vertex tie exactly; the header names the lower)."""
    for road, b in seeded:
        for box in (rc.EGO_BOX, BOX_OFF):
            wt = rc.witness(b, road, box)
            assert wt["gap"] >= 1e-6, wt["gap"]
            got = _margin(b, road, box)
            assert np.array_equal(got["margin"] >= 0.0, wt["inside"].any(2).all(1))
            assert np.abs(got["margin"] - wt["margin"]).max() <= 1e-9
            assert np.array_equal(got["corner"], wt["corner"]) and np.array_equal(got["ring"], wt["ring"])
            assert all(got["edge"][i] == min(wt["edges"][i]) for i in range(len(b)))
    # per corner, through a box shrunk to a point (every corner is the centre)
    road, b = seeded[3]
    pt = _margin(b, road, (0.0, 0.0))
    from matplotlib.path import Path
    ins = np.stack([Path(np.concatenate([road.ring(r), road.ring(r)[:1]]), closed=True).contains_points(b[:, :2]) for r in range(road.n_rings)], 1)
    assert np.array_equal(pt["margin"] > 0.0, ins.any(1)) and np.all(pt["corner"] == 0)


def test_closed_forms():
    """the 40 x 8 m rectangle road, the 4.5 x 2 m box at yaw 0 and lateral offset y: margin = 4 - 1 - |y|, negative = the overhang"""
    road = audit.Road.from_polygons([rc.RECT])
    ys = np.array([0.0, 0.25, -0.25, 1.5, -2.75, 2.999, 3.5, -3.7, 4.9, -6.0])
    b = np.stack([np.linspace(-10.0, 10.0, len(ys)), ys, np.zeros(len(ys))], 1)
    got = _margin(b, road)
    assert np.abs(got["margin"] - (3.0 - np.abs(ys))).max() <= 1e-12
    assert np.array_equal(got["margin"] < 0, np.abs(ys) > 3.0) and np.all(got["ring"] == 0)
    assert np.array_equal(got["edge"], np.where(ys >= 0, 2, 0)) and np.array_equal(got["corner"], np.where(ys >= 0, 0, 1))
    # longitudinally: the nose over the end of the road by 0.75 m
    nose = _margin([[18.5, 0.0, 0.0]], road)
    assert abs(nose["margin"][0] + 0.75) <= 1e-12 and nose["edge"][0] == 1 and nose["corner"][0] == 0
    # the same road and boxes rotated by 0.7 rad and carried thousands of metres away
    th, org = 0.7, np.array([6534.73, -3912.09])
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    far = audit.Road.from_polygons([np.asarray(rc.RECT) @ R.T + org])
    bf = np.concatenate([b[:, :2] @ R.T + org, b[:, 2:] + th], 1)
    gf = _margin(bf, far)
    assert np.abs(gf["margin"] - (3.0 - np.abs(ys))).max() <= 1e-12
    # (the two corners of the limiting side tie at yaw 0 -- all four at y = 0 --, where the first is named; rotated, the last bit decides)
    k = ys != 0.0
    assert np.array_equal(gf["edge"][k], got["edge"][k]) and np.all(np.where(ys > 0, np.isin(gf["corner"], (0, 3)), np.isin(gf["corner"], (1, 2)))[k])
    # a box carried 1.4 m forward of its reference point: the box of offset 0 at the moved centre
    off = _margin([[17.1, 0.0, 0.0]], road, BOX_OFF)
    assert abs(off["margin"][0] + 0.75) <= 1e-12


def test_edge_cases():
    m = lambda road, boxes, box=(0.0, 0.0): _margin(boxes, road, box)          # (a box of no size: the point itself)
    # a triangle
    tri = audit.Road.from_polygons([[(0, 0), (4, 0), (0, 4)]])
    r = m(tri, [[1, 1, 0], [3, 3, 0], [-1, 2, 0]])
    assert np.allclose(r["margin"], [1.0, -np.sqrt(2.0), -1.0], atol=1e-15) and r["edge"].tolist() == [0, 1, 2]
    # an L: the notch is outside, the arms inside
    L = audit.Road.from_polygons([[(0, 0), (6, 0), (6, 2), (2, 2), (2, 6), (0, 6)]])
    r = m(L, [[4, 4, 0], [1, 5, 0], [5, 1, 0], [3, 3, 0]])
    assert np.allclose(r["margin"], [-2.0, 1.0, 1.0, -1.0], atol=1e-15) and r["edge"].tolist() == [2, 3, 0, 2]
    # a ray through a vertex: the diamond's left and right vertices lie on the +x ray of the points of the row y = 0
    dia = audit.Road.from_polygons([[(2, 0), (0, 2), (-2, 0), (0, -2)]])
    r = m(dia, [[-3, 0, 0], [0, 0, 0], [3, 0, 0], [-2.5, 0, 0], [1, 0, 0]])
    assert np.array_equal(r["margin"] > 0, [False, True, False, False, True])
    assert np.allclose(r["margin"], [-1.0, np.sqrt(2.0), -1.0, -0.5, np.sqrt(0.5)], atol=1e-15)
    # a ray along a horizontal edge: the points of the row y = 4 of the rectangle's top edge, and of the L's inner edge y = 2
    rect = audit.Road.from_polygons([rc.RECT])
    r = m(rect, [[-25, 4, 0], [25, 4, 0], [-25, -4, 0]])
    assert np.allclose(r["margin"], [-5.0, -5.0, -5.0], atol=1e-15)
    r = m(L, [[-1, 2, 0], [1, 2, 0], [7, 2, 0], [-1, 0, 0], [-1, 6, 0]])
    assert np.array_equal(r["margin"] > 0, [False, True, False, False, False]) and np.allclose(r["margin"], [-1, 1, -1, -1, -1], atol=1e-15)
    # a duplicated vertex (a zero-length edge) is skipped: the same margins and decisions, the edge indices moved by it
    dup = audit.Road(np.array([(0, 0), (6, 0), (6, 0), (6, 2), (2, 2), (2, 2), (2, 6), (0, 6)], np.float64), [0, 8])
    pts = [[4, 4, 0], [1, 5, 0], [5, 1, 0], [3, 3, 0], [6.5, -0.5, 0], [7, 0, 0]]
    r, base = m(dup, pts), m(L, pts)
    assert np.array_equal(r["margin"], base["margin"]) and r["edge"].tolist() == [3, 5, 0, 3, 0, 0] and base["edge"].tolist() == [2, 3, 0, 2, 0, 0]
    dup_last = audit.Road(np.array([(0, 0), (4, 0), (0, 4), (0, 4)], np.float64), [0, 4])
    assert np.array_equal(m(dup_last, [[1, 1, 0], [3, 3, 0], [-1, 2, 0]])["margin"], m(tri, [[1, 1, 0], [3, 3, 0], [-1, 2, 0]])["margin"])
    # a ring given with its closing vertex
    closed = audit.Road.from_polygons([rc.RECT + rc.RECT[:1]])
    assert closed.poly_off.tolist() == [0, 4] and np.array_equal(closed.verts, rect.verts)
    # two abutting rings: inside, the margin is the documented lower bound -- the shared edge x = 0 limits it, the truth is the union's
    two = audit.Road.from_polygons([[(-20, -4), (0, -4), (0, 4), (-20, 4)], [(0, -4), (20, -4), (20, 4), (0, 4)]])
    r = m(two, [[-0.5, 0, 0], [1.5, 1, 0], [-10, 0, 0]])
    truth = m(rect, [[-0.5, 0, 0], [1.5, 1, 0], [-10, 0, 0]])["margin"]
    assert np.all(r["margin"] > 0) and np.all(r["margin"] <= truth) and r["margin"].tolist() == [0.5, 1.5, 4.0] and truth.tolist() == [4.0, 3.0, 4.0]
    assert r["ring"].tolist() == [0, 1, 0]
    # two overlapping rings: the containing ring with the greatest distance decides, the lowest ring on a tie
    over = audit.Road.from_polygons([[(-20, -4), (5, -4), (5, 4), (-20, 4)], [(-5, -4), (20, -4), (20, 4), (-5, 4)]])
    r = m(over, [[2, 0, 0], [-2, 0, 0], [0, 0, 0]])
    assert r["margin"].tolist() == [4.0, 4.0, 4.0] and r["ring"].tolist() == [1, 0, 0]
    r = m(over, [[3, 3.5, 0], [-3, 3.5, 0]])
    assert r["margin"].tolist() == [0.5, 0.5] and r["ring"].tolist() == [0, 0]
    r = m(over, [[4.5, 0, 0], [-4.5, 0, 0]])
    assert r["margin"].tolist() == [4.0, 4.0] and r["ring"].tolist() == [1, 0]
    # two disjoint rings with a point between them: minus the distance to the nearer, the lower ring on a tie
    apart = audit.Road.from_polygons([[(-20, -4), (-2, -4), (-2, 4), (-20, 4)], [(3, -4), (20, -4), (20, 4), (3, 4)]])
    r = m(apart, [[0, 0, 0], [1, 0, 0], [0.5, 0, 0]])
    assert r["margin"].tolist() == [-2.0, -2.0, -2.5] and r["ring"].tolist() == [0, 1, 0] and r["edge"].tolist() == [1, 3, 1]
    # exactly touching: 0.0 and no hit -- the box's left corners on the top edge; the nose on the end of the road
    r = _margin([[0.0, 3.0, 0.0], [17.75, 0.0, 0.0], [0.0, -3.0, 0.0]], rect)
    assert np.all(r["margin"] == 0.0) and not np.any(r["margin"] < 0.0)
    # a NaN state
    r = _margin([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1, 1, 0]], rect)
    assert np.isnan(r["margin"][1:4]).all() and r["margin"][[0, 4]].tolist() == [3.0, 2.0]
    for k in ("corner", "ring", "edge"):
        assert r[k][1:4].tolist() == [-1, -1, -1] and r[k][0] >= 0
    # corners only: a verge under the middle of the box is not seen (documented, not solved)
    slit = audit.Road.from_polygons([[(-20, -4), (-0.1, -4), (-0.1, 4), (-20, 4)], [(0.1, -4), (20, -4), (20, 4), (0.1, 4)]])
    assert _margin([[0.0, 0.0, 0.0]], slit)["margin"][0] > 0


MAP_COUNTS = {"demo_1": (3, 326), "demo_2": (3, 236), "demo_3": (2, 144), "demo_4": (3, 385)}


@pytest.mark.parametrize("name", sorted(MAP_COUNTS))
def test_static_map_keeps_the_drivable_areas(name):
    path = rc.map_json(name)
    smap = av2_lite.StaticMap.from_json(path)
    areas = smap.drivable_areas
    assert (len(areas), sum(len(a) for a in areas)) == MAP_COUNTS[name]
    assert all(a.dtype == np.float64 and a.ndim == 2 and a.shape[1] == 2 and len(a) >= 3 and not np.array_equal(a[0], a[-1]) for a in areas)
    import json
    raw = json.load(open(path))["drivable_areas"]
    for a, d in zip(areas, raw.values()):                           # the file's order, the file's numbers
        assert np.array_equal(a, np.array([[p["x"], p["y"]] for p in d["area_boundary"]]))
    road = audit.Road.from_map_json(path)
    assert (road.n_rings, len(road.verts)) == MAP_COUNTS[name] and road.poly_off.dtype == np.int32 and road.verts.dtype == np.float64
    assert np.array_equal(road.verts, np.concatenate(areas)) and np.array_equal(audit.Road.from_static_map(smap).verts, road.verts)
    # everything from_json returned before is unchanged: the compact form equals the committed scene file's
    with np.load(scene_io.scene_fixture_path(name), allow_pickle=False) as z:
        fixture = av2_lite.StaticMap.from_arrays({k: z[k] for k in z.files if k.startswith("lane_")})
    a, b = smap.to_arrays(), fixture.to_arrays()
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a) and not any("driv" in k for k in a)
    # a map from a scene file has no drivable areas, and says where they are
    assert fixture.drivable_areas is None
    with pytest.raises(ValueError, match=r"log_map_archive_<seq_id>\.json"):
        audit.Road.from_static_map(fixture)


@pytest.mark.parametrize("name", sorted(MAP_COUNTS))
def test_recorded_av_stays_on_the_road(name):
    """the nominal box at the recorded AV's state: no hit at ANY simulator step of the four scenes; every corner in exactly one ring"""
    road = rc.demo_road(name)
    w, times, ego, exo, valid, boxes = ac.recorded_scene(name)
    got = _margin(ego[:, [0, 1, 3]], road, trig=False)
    assert len(ego) == 546 and not np.any(got["margin"] < 0.0) and np.all(np.isfinite(got["margin"]))
    lo = {"demo_1": 0.71, "demo_2": 2.15, "demo_3": 0.49, "demo_4": 0.43}[name]
    assert abs(got["margin"].min() - lo) < 0.006, got["margin"].min()
    wt = rc.witness(ego[::5][:, [0, 1, 3]], road)
    assert np.all(wt["inside"].sum(2) == 1) and np.abs(wt["margin"] - got["margin"][::5]).max() <= 1e-9
    print(name, "least margin of the recorded AV", got["margin"].min(), "at step", int(np.argmin(got["margin"])))


def test_error_codes_of_the_host_entry():
    lib = _lib.load()
    road = audit.Road.from_polygons([rc.RECT, [(30, 0), (40, 0), (35, 5)]])
    boxes = np.array([[0.0, 0.0, 0.0], [35.0, 1.0, 0.3]])
    mg, cn = np.full(2, -7.0), np.full(2, -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))

    def call(n=2, boxes=boxes, box=_lib.AuditBox(4.5, 2.0, 0.0), verts=road.verts, off=road.poly_off, P=2, margin=mg, corner=cn):
        off = None if off is None else np.ascontiguousarray(off, np.int32)
        return lib.mind_debug_road_margin(n, dp(boxes), None if box is None else C.byref(box), dp(verts), ip(off), P, None, dp(margin), ip(corner), None, None)
    nan_v = road.verts.copy()
    nan_v[5, 1] = np.nan
    inf_v = road.verts.copy()
    inf_v[0, 0] = np.inf
    for bad in (dict(n=-1), dict(boxes=None), dict(box=None), dict(verts=None), dict(off=None), dict(P=0), dict(P=-1), dict(margin=None, corner=None),
                dict(box=_lib.AuditBox(-4.5, 2.0, 0.0)), dict(box=_lib.AuditBox(4.5, np.nan, 0.0)), dict(box=_lib.AuditBox(4.5, 2.0, np.inf)),
                dict(off=[1, 4, 7]), dict(off=[0, 2, 7]), dict(off=[0, 5, 7]), dict(off=[0, 7, 4]), dict(off=[0, 4, 4]), dict(verts=nan_v), dict(verts=inf_v),
                dict(P=(1 << 16) + 1)):
        assert call(**bad) == _lib.MIND_EINVAL, bad
    assert np.all(mg == -7.0) and np.all(cn == -7)                  # nothing was written
    assert call(n=0) == _lib.MIND_OK and np.all(mg == -7.0)
    assert call(corner=None) == _lib.MIND_OK and mg.tolist() == [3.0, mg[1]] and mg[1] < 0 and np.all(cn == -7)
    assert call(P=1, off=[0, 4]) == _lib.MIND_OK and call(margin=None) == _lib.MIND_OK and cn[0] == 0
    # the Python binding raises on the same
    with pytest.raises(ValueError):
        _lib.road_margin(boxes, rc.EGO_BOX, road.verts, [0, 2, 7])
    with pytest.raises(ValueError):
        _lib.road_margin(boxes, (4.5, -2.0), road.verts, road.poly_off)
    with pytest.raises(ValueError):
        audit.Road(road.verts, [0, 2, 7])
    with pytest.raises(ValueError):
        audit.Road.from_polygons([])
