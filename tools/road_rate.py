"""What the road audit's device call costs, against the path it replaces: device events on the context's stream around each call, after a
warm-up call, median of `--reps`, the two paths alternating in one process:

  device   HipPredictor.audit_road_plan (mind_audit_road_plan: upload of road and states, k_road_boxes, k_audit_plan_trees, read-back of
           every output)
  numpy    the candidate states read back from the device (a torch tensor's .cpu()) and a vectorised numpy evaluation of the same margins
           (world coordinates, projection form, crossing parity; 4 096 boxes at a time)

at the demo size (ONE candidate state set on the scripted 70-node branch3 tree, a planner-size tree, against the demo_1 road, 326
vertices) and at 4 096 candidates on the same tree against the demo_4 road (385 vertices).  The states are those of a six-iteration solve,
turned and carried to the recorded AV's pose in the scene and shifted sideways by 2 mm per copy.  The device's results must equal the host
evaluation of the same header (mind_debug_road_margin + the rules of tests/road_geom_restate.py) bit for bit and the numpy path's margins
to 1e-9 m.  At the large size the numpy path takes seconds per call and is repeated `--numpy-reps` times only, without a warm-up.

The arithmetic bound of k_road_boxes: (corner, edge) pairs x OPS_PER_PAIR float64 operations / the float64 vector rate.  OPS_PER_PAIR = 24:
per pair 4 subtractions (a, b), 3 (cr), 4 (t), 3 + 3 (a.a, b.b), 2 (cr cr rl) = 19, and a quarter of the per-edge work the four corners
share (the vertex offset 4, E 2, ll 3, the division ~ 11) = 5; compares and selects are not counted.  None of them can fuse (the header
has no fma), so the rate is one operation per lane per clock: 256 CUs x 4 SIMDs x 16 float64 lanes x 2.4 GHz = 39.3e12 / s, half the
lane rate behind the FP32 vector peak of 157.3 TFLOPS (78.6e12 fused operations / s).

`--once`: per size one warm-up and one device call and nothing else (for a kernel trace).

  python tools/road_rate.py [--cands 4096] [--reps 20] [--numpy-reps 2] [--out profiles/road_rate.json] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OPS_PER_PAIR = 24
F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def numpy_margin(boxes, box, road, chunk=4096):
    """the path the call replaces: the box margins [n] of boxes [n, 3] = (x, y, yaw), vectorised in world coordinates"""
    L, W = box[0], box[1]
    loc = np.array([[L / 2, W / 2], [L / 2, -W / 2], [-L / 2, -W / 2], [-L / 2, W / 2]])
    out = np.zeros(len(boxes))
    rings = []
    for r in range(road.n_rings):
        A = road.ring(r)
        B = np.roll(A, -1, axis=0)
        keep = np.any(A != B, axis=1)
        A, B = A[keep], B[keep]
        E = B - A
        rings.append((A, B, E, np.einsum("ej,ej->e", E, E)))
    for i0 in range(0, len(boxes), chunk):
        b = boxes[i0:i0 + chunk]
        c, s = np.cos(b[:, 2]), np.sin(b[:, 2])
        px = (b[:, None, 0] + c[:, None] * loc[None, :, 0] - s[:, None] * loc[None, :, 1]).reshape(-1, 1)
        py = (b[:, None, 1] + s[:, None] * loc[None, :, 0] + c[:, None] * loc[None, :, 1]).reshape(-1, 1)
        best_in, best_out, any_in = np.full(len(px), -np.inf), np.full(len(px), np.inf), np.zeros(len(px), bool)
        for A, B, E, ll in rings:
            ax, ay = A[None, :, 0] - px, A[None, :, 1] - py
            t = np.clip(-(ax * E[None, :, 0] + ay * E[None, :, 1]) / ll[None], 0.0, 1.0)
            qx, qy = ax + t * E[None, :, 0], ay + t * E[None, :, 1]
            d = np.sqrt((qx * qx + qy * qy).min(axis=1))
            by = B[None, :, 1] - py
            cross = ((ay > 0) != (by > 0)) & ((ax * by - ay * (B[None, :, 0] - px) > 0) == (by > ay))
            inside = cross.sum(axis=1) % 2 == 1
            best_in = np.where(inside, np.maximum(best_in, d), best_in)
            best_out = np.minimum(best_out, d)
            any_in |= inside
        out[i0:i0 + chunk] = np.where(any_in, best_in, -best_out).reshape(-1, 4).min(axis=1)
    return out


def timed(fn, reps, warm=True):
    """median / min / max ms of fn() between two events on the current stream (the context's), after one warm-up call"""
    import torch
    if warm:
        fn()
    ms, res = [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, res


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "road_rate.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    import audit_cases as ac
    import road_cases as rc
    from mind_amd.runtime import get_runtime
    from mind_amd.synth import scripted_scenario_tree
    from oracle import ilqr as oi
    rt = get_runtime()
    sst = scripted_scenario_tree("branch3", 12)
    flat = oi.flatten(sst["nodes"])
    xs0 = rt.ilqr_solve(oi.default_cfg(max_iter=6), [flat], oi.init_state(sst["state"], sst["ctrl"]), sst["target_lane"], sst["target_vel"], 1)[0][0]
    M = len(flat["parent"])
    out, same = {"reps": args.reps, "ops_per_pair": OPS_PER_PAIR, "f64_ops_per_s": F64_OPS_PER_S}, True
    for name, scene, n_cand in (("demo", "demo_1", 1), ("large", "demo_4", args.cands)):
        road = rc.demo_road(scene)
        av = ac.recorded_scene(scene)[2][0]                         # the recorded AV at step 0: (x, y, v, yaw)
        c, s = np.cos(av[3]), np.sin(av[3])
        xs = np.stack([xs0] * n_cand)
        dx, dy = xs0[:, 0] - xs0[0, 0], xs0[:, 1] - xs0[0, 1] + 0.002 * np.arange(n_cand)[:, None]
        xs[:, :, 0], xs[:, :, 1], xs[:, :, 3] = av[0] + c * dx - s * dy, av[1] + s * dx + c * dy, xs0[:, 3] + av[3]
        dev_call = lambda: rt.audit_road_plan([flat], [xs], road.verts, road.poly_off, rc.EGO_BOX)
        if args.once:
            dev_call()
            dev_call()
            continue
        xs_dev = torch.from_numpy(xs).cuda()
        np_call = lambda: numpy_margin(xs_dev.cpu().numpy().reshape(-1, 6)[:, [0, 1, 3]], rc.EGO_BOX, road)
        n_np = args.reps if n_cand == 1 else min(args.reps, args.numpy_reps)
        dev_call()
        if n_cand == 1:
            np_call()
        dev_ms, np_ms, res, ref = [], [], None, None
        for i in range(args.reps):                                  # alternating
            m, res = timed(dev_call, 1, warm=False)
            dev_ms += m
            if i < n_np:
                m, ref = timed(np_call, 1, warm=False)
                np_ms += m
        k = min(n_cand, 8)
        want = rc.host_plan([flat], [xs[:k]], road)
        ok = all(np.array_equal(res[q][0][:k], want[q][0]) for q in rc.PLAN_KEYS) and all(np.array_equal(res[q][:k], want[q]) for q in rc.TREE_KEYS)
        err = float(np.abs(res["node_margin"][0].ravel() - ref).max())
        same = same and ok and err <= 1e-9
        pairs = n_cand * M * 4 * len(road.verts)
        out[name] = dict(device=stats(dev_ms), numpy=stats(np_ms), candidates=n_cand, nodes=M, boxes=n_cand * M, road=scene, rings=road.n_rings,
                         vertices=len(road.verts), corner_edge_pairs=pairs, arithmetic_bound_ms=pairs * OPS_PER_PAIR / F64_OPS_PER_S * 1e3,
                         nodes_off_the_road=int((res["node_margin"][0] < 0).sum()), same_as_host=bool(ok), numpy_max_abs_diff_m=err)
    if args.once:
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
