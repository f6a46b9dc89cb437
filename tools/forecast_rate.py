"""What scoring a forecast on the device costs, against the path it replaces: device events on the context's stream around each call, after
a warm-up call, median of `--reps`, the two paths alternating in one process:

  device   HipPredictor.forecast_score (mind_forecast_score: upload of gt / valid, k_forecast_modes, k_forecast_scenes, read-back of every output)
  numpy    reg.cpu() + cls.cpu() and the vectorised numpy evaluation of the same quantities (np.linalg.norm, masked means, np.argmin)

at A = 36 agents in one scene (the demo size) and A = 16 384 agents in 256 scenes of 64 (K = 6, T = 60, horizons 10 / 30 / 60).  The batches
are the seeded ones of tests/forecast_cases.py; the device's results must equal the host evaluation of the same header
(mind_debug_forecast_score) bit for bit.  `--once`: per size one warm-up and one device call, then two calls with the single horizon 1 --
the serial pass cut to one sample, staging and the per-sample phase unchanged -- and nothing else (for a kernel trace).

  python tools/forecast_rate.py [--reps 20] [--out profiles/forecast_rate.json] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HZ = (10, 30, 60)
CFG = dict(miss_radius=2.0, disc_scale=1.0, disc_offset=0.5)
BYTES_PER_AGENT = 7200 + 960 + 60          # reg + gt + valid at K = 6, T = 60: what k_forecast_modes must read
HBM_BPS = 6.3e12                           # the achievable HBM rate of an MI355X


def numpy_path(reg, cls, off, gt, valid):
    """the path this replaces: read the forecast back, then min-ADE / min-FDE / miss rate / coverage vectorised on the host"""
    r, c = reg.cpu().numpy().astype(np.float64), cls.cpu().numpy()
    d = np.linalg.norm(r[..., :2] - gt[:, None], axis=-1)
    inside = d <= CFG["disc_scale"] * np.maximum(r[..., 2], r[..., 3]) + CFG["disc_offset"]
    v = valid != 0
    out = {}
    for e in HZ:
        m = v[:, None, :e]
        n = np.maximum(m.sum(-1), 1)
        ade = np.where(m, d[:, :, :e], 0.0).sum(-1) / n
        last = e - 1 - np.argmax(v[:, e - 1::-1], axis=1)
        fde = np.take_along_axis(d, last[:, None, None], axis=2)[..., 0]
        cover = (inside[:, :, :e] & m).sum(-1)
        seg = np.add.reduceat(np.concatenate([ade, fde], 1), off[:-1], axis=0) / np.maximum(np.diff(off), 1)[:, None]
        kf = np.argmin(seg[:, 6:], axis=1)
        out[e] = (ade.min(1), fde.min(1), cover, seg, kf, np.add.reduceat((fde[np.arange(len(fde)), np.repeat(kf, np.diff(off))] > CFG["miss_radius"]).astype(np.int64), off[:-1]))
    return out, c


def timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), res


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forecast_rate.json"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    import forecast_cases as fc
    from mind_amd import _lib
    from mind_amd.runtime import get_runtime
    rt = get_runtime()
    out, same = {"reps": args.reps, "horizons": list(HZ)}, True
    for tag, sizes in (("demo_36", (36,)), ("round_16384", (64,) * 256)):
        b = fc.batch(6, 60, fc.SEED, sizes)
        A = int(b["actor_off"][-1])
        reg, cls = torch.from_numpy(b["reg"].copy()).to(rt.device), torch.from_numpy(b["cls"].copy()).to(rt.device)
        dev = lambda: rt.forecast_score(reg, cls, b["actor_off"], b["gt"], b["valid"], None, HZ, **CFG)
        host = lambda: numpy_path(reg, cls, b["actor_off"].astype(np.int64), b["gt"], b["valid"])
        res = dev()
        if args.once:
            dev()
            for _ in range(2):
                rt.forecast_score(reg, cls, b["actor_off"], b["gt"], b["valid"], None, (1,), **CFG)
            continue
        host()
        t_dev, t_np = [], []
        for _ in range(args.reps):
            t_dev.append(timed(dev, 1)[0])
            t_np.append(timed(host, 1)[0])
        want = _lib.forecast_score_host(b["reg"], b["cls"], b["actor_off"], b["gt"], b["valid"], None, HZ, **CFG)
        try:
            fc.same(res, want)
            ok = True
        except AssertionError:
            ok = False
        same = same and ok
        out[tag] = dict(agents=A, scenes=len(sizes), device=stats(t_dev), numpy=stats(t_np), same_as_host=ok,
                        read_bound_us=BYTES_PER_AGENT * A / HBM_BPS * 1e6, reg_bytes=int(b["reg"].nbytes))
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
