"""What the feedback-policy calls cost against their nearest neighbours, in ONE process on one context, in interleaved blocks after a warm-up:

  (a) gains     one HipPredictor.ilqr_gains call (mind_ilqr_gains, k_ilqr_gains) on all cost trees of a plan
  (b) solve     one HipPredictor.ilqr_solve(max_iter = 1) from the same controls: the same derivative and backward work plus ten rollouts
  (c) rollouts  one HipPredictor.ilqr_policy_rollouts call (mind_ilqr_policy_rollouts, k_ilqr_policy) with C candidates
  (d) score     one HipPredictor.ilqr_score call with C candidate control trees (k_ilqr_score)

Cost trees: the five of planning cycle `--cycle` of the recorded demo_1 scene, as tools/ilqr_score_rate.py records them, or `--scripted`.
The controls are those of a six-iteration solve; the candidates of (c) are step sizes in [0, 1] with seeded start offsets, those of (d)
the controls plus seeded noise.  Checked on the way: the gains call's J is the solve's J_opt, and the rollout of step size 0 without an
offset is the scoring call's states for the nominal controls.

  python tools/ilqr_policy_rate.py [--cands 64] [--blocks 8] [--reps 20] [--scripted] [--out profiles/ilqr_policy.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ilqr_score_rate import recorded_plan, scripted_plan      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20, help="calls of each kind per block")
    ap.add_argument("--cycle", type=int, default=20)
    ap.add_argument("--scripted", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ilqr_policy.json"))
    args = ap.parse_args()
    rt, cfg, flats, x0, lane, tv = scripted_plan() if args.scripted else recorded_plan(args.cycle)
    Ms = [len(f["parent"]) for f in flats]
    cfg6, cfg1 = copy.copy(cfg), copy.copy(cfg)
    cfg6.max_iter, cfg1.max_iter = 6, 1
    us = rt.ilqr_solve(cfg6, flats, x0, lane, tv, 1)[1]
    rng = np.random.default_rng(0)
    C = args.cands
    alpha = rng.uniform(0.0, 1.0, size=C)
    dx0 = rng.normal(size=(C, 6)) * np.array([0.3, 0.3, 0.5, 0.02, 0.1, 0.01])
    alpha[0], dx0[0] = 0.0, 0.0
    cands = np.concatenate([u[None] + rng.normal(size=(C,) + u.shape) * np.array([0.5, 0.05]) for u in us], axis=1)
    cands[0] = np.concatenate(us)

    def gains():
        return rt.ilqr_gains(cfg1, flats, x0, lane, tv, 1, us, 1.0)

    def solve():
        return rt.ilqr_solve(cfg1, flats, x0, lane, tv, 1, us_init=us)

    g = gains()
    if np.any(g["bad_node"] >= 0):
        print("a Q_uu is singular at mu = 1:", g["bad_node"].tolist())
        return 1

    def rollouts():
        return rt.ilqr_policy_rollouts(cfg1, flats, x0, lane, tv, 1, us, g["k"], g["K"], alpha, dx0, want_xs=False, want_us=False, want_L=False)[3]

    def score():
        return rt.ilqr_score(cfg1, flats, x0, lane, tv, 1, cands, want_xs=False, want_L=False)[2]

    # warm-up of all four (first-use allocations, the library's staging) and the cross-checks
    st = solve()[2]
    Jc, Jd = rollouts(), score()
    xs0 = rt.ilqr_policy_rollouts(cfg1, flats, x0, lane, tv, 1, us, g["k"], g["K"], alpha[:1], dx0[:1])[0]
    sx0 = rt.ilqr_score(cfg1, flats, x0, lane, tv, 1, cands[:1])[0]
    same = bool(all(g["J"][t] == st[t]["J"] for t in range(len(flats))) and all(np.array_equal(a, b) for a, b in zip(xs0, sx0)))
    kinds = (("gains", gains), ("solve", solve), ("rollouts", rollouts), ("score", score))
    ms = {name: [] for name, _ in kinds}
    for b in range(args.blocks):
        for name, fn in kinds:
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            ms[name].append((time.perf_counter() - t0) / args.reps * 1e3)
    mean = {name: float(np.mean(v)) for name, v in ms.items()}
    out = {"trees": "scripted branch3 x 5" if args.scripted else f"demo_1, planning cycle {args.cycle}", "nodes": Ms, "agents": [int(f["mean"].shape[1]) for f in flats],
           "candidates": C, "blocks": args.blocks, "reps_per_block": args.reps, "cross_checks": same,
           "gains_ms": mean["gains"], "solve1_ms": mean["solve"], "rollouts_ms": mean["rollouts"], "score_ms": mean["score"],
           "gains_over_solve1": mean["gains"] / mean["solve"], "rollouts_over_score": mean["rollouts"] / mean["score"],
           "blocks_ms": {name: [float(v) for v in vals] for name, vals in ms.items()},
           "finite_J": bool(np.all(np.isfinite(Jc)) and np.all(np.isfinite(Jd)))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    rng_ = lambda v: f"{min(v):.3f} .. {max(v):.3f}"
    print(f"{len(flats)} trees of {Ms} nodes: gains {mean['gains']:.3f} ms (blocks {rng_(ms['gains'])}) against a one-iteration solve "
          f"{mean['solve']:.3f} ms ({rng_(ms['solve'])}); {C}-candidate rollouts {mean['rollouts']:.3f} ms ({rng_(ms['rollouts'])}) against a "
          f"{C}-candidate score {mean['score']:.3f} ms ({rng_(ms['score'])}); cross-checks: {same}")
    print(json.dumps({k: out[k] for k in ("gains_ms", "solve1_ms", "rollouts_ms", "score_ms", "gains_over_solve1", "rollouts_over_score", "cross_checks")}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
