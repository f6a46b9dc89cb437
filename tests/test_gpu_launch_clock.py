"""The launch clock (mind_amd/csrc/launch_clock.h; mind_set_tuning "prof_clock") on the GPU, at the smallest shapes that exercise the pair
kernels' job walk: one scene of 3 agents + 13 lanes (N = 17: two tiles per column, the last one partly filled) and two scenes of unequal size
(2 + 5 and 4 + 20) under the seed-7 pseudo-random weights.

  bits    cls, reg, vel and the edge tensor of every launchable pair family (and of k_actor_mfma<6>, the ActorNet of the default arithmetic) are
          bitwise equal with profiling off, with HIP events ("prof_clock" 0), with the clock (1) and with both (2)
  timing  both mechanisms on the same launches ("prof_clock" 2): for every launch 0 < clock <= event -- the clock runs from the first workgroup in
          to the last workgroup out, the events also hold the dispatch on either side.  Median and largest event - clock are printed and written
          to profiles/launch_clock_vs_events.txt: the size of the definition shift, not asserted beyond the inequality
  loop    twelve cycles of the native loop across an episode restart give identical plans and controls under "prof_clock" 0 and 1, the same
          pair_launches and ilqr_launches in mind_loop_totals, and a positive pair_ms"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mind_amd.synth import predictor_batch
from oracle import predictor as op

pytestmark = pytest.mark.gpu

# (arithmetic, pair_tile): k_pair | k_pair_bf<3>, k_pair_t<3> | k_pair_bf<1>, k_pair_t<1> | k_pair_t6 (with k_actor_mfma<6>)
FORMS = {"f32": ("f32", 1), "bf16x3-tile0": ("bf16x3", 0), "bf16x3-tile1": ("bf16x3", 1), "bf16-tile0": ("bf16", 0), "bf16-tile1": ("bf16", 1),
         "bf16x6": ("bf16x6", 1)}
SHAPES = ["one-3-13", "two-2-5-4-20"]
SHIFTS = []           # (form, shape, kind, clock ms, event ms) of every launch the timing test saw


@functools.lru_cache(maxsize=None)
def _batch(shape):
    if shape.startswith("one"):
        pb = predictor_batch(3, 13, 1, seed=5)
    else:
        s, b = predictor_batch(2, 5, 1, seed=6), predictor_batch(4, 20, 1, seed=7)
        pb = {"ACTORS": np.concatenate([s["ACTORS"], b["ACTORS"]]), "LANES": np.concatenate([s["LANES"], b["LANES"]]),
              "ACTOR_IDCS": [np.arange(2), np.arange(2, 6)], "LANE_IDCS": [np.arange(5), np.arange(5, 25)],
              "CTRS": s["CTRS"] + b["CTRS"], "VECS": s["VECS"] + b["VECS"],
              "TGT_NODES": np.concatenate([s["TGT_NODES"], b["TGT_NODES"]]), "TGT_RPE": np.concatenate([s["TGT_RPE"], b["TGT_RPE"]])}
    pb["RPE"] = [op.rpe(torch.from_numpy(c), torch.from_numpy(v)).numpy() for c, v in zip(pb["CTRS"], pb["VECS"])]
    return pb


@pytest.fixture(scope="module")
def clock_predictor():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mind_amd.predictor import HipPredictor
    from mind_amd.weights import formula_state_dict
    hp = HipPredictor(0)
    hp.load_state_dict(formula_state_dict(seed=7, as_torch=True))
    yield hp
    hp.close()
    _write_shifts()


def _run(hp, form, shape, profiling, prof_clock):
    """cls / reg / vel of a full call and the edge tensor after five fusion layers, as raw bytes; the per-launch times of the full call"""
    prec, tile = FORMS[form]
    pb = _batch(shape)
    before = hp.pair_precision()
    try:
        hp.set_pair_precision(prec)
        hp.set_tuning("pair_tile", tile)
        hp.set_tuning("prof_clock", prof_clock)
        hp.set_profiling(profiling)
        out = hp.predict_numpy_batch(pb)
        got = {k: out[k].cpu().numpy().tobytes() for k in ("cls", "reg", "vel")}
        stats = dict(fusion=hp.fusion_stats(), actor=hp.last_actor_stats(), pair=hp.launch_times("pair"), act=hp.launch_times("actor")) if profiling else None
        hp.debug_set_layers(5)
        hp.predict_numpy_batch(pb)
        got["edge"] = hp.debug_read("edge").tobytes()
    finally:
        hp.debug_set_layers(6)
        hp.set_profiling(False)
        hp.set_tuning("prof_clock", 1)
        hp.set_tuning("pair_tile", 1)
        hp.set_pair_precision(before)
    return got, stats


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_bits_do_not_depend_on_how_launches_are_timed(form, shape, clock_predictor):
    hp = clock_predictor
    plain, _ = _run(hp, form, shape, False, 1)
    assert len(plain["edge"]) > 0
    for prof_clock in (0, 1, 2):
        got, stats = _run(hp, form, shape, True, prof_clock)
        for k in ("cls", "reg", "vel", "edge"):
            assert got[k] == plain[k], (form, shape, prof_clock, k)
        # the figures go out under the same names whichever mechanism measured them
        n, ms, _ = stats["fusion"]
        assert n == 6 and ms > 0.0, (form, shape, prof_clock, stats["fusion"])
        assert stats["actor"]["ms"] > 0.0, (form, shape, prof_clock, stats["actor"])
        ck, ev = stats["pair"]
        assert (len(ck), len(ev)) == {0: (0, 6), 1: (6, 0), 2: (6, 6)}[prof_clock], (form, shape, prof_clock, ck, ev)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", list(FORMS))
def test_clock_duration_is_positive_and_within_the_event_duration(form, shape, clock_predictor):
    hp = clock_predictor
    _run(hp, form, shape, True, 2)            # (first call of a shape: tables built, buffers grown, the ring sized)
    _, stats = _run(hp, form, shape, True, 2)
    for kind, want in (("pair", 6), ("act", 1)):
        ck, ev = stats[kind]
        assert len(ck) == len(ev) == want, (form, shape, kind, ck, ev)
        for i, (c, e) in enumerate(zip(ck, ev)):
            print(f"{form} {shape} {kind} launch {i}: clock {c * 1e3:8.2f} us  events {e * 1e3:8.2f} us  events - clock {(e - c) * 1e3:7.2f} us")
            SHIFTS.append((form, shape, kind, c, e))
        for i, (c, e) in enumerate(zip(ck, ev)):
            assert 0.0 < c <= e, (form, shape, kind, i, c, e)
    # the sums handed out are the clock's
    assert stats["fusion"][1] == pytest.approx(sum(stats["pair"][0]), rel=1e-5)
    assert stats["actor"]["ms"] == pytest.approx(stats["act"][0][0], rel=1e-5)


def _write_shifts():
    if not SHIFTS:
        return
    lines = ["# tests/test_gpu_launch_clock.py, \"prof_clock\" 2: every timed launch by the launch clock (first workgroup in to last workgroup out) and by HIP",
             "# events around it (with the dispatch on either side), us; events - clock is the size of the definition shift"]
    for kind in ("pair", "act"):
        d = np.array([(e - c) * 1e3 for f, s, k, c, e in SHIFTS if k == kind])
        ck = np.array([c * 1e3 for f, s, k, c, e in SHIFTS if k == kind])
        if d.size:
            lines.append(f"{'pair kernels' if kind == 'pair' else 'ActorNet'}: {d.size} launches, clock median {np.median(ck):.2f} us; events - clock: median {np.median(d):.2f} us, "
                         f"largest {d.max():.2f} us, smallest {d.min():.2f} us")
    for f, s, k, c, e in SHIFTS:
        lines.append(f"{f:14s} {s:14s} {k:5s} clock {c * 1e3:9.2f}  events {e * 1e3:9.2f}  events - clock {(e - c) * 1e3:8.2f}")
    print("\n".join(lines[:4]))
    try:
        with open(os.path.join(ROOT, "profiles", "launch_clock_vs_events.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    except OSError:
        pass          # (a read-only checkout: the lines above were printed)


def test_native_loop_plans_the_same_under_either_mechanism():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_native_loop import _make, _same, _snapshot
    pa, sa = _make("demo_1", None, episode_plans=6)
    pb, sb = _make("demo_1", None, episode_plans=6)
    assert sa._native is not None and sb._native is not None
    rt = pa.network.rt
    assert rt is pb.network.rt                 # (the planners of a thread share its context: the knob is set in front of every cycle)
    ta0, tb0 = sa._native.totals(), sb._native.totals()
    try:
        rt.set_profiling(True)
        for cycle in range(12):
            rt.set_tuning("prof_clock", 0)
            sa.run_plans(1)
            a = _snapshot(pa, sa)
            rt.set_tuning("prof_clock", 1)
            sb.run_plans(1)
            b = _snapshot(pb, sb)
            _same(a, b, cycle)
    finally:
        rt.set_profiling(False)
        rt.set_tuning("prof_clock", 1)
    assert sa.n_episodes == sb.n_episodes >= 1 and sa._native is not None and sb._native is not None
    ta, tb = sa._native.totals(), sb._native.totals()
    d = lambda t1, t0, k: t1[k] - t0[k]
    assert d(ta, ta0, "plans") == d(tb, tb0, "plans") == 12
    assert d(ta, ta0, "pair_launches") == d(tb, tb0, "pair_launches") > 0
    assert d(ta, ta0, "ilqr_launches") == d(tb, tb0, "ilqr_launches") > 0
    assert d(ta, ta0, "pair_ms") > 0.0 and d(tb, tb0, "pair_ms") > 0.0
    print(f"pair_ms over 12 cycles: events {d(ta, ta0, 'pair_ms'):.4f}  clock {d(tb, tb0, 'pair_ms'):.4f}  ({d(tb, tb0, 'pair_launches')} launches)")
