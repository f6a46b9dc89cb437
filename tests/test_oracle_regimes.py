"""CPU: what the weight regimes of tests/weight_regimes.py claim, pinned on the oracle -- so that the GPU tests that rely on them
(tests/test_gpu_predictor_regimes.py) cannot go quietly blind:

  * the float32 oracle stays within 3e-5 of the float64 oracle under every asserted regime (a condition on the inputs: the GPU bar is a
    multiple of that error);
  * attention is flat under the formula weights and peaked under `peaked`;
  * dropping the normalisation epsilon at any one of the 83 LayerNorm / GroupNorm sites moves an output by more than 5e-5 under `small`,
    and at next to none of them under the formula weights (why the regime is needed);
  * the oracle equals the imported reference network under `peaked`, `small` and `gains` (recorded values), so the oracle's own epsilon and
    softmax are the reference's."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import weight_regimes as wr
from mind_amd.synth import predictor_batch
from mind_amd.weights import state_dict_spec
from oracle import predictor as op
from oracle import ref_harness as rh
from ref_golden import Recorded
from test_oracle_predictor import TOL, to_t

EPS_MOVE = 5e-5             # an epsilon mutation "shows" when it moves some output by more than this (a quarter of the 2e-4 parity bar)


def outputs(sd, tb, dtype):
    """(reg, vel, cls) of all scenes as float64 numpy"""
    cls, reg, vel = op.forward(sd, tb, dtype=dtype)
    cat = lambda xs: np.concatenate([x.double().numpy().reshape(-1) for x in xs])
    return cat(reg), cat(vel), cat(cls)


def max_err(a, b):
    with np.errstate(invalid="ignore"):
        d = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
    return d if np.isfinite(d) else float("inf")


@pytest.mark.parametrize("a,l,B", [(8, 20, 2), (17, 30, 1), (3, 4, 1), (17, 30, 2), (16, 112, 1)])      # ... and the shapes of the GPU tests
@pytest.mark.parametrize("regime", wr.ASSERTED)
def test_reference_error_per_regime(regime, a, l, B):
    """Measured max |float32 - float64| over reg, vel, cls at these shapes: plain / seed7 <= 3.1e-6, peaked <= 1.9e-5, small <= 4.7e-7,
    offset <= 1.2e-5, gains <= 1.5e-5 (saturated: 3e-4 .. 1.5e-3, which is why it is not an asserted regime).  The float32 figure moves
    with the BLAS and its thread count (peaked: 1.3e-5 .. 1.9e-5 on two hosts)."""
    sd = wr.regime_state_dict(regime)
    tb = to_t(predictor_batch(a, l, B, seed=wr.BATCH_SEED))
    e = max_err(outputs(sd, tb, torch.float32), outputs(sd, tb, torch.float64))
    print(f"{regime} a={a} l={l} B={B}: max |float32 oracle - float64 oracle| = {e:.2e}")
    assert e <= wr.REF_ERR_BAR


def _fusion_peaks(monkeypatch, regime):
    """median over (query, head) of the largest attention weight, per fusion layer of one (8, 20) scene"""
    peaks = []
    real = torch.softmax

    def tapped(x, dim=-1, **kw):
        p = real(x, dim=dim, **kw)
        if x.dim() == 3 and x.shape[1] == 8 and x.shape[0] == x.shape[2]:      # fusion_layer's [query j, head, key i]
            peaks.append(float(p.max(dim=-1).values.median()))
        return p
    monkeypatch.setattr(torch, "softmax", tapped)
    op.forward(wr.regime_state_dict(regime), to_t(predictor_batch(8, 20, 1, seed=wr.BATCH_SEED)), dtype=torch.float64)
    monkeypatch.setattr(torch, "softmax", real)
    assert len(peaks) == 6
    return peaks


def test_attention_is_flat_under_formula_weights_and_peaked_under_peaked(monkeypatch):
    """Uniform is 1/29 = 0.034 at N = 29."""
    flat, sharp = _fusion_peaks(monkeypatch, "plain"), _fusion_peaks(monkeypatch, "peaked")
    print("median peak attention weight per fusion layer: plain", [f"{v:.3f}" for v in flat], "peaked", [f"{v:.3f}" for v in sharp])
    assert max(flat) <= 0.1
    assert min(sharp) >= 0.4


def _eps_moved_sites(monkeypatch, regime):
    """norm sites at which dropping the epsilon moves some output (reg, vel, cls) by more than EPS_MOVE; float64, (8, 20, 1)"""
    sd = wr.regime_state_dict(regime)
    sites = wr.norm_sites(sd)
    assert len(sites) == 83 and len(set(sites)) == 83
    tb = to_t(predictor_batch(8, 20, 1, seed=wr.BATCH_SEED))
    base = outputs(sd, tb, torch.float64)
    site = [None]
    # copies of the oracle's two normalisations whose epsilon is 0 at the named site
    ln = lambda x, s, p, dt: F.layer_norm(x, (x.shape[-1],), op._w(s, p + ".weight", dt), op._w(s, p + ".bias", dt), 0.0 if p == site[0] else 1e-5)
    gn = lambda x, s, p, dt: F.group_norm(x, 1, op._w(s, p + ".weight", dt), op._w(s, p + ".bias", dt), 0.0 if p == site[0] else 1e-5)
    monkeypatch.setattr(op, "_ln", ln)
    monkeypatch.setattr(op, "_gn", gn)
    assert max_err(outputs(sd, tb, torch.float64), base) == 0.0          # the copies are the oracle's own when no site is named
    moved = []
    for s in sites:
        site[0] = s
        if max_err(outputs(sd, tb, torch.float64), base) > EPS_MOVE:
            moved.append(s)
    monkeypatch.undo()
    return moved, sites


def test_epsilon_shows_at_every_norm_site_under_small(monkeypatch):
    moved, sites = _eps_moved_sites(monkeypatch, "small")
    assert moved == sites, sorted(set(sites) - set(moved))


def test_epsilon_is_invisible_under_formula_weights(monkeypatch):
    """... which is why the `small` regime exists: with formula weights a kernel whose epsilon is missing passes a 2e-4 bar at all but a
    handful of its normalisations."""
    moved, _ = _eps_moved_sites(monkeypatch, "plain")
    print(f"plain: epsilon visible at {len(moved)} of 83 sites: {moved}")
    assert len(moved) <= 5


def test_gpu_shapes_reach_the_column_split_mechanisms():
    """The three scene sizes of tests/test_gpu_predictor_regimes.py on the pair kernels' host-side schedule (mind_debug_pair_schedule, no device):
    N = 8 one job per column; N = 48 three one-tile partials per column; N = 129 eight partials per column, one of them over two tiles (the
    running-maximum rescale inside a job and the recombination across jobs both run)."""
    import ctypes as C
    from mind_amd import _lib
    from test_gpu_predictor_regimes import SHAPES
    lib = _lib.load()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    spans = {}
    for a, l, _ in SHAPES:
        N = a + l + 1
        out, info = np.zeros((N * 8, 6), np.int32), np.zeros(4, np.int32)
        n = lib.mind_debug_pair_schedule(ip(np.array([N], np.int32)), ip(np.array([1], np.int32)), 1, 256, 0, ip(out), N * 8, ip(info))
        assert n == N * info[0]
        col0 = out[:n][out[:n, 1] == 0]                      # [scene, column, first tile, end tile, ...] of column 0's jobs
        spans[N] = sorted((col0[:, 3] - col0[:, 2]).tolist())
    assert spans == {8: [1], 48: [1, 1, 1], 129: [1] * 7 + [2]}


@pytest.mark.reference
@pytest.mark.parametrize("regime", ["peaked", "small", "gains"])
def test_oracle_matches_imported_reference_under_regime(regime):
    sd = wr.regime_state_dict(regime)
    tb = to_t(predictor_batch(6, 9, 2, seed=7))

    def ref():
        m = rh.ref_modules()
        net = rh.build_ref_network(sd)
        get_rpe = m["planners.mind.utils"].get_rpe
        rpes = [{"scene": get_rpe(c, v)[0], "scene_mask": None} for c, v in zip(tb["CTRS"], tb["VECS"])]
        with torch.no_grad():
            rc, rr, ra = net((tb["ACTORS"], tb["ACTOR_IDCS"], tb["LANES"], tb["LANE_IDCS"], rpes, tb["TGT_NODES"], tb["TGT_RPE"]))
        return list(net.state_dict().keys()), [rc[b] for b in range(2)], [rr[b] for b in range(2)], [ra[b][0] for b in range(2)]
    keys, rc, rr, ra = Recorded("oracle_regimes")("batch6x9x2_seed7_" + regime, ref)
    assert [k for k, _ in state_dict_spec()] == keys
    oc, orr, ov = op.forward(sd, tb)
    for b in range(2):
        assert (torch.as_tensor(rc[b]) - oc[b]).abs().max() < 1e-6
        assert (torch.as_tensor(rr[b]) - orr[b]).abs().max() < TOL
        assert (torch.as_tensor(ra[b]) - ov[b]).abs().max() < TOL
