"""GPU: the decoder's aux outputs (cov_vel, param: the rest of the reference's res_aux, network.py:554), the monomial curve basis
(param_out='monomial', network.py:422-435, :466-481, :525-534) and curve sampling at arbitrary times (k_dec_curve), for every form of the
decoder's actor part: k_dec_actor<0> ("dec_overlap" 0), the split head k_dec_actor<2, RAT> ("dec_head_ra" 1 / 2 / 4) and
k_dec_actor_mfma<NP> ("dec_mfma_min" 0 under bf16x6: NP = 6, and under bf16x3 with "actor_split" 3: NP = 3).

Against tests/golden/decoder_aux.npz (the imported reference, both bases: tests/golden/gen_decoder_aux.py), against a float64 restatement
from the device's own control points under the rounding-error bound of tests/decoder_aux_restate.py, across the forms bit for bit on ragged
agent counts with a guard row behind every output, and with / without aux.  Nothing here reads the reference tree."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decoder_aux_restate import GRID, bound_violations, reference64  # noqa: E402

from mind_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 2e-4          # the project's bar against the reference (tests/test_gpu_predictor.py)
CLS_TOL = 1e-5
CASES = [(3, 4, 2, 1), (2, 2, 1, 3), (5, 6, 3, 2)]
# (knobs, arithmetic or None = the context's) of every form of the decoder's actor part
FORMS = {
    "one": ({"dec_overlap": 0}, None),
    "split1": ({"dec_head_ra": 1}, None),
    "split2": ({"dec_head_ra": 2}, None),
    "split4": ({"dec_head_ra": 4}, None),
    "mfma_x6": ({"dec_mfma_min": 0}, "bf16x6"),
    "mfma_x3": ({"dec_mfma_min": 0, "actor_split": 3}, "bf16x3"),
}
IRREGULAR = np.array([0.0, 1.0, 1 / 59 - 1e-9, 1 / 59 + 1e-9, 0.5, 0.123456789, 0.999, 0.25, 0.75, 1 / 3, 2 / 3, 0.01, 0.99, 0.6180339887, 0.0001,
                      0.9999, 0.42])
assert len(IRREGULAR) == 17


def _created_with():
    """the knobs this file moves, as a context is created with them (the library's defaults or their MIND_* overrides)"""
    env = lambda k, d: int(os.environ.get("MIND_" + k.upper(), d))
    return {"dec_overlap": env("dec_overlap", 1), "dec_head_ra": env("dec_head_ra", 0), "dec_mfma_min": env("dec_mfma_min", 1 << 30),
            "actor_split": env("actor_split", 6)}


class _Form:
    """a form of the actor part (and a curve basis) on a predictor for the length of a with block; everything is put back afterwards"""

    def __init__(self, hp, form=None, basis=None):
        self.hp, self.form, self.basis = hp, form, basis

    def __enter__(self):
        hp = self.hp
        self.prec, self.was_basis = hp.pair_precision(), hp.get_decoder_basis()
        if self.form is not None:
            knobs, prec = FORMS[self.form]
            for k, v in knobs.items():
                hp.set_tuning(k, v)
            if prec is not None:
                hp.set_pair_precision(prec)
        if self.basis is not None:
            hp.set_decoder_basis(self.basis)
        return hp

    def __exit__(self, *exc):
        hp = self.hp
        hp.synchronize()
        for k, v in _created_with().items():
            hp.set_tuning(k, v)
        hp.set_pair_precision(self.prec)
        hp.set_decoder_basis(self.was_basis)
        return False


@pytest.fixture(scope="module")
def fixture_aux():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "decoder_aux.npz")))


def _key(basis, case):
    return "%s_a%d_l%d_b%d_s%d" % ((basis,) + tuple(case))


def _np(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _expected_form(hp, form, pb):
    """the kernel-choice record says the form under test is the one that runs (a knob that stopped selecting it would make the test vacuous)"""
    scenes = [(len(a), len(l)) for a, l in zip(pb["ACTOR_IDCS"], pb["LANE_IDCS"])]
    knobs = dict(_created_with())
    knobs.update(FORMS[form][0])
    ch = _lib.predict_choice(knobs, FORMS[form][1] or hp.pair_precision(), scenes)
    want = {"one": (0, 0, 0), "split1": (1, 1, 0), "split2": (1, 2, 0), "split4": (1, 4, 0), "mfma_x6": (2, 0, 6), "mfma_x3": (2, 0, 3)}[form]
    assert (ch["dec_actor"], ch["dec_head_ra"], ch["dec_np"]) == want, (form, ch["dec_actor"], ch["dec_head_ra"], ch["dec_np"])


# ---- 1. against the fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_l%d_b%d_s%d" % tuple(c))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("basis", _lib.BASIS)
def test_every_form_matches_the_reference_in_both_bases(hip_predictor, fixture_aux, basis, form, case):
    from mind_amd.synth import predictor_batch
    a, l, B, seed = case
    pb = predictor_batch(a, l, B, seed=seed)
    _expected_form(hip_predictor, form, pb)
    with _Form(hip_predictor, form, basis) as hp:
        out = _np(hp.predict_numpy_batch(pb, aux=True))
    g, k = fixture_aux, _key(basis, case)
    assert out["cov_vel"].shape == (a * B, 6, 60, 3) and out["param"].shape == (a * B, 6, 8, 5)
    err = {n: float(np.abs(out[n] - g[k + "_" + n]).max()) for n in ("cls", "reg", "vel", "cov_vel", "param")}
    print(basis, form, k, " ".join("%s %.2e" % kv for kv in err.items()))
    assert err["cls"] < CLS_TOL, err
    assert max(err[n] for n in ("reg", "vel", "cov_vel", "param")) < TOL, err


# ---- 2. against float64 from the device's own control points ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("basis", _lib.BASIS)
def test_curve_step_is_within_the_rounding_bound_of_float64(hip_predictor, basis, form):
    """reg / vel / cov_vel recomputed in float64, with float64 tables, from the param the same call returned: |o_dev - o_64| <= 16 u S for
    the linear outputs, relative 16 u S + 4 u for the three exp outputs (tests/decoder_aux_restate.py; the CPU test of that file's
    emulation found 0.18-0.27 of the bound)"""
    from mind_amd.synth import predictor_batch
    pb = predictor_batch(5, 6, 3, seed=2)
    with _Form(hip_predictor, form, basis) as hp:
        out = _np(hp.predict_numpy_batch(pb, aux=True))
    worst = bound_violations(out["param"], basis, GRID, out["reg"], out["vel"], out["cov_vel"])
    print(basis, form, worst)
    assert max(worst.values()) <= 1.0, worst


# ---- 3. ragged counts: the forms agree bit for bit, nothing lands behind row A -----------------------------------------------------------
def _inputs(hp, pb):
    import torch
    dev = hp.device
    B = len(pb["ACTOR_IDCS"])
    a_off = [0] + [int(v) for v in np.cumsum([len(x) for x in pb["ACTOR_IDCS"]])]
    l_off = [0] + [int(v) for v in np.cumsum([len(x) for x in pb["LANE_IDCS"]])]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    na = [a_off[b + 1] - a_off[b] for b in range(B)]
    ten = dict(actors=t(pb["ACTORS"]), lanes=t(pb["LANES"]), tgt_nodes=t(pb["TGT_NODES"]), tgt_rpe=t(pb["TGT_RPE"]),
               actor_ctrs=t(np.concatenate([pb["CTRS"][b][:na[b]] for b in range(B)])), actor_vecs=t(np.concatenate([pb["VECS"][b][:na[b]] for b in range(B)])),
               lane_ctrs=t(np.concatenate([pb["CTRS"][b][na[b]:] for b in range(B)])), lane_vecs=t(np.concatenate([pb["VECS"][b][na[b]:] for b in range(B)])))
    return B, a_off, l_off, ten


def _raw_predict(hp, pb, entry="aux", aux=("cov_vel", "param")):
    """mind_predict_batch (entry "plain") or mind_predict_batch_aux (aux: the pointers that are set; None = a null mind_pred_aux) into
    buffers of A + 1 rows filled with NaN: -> dict of the A rows, after checking that row A is still NaN in every buffer"""
    import torch
    B, a_off, l_off, ten = _inputs(hp, pb)
    A = a_off[-1]
    nan = lambda *s: torch.full(s, float("nan"), device=hp.device)
    out = {"cls": nan(B + 1, 6), "reg": nan(A + 1, 6, 60, 5), "vel": nan(A + 1, 6, 60, 2), "cov_vel": nan(A + 1, 6, 60, 3), "param": nan(A + 1, 6, 8, 5)}
    sb = _lib.SceneBatch()
    sb.n_scenes = B
    sb.actor_off, sb.lane_off = (C.c_int32 * (B + 1))(*a_off), (C.c_int32 * (B + 1))(*l_off)
    for k, v in ten.items():
        setattr(sb, k, C.c_void_p(v.data_ptr()))
    po = _lib.PredOut()
    po.cls, po.reg, po.vel = out["cls"].data_ptr(), out["reg"].data_ptr(), out["vel"].data_ptr()
    if entry == "plain":
        rc = hp.lib.mind_predict_batch(hp.ctx, C.byref(sb), C.byref(po))
    else:
        pa = None
        if aux is not None:
            pa = _lib.PredAux(out["cov_vel"].data_ptr() if "cov_vel" in aux else None, out["param"].data_ptr() if "param" in aux else None)
        rc = hp.lib.mind_predict_batch_aux(hp.ctx, C.byref(sb), C.byref(po), C.byref(pa) if pa is not None else None)
    _lib.check(hp.lib, hp.ctx, rc, "mind_predict_batch_aux")
    hp.synchronize()
    res = _np(out)
    written = {"cls", "reg", "vel"} | (set(aux or ()) if entry == "aux" else set())
    for k, v in res.items():
        n = B if k == "cls" else A
        assert np.isnan(v[n:]).all(), (k, "a write behind the last row")
        if k in written:
            assert np.isfinite(v[:n]).all(), k
        else:
            assert np.isnan(v).all(), (k, "written though not asked for")
    return {k: v[:(B if k == "cls" else A)] for k, v in res.items()}


@pytest.fixture(scope="module")
def seed7_predictor():
    import weight_regimes as wr
    from mind_amd.predictor import HipPredictor
    hp = HipPredictor(0)
    hp.load_state_dict(wr.regime_state_dict("seed7"))
    yield hp
    hp.close()


@pytest.mark.parametrize("scenes", [1, 3])
@pytest.mark.parametrize("agents", [1, 3, 5, 9])
@pytest.mark.parametrize("basis", _lib.BASIS)
def test_forms_agree_bit_for_bit_on_ragged_counts_and_stay_inside_their_rows(seed7_predictor, basis, agents, scenes):
    """random weights (formula weights can hide a wrong row); the VALU forms are one arithmetic, each MFMA form its own"""
    from mind_amd.synth import predictor_batch
    pb = predictor_batch(agents, 4, scenes, seed=3)
    outs = {}
    for form in FORMS:
        with _Form(seed7_predictor, form, basis) as hp:
            outs[form] = _raw_predict(hp, pb)
    ref = outs["split4"]
    assert np.unique(ref["param"].reshape(agents * scenes * 6, -1), axis=0).shape[0] == agents * scenes * 6      # every (agent, mode) row differs
    for form in ("one", "split1", "split2"):
        for k in ("cls", "reg", "vel", "cov_vel", "param"):
            assert _same_bits(outs[form][k], ref[k]), (form, k)
    for form in ("mfma_x6", "mfma_x3"):      # (other arithmetics: same rows, close values)
        for k in ("reg", "vel", "cov_vel", "param"):
            assert np.abs(outs[form][k] - ref[k]).max() < 1e-2 * max(1.0, float(np.abs(ref[k]).max())), (form, k)


# ---- 4. aux changes nothing else -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_aux_outputs_leave_cls_reg_vel_bit_identical(seed7_predictor, form):
    from mind_amd.synth import predictor_batch
    pb = predictor_batch(5, 4, 3, seed=3)
    scenes = [(len(a), len(l)) for a, l in zip(pb["ACTOR_IDCS"], pb["LANE_IDCS"])]
    with _Form(seed7_predictor, form) as hp:
        knobs = dict(_created_with(), **FORMS[form][0])
        before = _lib.predict_choice(knobs, hp.pair_precision(), scenes)
        plain = _raw_predict(hp, pb, entry="plain")
        null = _raw_predict(hp, pb, aux=None)
        both = _raw_predict(hp, pb)
        only_c = _raw_predict(hp, pb, aux=("cov_vel",))
        only_p = _raw_predict(hp, pb, aux=("param",))
        empty = _raw_predict(hp, pb, aux=())
        # the launches of a call are a function of knobs, arithmetic and scene sizes alone (pred_choose): aux is not among its inputs and adds none
        assert _lib.predict_choice(knobs, hp.pair_precision(), scenes) == before and len(before) == len(_lib.PRED_CHOICE_FIELDS) + 1
    for name, o in (("null aux", null), ("both", both), ("cov_vel only", only_c), ("param only", only_p), ("no pointer", empty)):
        for k in ("cls", "reg", "vel"):
            assert _same_bits(o[k], plain[k]), (form, name, k)
    assert _same_bits(only_c["cov_vel"], both["cov_vel"]) and _same_bits(only_p["param"], both["param"])


# ---- 5. curve sampling -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_curves(seed7_predictor):
    """per basis: the decoder's own outputs for 9 agents (54 rows of control points), kept on the device"""
    from mind_amd.synth import predictor_batch
    pb = predictor_batch(9, 4, 1, seed=3)
    res = {}
    for basis in _lib.BASIS:
        with _Form(seed7_predictor, None, basis) as hp:
            res[basis] = hp.predict_numpy_batch(pb, aux=True)
    return res


@pytest.mark.parametrize("explicit", [False, True], ids=["context_basis", "explicit_basis"])
@pytest.mark.parametrize("basis", _lib.BASIS)
def test_curve_eval_on_the_decoders_grid_is_the_decoder_bit_for_bit(seed7_predictor, device_curves, basis, explicit):
    dec = device_curves[basis]
    other = _lib.BASIS[1 - _lib.BASIS.index(basis)]
    # explicit: the context is set to the OTHER basis and the call names its own; else the context's basis through basis = -1
    with _Form(seed7_predictor, None, other if explicit else basis) as hp:
        got = _np(hp.curve_eval(dec["param"], GRID, basis=basis if explicit else None))
    for k in ("reg", "vel", "cov_vel"):
        assert _same_bits(got[k], dec[k].cpu().numpy()), (basis, k)


@pytest.mark.parametrize("n_tau", [1, 60, 301])
@pytest.mark.parametrize("n_rows", [1, 7, 54])
@pytest.mark.parametrize("basis", _lib.BASIS)
def test_curve_eval_shapes_against_float64_and_single_outputs(seed7_predictor, device_curves, basis, n_rows, n_tau):
    hp = seed7_predictor
    param = device_curves[basis]["param"].reshape(54, 8, 5)[:n_rows].contiguous()
    tau = np.array([0.37]) if n_tau == 1 else np.linspace(0.0, 1.0, n_tau)
    got = _np(hp.curve_eval(param, tau, basis=basis))
    assert got["reg"].shape == (n_rows, n_tau, 5) and got["vel"].shape == (n_rows, n_tau, 2) and got["cov_vel"].shape == (n_rows, n_tau, 3)
    worst = bound_violations(param.cpu().numpy(), basis, tau, got["reg"], got["vel"], got["cov_vel"])
    print(basis, n_rows, n_tau, worst)
    assert max(worst.values()) <= 1.0, worst
    for k in ("reg", "vel", "cov_vel"):
        alone = _np(hp.curve_eval(param, tau, basis=basis, want=(k,)))
        assert list(alone) == [k] and _same_bits(alone[k], got[k]), k


@pytest.mark.parametrize("basis", _lib.BASIS)
def test_curve_eval_at_irregular_times_and_at_the_end_points(seed7_predictor, device_curves, basis):
    hp = seed7_predictor
    param = device_curves[basis]["param"].reshape(54, 8, 5)
    p = param.cpu().numpy()
    got = _np(hp.curve_eval(param, IRREGULAR, basis=basis))
    worst = bound_violations(p, basis, IRREGULAR, got["reg"], got["vel"], got["cov_vel"])
    print(basis, worst)
    assert max(worst.values()) <= 1.0, worst
    assert np.abs(got["reg"] - reference64(p, basis, IRREGULAR)[0]).max() < TOL * max(1.0, float(np.abs(got["reg"]).max()))
    # tau = 0 is the first control point in both bases, tau = 1 the last one under Bezier: exactly (the other basis entries are 0)
    assert _same_bits(got["reg"][:, 0, :2], p[:, 0, :2])
    if basis == "bezier":
        assert _same_bits(got["reg"][:, 1, :2], p[:, 7, :2])
    # 1/59 -+ 1e-9 straddle the decoder's second sample: continuous there
    assert np.abs(got["reg"][:, 2] - got["reg"][:, 3]).max() < 1e-5 * max(1.0, float(np.abs(got["reg"]).max()))


def test_curve_eval_rejects_bad_arguments_by_name(seed7_predictor, device_curves):
    import torch
    hp = seed7_predictor
    param = device_curves["bezier"]["param"].reshape(54, 8, 5)
    out = torch.full((54 * 4 * 5 + 1,), float("nan"), device=hp.device)
    dp = C.POINTER(C.c_double)

    def call(tau, basis=0, n_rows=54, n_tau=None, reg=True, p=True):
        tau = np.ascontiguousarray(tau, np.float64)
        return hp.lib.mind_curve_eval(hp.ctx, basis, C.c_void_p(param.data_ptr()) if p else None, n_rows, tau.ctypes.data_as(dp),
                                      len(tau) if n_tau is None else n_tau, C.c_void_p(out.data_ptr()) if reg else None, None, None)

    E = _lib.MIND_EINVAL
    for bad in ([float("nan")], [float("inf")], [-1e-9], [1.0 + 1e-9], [0.1, 0.2, 7.0, 0.3]):
        assert call(bad) == E, bad
    assert call([0.5], n_tau=0) == E and call([0.5], n_tau=-1) == E
    assert call([0.5], n_rows=-1) == E
    assert call([0.5], reg=False) == E                       # all three outputs null
    assert call([0.5], basis=2) == E and call([0.5], basis=-2) == E
    assert call([0.5], p=False) == E                         # rows but no control points
    assert call([0.5] * 4, n_rows=(1 << 26) // 4 + 1) == E    # n_rows * n_tau above MIND_CURVE_MAX_POINTS
    assert call([0.5], n_rows=(1 << 40)) == E
    assert b"points supported" in hp.lib.mind_last_error_string(hp.ctx)
    hp.synchronize()
    assert torch.isnan(out).all()                            # none of the rejected calls wrote
    assert call([0.5] * 4, n_rows=0) == _lib.MIND_OK and call([0.5], n_rows=0, p=False) == _lib.MIND_OK       # a successful no-op
    hp.synchronize()
    assert torch.isnan(out).all()
    assert call([0.0, 0.25, 0.5, 1.0]) == _lib.MIND_OK       # ... and the context still works
    hp.synchronize()
    assert torch.isfinite(out[:-1]).all() and torch.isnan(out[-1])
    with pytest.raises(ValueError):
        hp.curve_eval(param, [0.5], basis="spline")
    with pytest.raises(ValueError):
        hp.curve_eval(param, [0.5], want=("reg", "acc"))


# ---- 6. basis state --------------------------------------------------------------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_basis_setting_holds_across_loads_and_switching_back_restores_the_bits(formula_sd, fixture_aux):
    from mind_amd.predictor import HipPredictor
    from mind_amd.synth import predictor_batch
    case = CASES[0]
    pb = predictor_batch(*case[:3], seed=case[3])
    kb, km = _key("bezier", case), _key("monomial", case)
    close = lambda out, k: all(np.abs(out[n] - fixture_aux[k + "_" + n]).max() < TOL for n in ("reg", "vel", "cov_vel", "param"))
    hp = HipPredictor(0)
    try:
        assert hp.get_decoder_basis() == "bezier"
        hp.set_decoder_basis("monomial")                    # set before the first load
        hp.load_state_dict(formula_sd)
        m0 = _np(hp.predict_numpy_batch(pb, aux=True))
        assert hp.get_decoder_basis() == "monomial" and close(m0, km) and not close(m0, kb)
        hp.load_state_dict(formula_sd)                      # a second load keeps the setting
        m1 = _np(hp.predict_numpy_batch(pb, aux=True))
        assert hp.get_decoder_basis() == "monomial" and all(_same_bits(m0[k], m1[k]) for k in m0)
        hp.set_decoder_basis("bezier")                      # set after the load: the tables are rewritten in place
        b0 = _np(hp.predict_numpy_batch(pb, aux=True))
        assert close(b0, kb) and not close(b0, km)
        assert _same_bits(b0["param"], m0["param"])         # (the control points do not depend on the basis)
    finally:
        hp.close()
    hp = HipPredictor(0)
    try:
        hp.load_state_dict(formula_sd)                      # a context that never left Bezier: the parent's bits
        never = _np(hp.predict_numpy_batch(pb))
        hp.set_decoder_basis("monomial")                    # set after the load ...
        m2 = _np(hp.predict_numpy_batch(pb, aux=True))
        assert all(_same_bits(m2[k], m0[k]) for k in m0)    # ... equals set before the load
        hp.load_state_dict(formula_sd, param_out="bezier")  # and back through load_state_dict's argument
        back = _np(hp.predict_numpy_batch(pb))
        assert hp.get_decoder_basis() == "bezier"
        for k in ("cls", "reg", "vel"):
            assert _sha(back[k]) == _sha(never[k]) == _sha(b0[k]), k
        assert hp.lib.mind_set_decoder_basis(hp.ctx, 2) == _lib.MIND_EINVAL and hp.lib.mind_set_decoder_basis(hp.ctx, -1) == _lib.MIND_EINVAL
        assert hp.get_decoder_basis() == "bezier"
        with pytest.raises(ValueError):
            hp.set_decoder_basis("none")
    finally:
        hp.close()


def test_a_busy_context_refuses_a_basis_change(hip_predictor):
    """a tree-iLQR call begun with mind_ilqr_contingency_begin is pending: MIND_ESTATE, the basis stays, and the call still finishes"""
    from mind_amd.predictor import IlqrCall
    from mind_amd.synth import scripted_scenario_tree
    from oracle import ilqr as oi
    hp = hip_predictor
    sst = scripted_scenario_tree("lead", 4)
    flat = oi.flatten(sst["nodes"])
    x0 = oi.init_state(sst["state"], sst["ctrl"])
    call = IlqrCall(hp.lib, oi.default_cfg(), [flat], x0, sst["target_lane"], sst["target_vel"], cfg_full=oi.default_cfg()).begin(hp)
    assert call.rc == _lib.MIND_OK
    try:
        assert hp.lib.mind_set_decoder_basis(hp.ctx, 1) == _lib.MIND_ESTATE
        assert b"tree-iLQR" in hp.lib.mind_last_error_string(hp.ctx)
        assert hp.lib.mind_set_decoder_basis(hp.ctx, 0) == _lib.MIND_ESTATE      # (even to the basis it has: the context is not to be touched)
        assert hp.get_decoder_basis() == "bezier"
    finally:
        call.wait()
    xs, us, st_w, st_f = call.finish()
    assert np.isfinite(xs[0]).all() and st_f[0]["iterations"] > 0
    assert hp.lib.mind_set_decoder_basis(hp.ctx, 0) == _lib.MIND_OK


# ---- 7. the native plan under the monomial basis -----------------------------------------------------------------------------------------
def test_native_plan_equals_the_round_path_under_the_monomial_basis():
    """tests/test_gpu_aime_native.py's smallest synthetic world (16 agents, 4 lanes), the predictor's OWN modes (branching formula weights; the
    scripted modes would overwrite what the basis changes): mind_aime_plan and the round-by-round Python path run the same predictor stages,
    so with the contexts set to monomial their trees are identical -- and they are not the Bezier trees.  (Observed: decoded with the monomial
    basis, the Bezier-shaped formula weights end the tree after its root round -- 2 internal nodes and 1 tree node per cycle against 3 and 2
    under Bezier -- so this compares one round per cycle, not a deep tree.)"""
    sys.path.insert(0, ROOT)
    from bench import BRANCHING_WEIGHTS, make_closed_loop
    from test_gpu_aime_native import _flat
    wkw = dict(n_agents=16, n_lanes=4, n_segs=8, seed=4)
    sims = []
    for native, basis in ((True, "monomial"), (False, "monomial"), (True, "bezier")):
        pl, sim, _ = make_closed_loop(wkw, scripted=False, ckpt=BRANCHING_WEIGHTS, speculative=False, own_context=True)
        pl.scen_tree_gen.native_aime = native
        pl.scen_tree_gen.device_root = False
        pl.network.rt.set_decoder_basis(basis)
        sims.append((pl, sim))
    try:
        differs = 0
        for cycle in range(2):
            res = []
            for pl, sim in sims:
                sim.run_plans(1)
                gen = pl.scen_tree_gen
                internal = [(k, n.parent_key, bool(n.data.branch_flag), bool(n.data.end_flag), bool(n.data.terminate_flag)) for k, n in gen.tree.nodes.items()]
                res.append((internal, _flat(gen.get_scenario_tree()), np.array(sim.ctrl)))
            (ia, fa, ca), (ib, fb, cb), (ic, fc, cc) = res
            print("cycle", cycle, "internal nodes", len(ia), "tree nodes", len(fa), "bezier:", len(ic), len(fc))
            assert ia == ib and len(fa) == len(fb) and np.array_equal(ca, cb), cycle
            for x, y in zip(fa, fb):
                assert x[0] == y[0] and x[1] == y[1]
                for u, v in zip(x[2:], y[2:]):
                    assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v), (cycle, x[0])
            differs += len(fa) != len(fc) or any(u.shape != v.shape or not np.array_equal(u, v) for x, y in zip(fa, fc) for u, v in zip(x[2:], y[2:]))
        assert sims[0][0].scen_tree_gen.n_native_plans == 2 and sims[1][0].scen_tree_gen.n_native_plans == 0
        assert differs == 2
    finally:
        for pl, _ in sims:
            pl.network.rt.close()


# ---- 8. ScenePredNet -------------------------------------------------------------------------------------------------------------------
def _net_data(pb):
    return {k: pb[k] for k in ("ACTORS", "ACTOR_IDCS", "LANES", "LANE_IDCS", "TGT_NODES", "TGT_RPE")} | \
        {"ACTOR_CTRS": np.concatenate([c[:len(i)] for c, i in zip(pb["CTRS"], pb["ACTOR_IDCS"])]),
         "ACTOR_VECS": np.concatenate([c[:len(i)] for c, i in zip(pb["VECS"], pb["ACTOR_IDCS"])]),
         "LANE_CTRS": np.concatenate([c[len(i):] for c, i in zip(pb["CTRS"], pb["ACTOR_IDCS"])]),
         "LANE_VECS": np.concatenate([c[len(i):] for c, i in zip(pb["VECS"], pb["ACTOR_IDCS"])])}


def test_scene_pred_net_returns_the_references_res_aux(formula_sd, fixture_aux, hip_predictor):
    import torch
    from mind_amd import runtime
    from mind_amd.planners.mind.networks.network import ScenePredNet
    from mind_amd.synth import predictor_batch
    case = CASES[2]
    a, l, B, seed = case
    pb = predictor_batch(a, l, B, seed=seed)
    dev = torch.device("cuda", 0)
    net = ScenePredNet({"param_out": "monomial"}, dev, own_context=True)
    try:
        net.want_aux = True
        net.load_state_dict(formula_sd)
        assert net.rt.get_decoder_basis() == "monomial"
        with torch.cuda.stream(net.rt.torch_stream):      # (a context of its own runs on a stream of its own: the uploads belong on it)
            rc, rr, ra = net(net.pre_process(_net_data(pb)))
        net.rt.synchronize()
        k = _key("monomial", case)
        assert len(rc) == len(rr) == len(ra) == B
        for b in range(B):
            vel, cov_vel, param = ra[b]
            sl = slice(b * a, (b + 1) * a)
            assert tuple(rc[b].shape) == (1, 6) and tuple(rr[b].shape) == (a, 6, 60, 5) and tuple(vel.shape) == (a, 6, 60, 2)
            assert tuple(cov_vel.shape) == (a, 6, 60, 3) and tuple(param.shape) == (6, a, 8, 5)          # the reference's layouts
            assert np.abs(rr[b].cpu().numpy() - fixture_aux[k + "_reg"][sl]).max() < TOL
            assert np.abs(vel.cpu().numpy() - fixture_aux[k + "_vel"][sl]).max() < TOL
            assert np.abs(cov_vel.cpu().numpy() - fixture_aux[k + "_cov_vel"][sl]).max() < TOL
            assert np.abs(param.permute(1, 0, 2, 3).cpu().numpy() - fixture_aux[k + "_param"][sl]).max() < TOL
            assert np.abs(rc[b].cpu().numpy()[0] - fixture_aux[k + "_cls"][b]).max() < CLS_TOL
    finally:
        net.rt.close()
    # the default object: Bezier, (vel, None, None), on the thread's shared context -- which a net of another basis may not take over
    shared = runtime.get_runtime(0)
    plain = ScenePredNet(None, dev)
    assert plain.rt is shared and plain.want_aux is False and plain.param_out == "bezier"
    plain.load_state_dict(formula_sd)
    rc, rr, ra = plain(plain.pre_process(_net_data(pb)))
    kb = _key("bezier", case)
    assert all(len(x) == 3 and x[1] is None and x[2] is None for x in ra)
    assert np.abs(torch.cat(rr).cpu().numpy() - fixture_aux[kb + "_reg"]).max() < TOL
    intruder = ScenePredNet({"param_out": "monomial"}, dev)
    assert intruder.rt is shared
    with pytest.raises(RuntimeError, match="own_context=True"):
        intruder.load_state_dict(formula_sd)
    assert shared.get_decoder_basis() == "bezier"
