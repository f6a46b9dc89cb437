"""CPU: the decoder's curve bases as the host evaluates them (mind_debug_curve_basis; weight_pack.h wp_basis_rows) against a float64
restatement of the reference's four table functions (planners/mind/networks/network.py:449-481), against the packed weight blob, at the
end points and for the arguments the library rejects; and ScenePredNet's reading of cfg["param_out"]."""
import ctypes as C
import math

import numpy as np
import pytest

from mind_amd import _lib

GRID = np.linspace(0.0, 1.0, 60, endpoint=True)


def tables64(basis, ts):
    """network.py:449-481 in float64 at the times ts: (T [n,8], Tp [n,7])"""
    ts = np.asarray(ts, np.float64)
    if basis == "bezier":
        T = [math.comb(7, i) * (1.0 - ts) ** (7 - i) * ts ** i for i in range(8)]
        Tp = [7 * math.comb(6, i) * (1.0 - ts) ** (6 - i) * ts ** i for i in range(7)]
    else:
        T = [ts ** i for i in range(8)]
        Tp = [(i + 1) * (ts ** i) for i in range(7)]
    return np.array(T).T, np.array(Tp).T


def ulp_distance(a, b):
    """distance in fp32 steps between two float32 arrays of one sign pattern (all tables are >= 0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("basis", _lib.BASIS)
@pytest.mark.parametrize("ts", [GRID, np.array([0.0, 1.0, 1 / 59 - 1e-9, 1 / 59 + 1e-9, 0.5, 0.123456789, 0.999])], ids=["grid", "irregular"])
def test_basis_tables_match_float64_restatement(basis, ts):
    T, Tp = _lib.curve_basis(basis, ts)
    T64, Tp64 = tables64(basis, ts)
    assert T.shape == (len(ts), 8) and Tp.shape == (len(ts), 7) and T.dtype == np.float32
    assert ulp_distance(T, T64.astype(np.float32)).max() <= 1
    assert ulp_distance(Tp, Tp64.astype(np.float32)).max() <= 1


def test_bezier_tables_on_the_grid_are_the_blobs(formula_sd):
    blob, entries = _lib.weight_image(formula_sd)
    ent = {k: (o, n) for k, o, n in entries}
    T, Tp = _lib.curve_basis("bezier", GRID)
    (oT, nT), (oP, nP) = ent["dec.T"], ent["dec.Tp"]
    assert (nT, nP) == (480, 420)
    assert np.array_equal(blob[oT:oT + nT].view(np.uint32), T.ravel().view(np.uint32))
    assert np.array_equal(blob[oP:oP + nP].view(np.uint32), Tp.ravel().view(np.uint32))


def test_basis_end_points():
    for basis in _lib.BASIS:
        T, _ = _lib.curve_basis(basis, [0.0])
        assert T[0].tolist() == [1.0] + [0.0] * 7, basis
    T, Tp = _lib.curve_basis("bezier", [1.0])
    assert T[0].tolist() == [0.0] * 7 + [1.0]
    assert Tp[0].tolist() == [0.0] * 6 + [7.0]
    T, Tp = _lib.curve_basis("monomial", [1.0])
    assert T[0].tolist() == [1.0] * 8 and Tp[0].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]


def test_basis_numbers_and_names():
    assert _lib.BASIS == ("bezier", "monomial")
    a, b = _lib.curve_basis(0, GRID), _lib.curve_basis("bezier", GRID)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = _lib.curve_basis(1, GRID), _lib.curve_basis("monomial", GRID)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(_lib.curve_basis(0, GRID)[0], _lib.curve_basis(1, GRID)[0])


def test_curve_basis_rejects_bad_arguments_by_name():
    lib = _lib.load()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    T, Tp = np.zeros((4, 8), np.float32), np.zeros((4, 7), np.float32)

    def call(basis, tau, n=None, T_=T, Tp_=Tp):
        tau = np.ascontiguousarray(tau, np.float64)
        return lib.mind_debug_curve_basis(basis, tau.ctypes.data_as(dp), len(tau) if n is None else n,
                                          T_.ctypes.data_as(fp) if T_ is not None else None, Tp_.ctypes.data_as(fp) if Tp_ is not None else None)

    assert call(0, [0.0, 0.5, 1.0]) == _lib.MIND_OK
    for bad in ([float("nan")], [float("inf")], [-float("inf")], [-1e-12], [1.0 + 1e-12], [0.5, 2.0]):
        for basis in (0, 1):
            assert call(basis, bad) == _lib.MIND_EINVAL, bad
    assert call(0, [0.5], n=0) == _lib.MIND_EINVAL
    assert call(0, [0.5], n=-3) == _lib.MIND_EINVAL
    assert call(2, [0.5]) == _lib.MIND_EINVAL and call(-1, [0.5]) == _lib.MIND_EINVAL
    assert call(0, [0.5], T_=None) == _lib.MIND_EINVAL and call(0, [0.5], Tp_=None) == _lib.MIND_EINVAL
    assert lib.mind_debug_curve_basis(0, None, 1, T.ctypes.data_as(fp), Tp.ctypes.data_as(fp)) == _lib.MIND_EINVAL
    with pytest.raises(ValueError):
        _lib.curve_basis("bezier", [1.5])


def test_context_entry_points_reject_a_null_context():
    lib = _lib.load()
    assert lib.mind_set_decoder_basis(None, 0) == _lib.MIND_EINVAL
    assert lib.mind_get_decoder_basis(None) == _lib.MIND_EINVAL
    assert lib.mind_predict_batch_aux(None, None, None, None) == _lib.MIND_EINVAL
    tau = (C.c_double * 1)(0.5)
    assert lib.mind_curve_eval(None, 0, None, 0, tau, 1, None, None, None) == _lib.MIND_EINVAL
    assert C.sizeof(_lib.PredAux) == 16 and C.sizeof(_lib.PredOut) == 48      # mind_pred_out keeps its layout


def test_default_weight_image_is_untouched_by_the_basis_code(formula_sd):
    """the image mind_debug_weight_image packs is the Bezier one whatever was evaluated before it (the setting lives in a context)"""
    _lib.curve_basis("monomial", GRID)
    blob, entries = _lib.weight_image(formula_sd)
    o, n = {k: (o, n) for k, o, n in entries}["dec.T"]
    assert np.array_equal(blob[o:o + n], tables64("bezier", GRID)[0].astype(np.float32).ravel()) or \
        ulp_distance(blob[o:o + n], tables64("bezier", GRID)[0].astype(np.float32).ravel()).max() <= 1


def test_scene_pred_net_reads_param_out_without_a_gpu():
    from mind_amd.planners.mind.networks.network import ScenePredNet
    assert ScenePredNet.want_aux is False and ScenePredNet.param_out == "bezier"
    assert ScenePredNet.check_param_out("bezier") == "bezier" and ScenePredNet.check_param_out("monomial") == "monomial"
    with pytest.raises(NotImplementedError, match=r"N_ORDER.*network\.py:537.*\[300,128\]"):
        ScenePredNet({"param_out": "none"})
    with pytest.raises(ValueError, match="param_out"):
        ScenePredNet({"param_out": "spline"})


IRREGULAR = np.array([0.0, 1.0, 1 / 59 - 1e-9, 1 / 59 + 1e-9, 0.5, 0.123456789, 0.999, 0.25, 0.75, 1 / 3, 2 / 3, 0.01, 0.99, 0.6180339887, 0.0001,
                      0.9999, 0.42])


@pytest.mark.parametrize("basis", _lib.BASIS)
def test_error_bound_holds_for_an_emulated_fp32_chain_on_the_fixture(basis):
    """The bound the GPU tests hold the kernels to (tests/decoder_aux_restate.py) is checked here against a numpy emulation of the device's
    fp32 chain on the fixture's control points: found 0.18-0.27 of the bound for every output, both bases, on the decoder's grid and on 17
    irregular times -- and the emulation reproduces the reference's float32 vel / cov_vel exactly and its reg to 2.4e-7."""
    import os
    from decoder_aux_restate import GRID as G, bound_violations, emulate_fp32
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_aux.npz"))
    keys = [k[:-len("_param")] for k in g.files if k.startswith(basis) and k.endswith("_param")]
    assert len(keys) == 3
    for ts in (G, IRREGULAR):
        T, Tp = _lib.curve_basis(basis, ts)
        for k in keys:
            reg, vel, cov_vel = emulate_fp32(g[k + "_param"], basis, T, Tp)
            worst = bound_violations(g[k + "_param"], basis, ts, reg, vel, cov_vel)
            print(basis, k, len(ts), worst)
            assert set(worst) == {"pos", "cov", "vel", "cov_vel"} and max(worst.values()) <= 1.0, (k, worst)
            if ts is G:
                assert np.abs(reg - g[k + "_reg"]).max() < 1e-6 and np.abs(vel - g[k + "_vel"]).max() < 1e-6
                assert np.abs(cov_vel - g[k + "_cov_vel"]).max() < 1e-6
