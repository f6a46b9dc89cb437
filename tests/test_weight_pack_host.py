"""CPU checks of the weight path (mind_amd/csrc/weight_pack.h) -- no GPU needed.

The packed blob of two formula state_dicts must equal, entry by entry (key, offset, length, SHA-256 of the bytes), the blob the commit before
the packer moved into its header produced (tests/golden/weight_blob_parent.json): the device layout did not move.  Every packer that had no
host test is checked against a numpy restatement of the layout formula in its comment, at the strides and start offsets wp_pack uses.  The
binder must name a missing required entry and accept the absence of the optional ones."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from mind_amd import _lib
from mind_amd.weights import formula_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weight_blob_parent.json")
LANE = np.arange(64)
R, Q = LANE & 15, LANE >> 4


@pytest.fixture(scope="module")
def sd():
    return formula_state_dict(20240121)


@pytest.fixture(scope="module")
def image(sd):
    blob, entries = _lib.weight_image(sd)
    return blob, {k: blob[o:o + n] for k, o, n in entries}


def bf16_rne(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def halves(dwords):
    """uint32 [...] -> float32 [..., 2]: the bf16 values in bits 0..15 and 16..31"""
    d = np.ascontiguousarray(dwords, np.uint32)
    return np.stack([(d << 16).view(np.float32), (d & 0xffff0000).view(np.float32)], -1)


def block(rng, stride, col0):
    """a random [128][stride] matrix, the flat array from its column col0 on (what the loader hands a packer), the [128][128] block there"""
    W = rng.standard_normal((128, stride)).astype(np.float32)
    return W.ravel()[col0:], W[:, col0:col0 + 128]


# ---- the blob did not move
@pytest.mark.parametrize("seed", [20240121, 7])
def test_blob_equals_the_parent_commits(seed):
    want = json.load(open(GOLDEN))[str(seed)]
    blob, entries = _lib.weight_image(formula_state_dict(seed))
    assert blob.size == want["floats"] and len(entries) == len(want["entries"])
    for (k, o, n), (wk, wo, wn, wsha) in zip(entries, want["entries"]):
        assert (k, o, n) == (wk, wo, wn)
        assert o % 64 == 0
        assert hashlib.sha256(blob[o:o + n].tobytes()).hexdigest() == wsha, k


# ---- packers
@pytest.mark.parametrize("stride,col0", [(128, 0), (256, 0), (256, 128), (384, 0), (384, 128), (384, 256)])
def test_pack_afrag(stride, col0):
    """[ob 8][s4 8][lane 64][w 4] = W[16 ob + (lane & 15)][16 s4 + 4 (lane >> 4) + w]"""
    flat, W = block(np.random.default_rng(stride + col0), stride, col0)
    got = _lib.pack("afrag", flat, stride).reshape(8, 8, 64, 4)
    ob, s4, w = np.arange(8)[:, None, None, None], np.arange(8)[None, :, None, None], np.arange(4)[None, None, None, :]
    want = W[16 * ob + R[None, None, :, None], 16 * s4 + 4 * Q[None, None, :, None] + w]
    assert np.array_equal(got, want)


def test_pack_wk_frag():
    """[hd 8][ob 8][lane 64][w 4] = Wk[16 hd + 4 (lane >> 4) + w][16 ob + (lane & 15)]"""
    Wk = np.random.default_rng(1).standard_normal((128, 128)).astype(np.float32)
    got = _lib.pack("wk_frag", Wk).reshape(8, 8, 64, 4)
    hd, ob, w = np.arange(8)[:, None, None, None], np.arange(8)[None, :, None, None], np.arange(4)[None, None, None, :]
    want = Wk[16 * hd + 4 * Q[None, None, :, None] + w, 16 * ob + R[None, None, :, None]]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("stride,col0", [(128, 0), (256, 0), (256, 128), (384, 128), (384, 256)])
def test_pack_tok_bfrag(stride, col0):
    """[ob 8][part * 4 + g][lane 64][dword 4]: dword d packs W[16 ob + r][32 g + 8 q + 2 d (+ 1)], hi part then lo part of the bf16 two-way
    split x ~ hi + lo (hi = rne(x), lo = rne(x - hi))"""
    flat, W = block(np.random.default_rng(stride + col0 + 1), stride, col0)
    got = halves(_lib.pack("tok_bfrag", flat, stride).view(np.uint32).reshape(8, 2, 4, 64, 4))      # [ob][part][g][lane][d][e]
    ob, g = np.arange(8)[:, None, None, None, None], np.arange(4)[None, :, None, None, None]
    d, e = np.arange(4)[None, None, None, :, None], np.arange(2)[None, None, None, None, :]
    x = W[16 * ob + R[None, None, :, None, None], 32 * g + 8 * Q[None, None, :, None, None] + 2 * d + e]
    hi = bf16_rne(x)
    assert np.array_equal(got[:, 0], hi) and np.array_equal(got[:, 1], bf16_rne(x - hi))


@pytest.mark.parametrize("stride", [128, 384])
def test_pack_bfrag_lo3_completes_the_exact_split(stride):
    """[ob 8][g 4][lane 64][dword 4], k-slot (q, i = 2 d + e) <-> feature 16 (2 g + (i >> 2)) + 4 q + (i & 3): the third bf16 part; with
    pack_bfrag's hi and lo (= mid) parts, hi + mid + lo == w exactly in fp32"""
    W = np.random.default_rng(stride).standard_normal((128, stride)).astype(np.float32)
    lo = halves(_lib.pack("bfrag_lo3", W, stride).view(np.uint32).reshape(8, 4, 64, 4))             # [ob][g][lane][d][e]
    two = np.zeros(16384, np.uint32)
    import ctypes as C
    assert _lib.load().mind_debug_pack_bfrag(W.ctypes.data_as(C.POINTER(C.c_float)), stride, two.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    hi, mid = halves(two.reshape(2, 8, 4, 64, 4))
    ob, g = np.arange(8)[:, None, None, None, None], np.arange(4)[None, :, None, None, None]
    i = 2 * np.arange(4)[None, None, None, :, None] + np.arange(2)[None, None, None, None, :]
    x = W[16 * ob + R[None, None, :, None, None], 16 * (2 * g + (i >> 2)) + 4 * Q[None, None, :, None, None] + (i & 3)]
    r1 = x - bf16_rne(x)
    assert np.array_equal(lo, bf16_rne(r1 - bf16_rne(r1)))
    assert np.array_equal((hi.astype(np.float64) + mid + lo).astype(np.float32), x)


@pytest.mark.parametrize("co,ci,ksz", [(32, 14, 3), (64, 32, 1), (256, 128, 3)])
def test_pack_conv_f32(co, ci, ksz):
    """[m-tile co/16][k-group of 16][lane 64][4] = w[16 mt + r][ci][dk], k = 16 g + 4 q + m = dk * ci_pad + ci (zeros beyond ci).  The first
    conv of the net (14 -> 32 channels: ci padded to 16), a downsample (32 -> 64, one tap), the widest conv (128 -> 256)."""
    w = np.random.default_rng(co + ci).standard_normal((co, ci, ksz)).astype(np.float32)
    cp = 16
    while cp < ci:
        cp *= 2
    G = ksz * cp // 16
    got = _lib.pack("conv_f32", w, co, ci, ksz).reshape(co // 16, G, 64, 4)
    wp = np.zeros((co, cp, ksz), np.float32)
    wp[:, :ci] = w
    k = 16 * np.arange(G)[None, :, None, None] + 4 * Q[None, None, :, None] + np.arange(4)[None, None, None, :]
    want = wp[16 * np.arange(co // 16)[:, None, None, None] + R[None, None, :, None], k % cp, k // cp]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n_in", [128, 384])
def test_center_outputs_folds_the_layernorm_mean(n_in):
    rng = np.random.default_rng(n_in)
    W, b = rng.standard_normal((128, n_in)).astype(np.float32), rng.standard_normal(128).astype(np.float32)
    out = _lib.pack("center_outputs", np.concatenate([W.ravel(), b]), 128, n_in)
    Wc, bc = out[:128 * n_in].reshape(128, n_in).astype(np.float64), out[128 * n_in:].astype(np.float64)
    assert out.size == 128 * n_in + 128
    assert np.abs(Wc.mean(0)).max() < 1e-6 and abs(bc.mean()) < 1e-6

    def ln(y):
        return (y - y.mean()) / np.sqrt(y.var() + 1e-5)
    x = rng.standard_normal(n_in)
    assert np.abs(ln(Wc @ x + bc) - ln(W.astype(np.float64) @ x + b)).max() < 1e-5


def test_rpe_table_and_vtab_slots(sd, image):
    """fus.rtab [32 chunks][8][4]: rows 0..4 W_r[f][k], 5 bias, 6 gamma, 7 beta of feature f = 4 chunk + w; fus.L*.vtab: seven 128-vectors
    gamma_m, beta_m, b_p (centred), gamma_p, beta_p, gamma_e, beta_e -- the last five zero in the last layer, which has no proj_edge"""
    _, ent = image
    t = ent["fus.rtab"].reshape(32, 8, 4)
    p = "fusion_net.proj_rpe_scene."
    assert np.array_equal(t[:, :5].transpose(0, 2, 1).reshape(128, 5), sd[p + "0.weight"])
    for row, key in ((5, "0.bias"), (6, "1.weight"), (7, "1.bias")):
        assert np.array_equal(t[:, row].ravel(), sd[p + key])
    for L in range(6):
        vt = ent[f"fus.L{L}.vtab"].reshape(7, 128)
        p = f"fusion_net.fuse_scene.fusion.{L}."
        assert np.array_equal(vt[0], sd[p + "proj_memory.1.weight"]) and np.array_equal(vt[1], sd[p + "proj_memory.1.bias"])
        if L == 5:
            assert not vt[2:].any()
            continue
        bp = sd[p + "proj_edge.0.bias"].astype(np.float64)
        assert np.abs(vt[2] - (bp - bp.mean())).max() < 1e-6
        for row, key in ((3, "proj_edge.1.weight"), (4, "proj_edge.1.bias"), (5, "norm_edge.weight"), (6, "norm_edge.bias")):
            assert np.array_equal(vt[row], sd[p + key])


def test_bezier_basis(image):
    """dec.T [60][8], dec.Tp [60][7]: Bernstein bases of degree 7 and (times 7) degree 6 on linspace(0, 1, 60), float64 rounded to fp32"""
    from math import comb
    _, ent = image
    ts = np.linspace(0.0, 1.0, 60)[:, None]
    for key, n, scale in (("dec.T", 7, 1.0), ("dec.Tp", 6, 7.0)):
        i = np.arange(n + 1)[None, :]
        want = scale * np.array([comb(n, k) for k in range(n + 1)])[None, :] * (1.0 - ts) ** (n - i) * ts ** i
        # one fp32 ulp (2^-23 relative): half an ulp of rounding, and the rounding may flip where the two pow() differ in their last float64 bit
        assert (np.abs(ent[key].reshape(60, n + 1) - want) <= 2.0 ** -23 * np.abs(want)).all()


# ---- binder
def test_full_blob_binds_without_the_optional_entries(sd, image):
    _, ent = image
    assert "fus.L5.WAp" not in ent and "act.r1.ds" not in ent and "act.r8.dsB" not in ent
    assert "fus.L4.WAp" in ent and "act.r0.ds" in ent
    assert _lib.weight_bind(sd) is None


@pytest.mark.parametrize("key", ["fus.L3.WqM", "dec.reg6.bB", "act.lat2.WF", "act.r2.dsB", "fus.L4.WLp"])
def test_bind_names_the_missing_entry(sd, key):
    assert _lib.weight_bind(sd, drop=key) == key


def test_pack_names_the_missing_tensor(sd):
    name = "fusion_net.proj_rpe_scene.1.bias"
    bad = {k: v for k, v in sd.items() if k != name}
    assert len(bad) == len(sd) - 1
    assert _lib.weight_bind(bad) == name
    with pytest.raises(KeyError, match=name):
        _lib.weight_image(bad)
    short = dict(sd)
    short[name] = sd[name][:-1]
    assert _lib.weight_bind(short) == name
