"""CPU: the launch list of the layer-wise batched ActorNet (mind_amd/csrc/actor_lw_kernels.hip) as mind_predict_batch issues it --
mind_debug_actor_lw_plan returns it without a GPU.  The 26 stages are k_actor_mfma's (res[0..7] with a downsample in 0, 2, 4, 6; the
laterals top-down; the output Res1d), every chunk of actors runs the input split and then conv + GroupNorm per stage, the chunks cover
every actor exactly once and the scratch arena is one chunk whatever the call's size."""
import ctypes as C

import numpy as np
import pytest

from mind_amd import _lib

REC = 16
DEFAULT_CHUNK = 1024

# (Cin, Cout, ksz, stride, Tin, Tout) of the 26 convolutions, in order (planners/mind/networks/network.py:20-61: ActorNet)
STAGES = [
    (14, 32, 3, 1, 48, 48), (14, 32, 1, 1, 48, 48), (32, 32, 3, 1, 48, 48),          # res[0]: conv1, downsample, conv2
    (32, 32, 3, 1, 48, 48), (32, 32, 3, 1, 48, 48),                                  # res[1]
    (32, 64, 3, 2, 48, 24), (32, 64, 1, 2, 48, 24), (64, 64, 3, 1, 24, 24),          # res[2]
    (64, 64, 3, 1, 24, 24), (64, 64, 3, 1, 24, 24),                                  # res[3]
    (64, 128, 3, 2, 24, 12), (64, 128, 1, 2, 24, 12), (128, 128, 3, 1, 12, 12),      # res[4]
    (128, 128, 3, 1, 12, 12), (128, 128, 3, 1, 12, 12),                              # res[5]
    (128, 256, 3, 2, 12, 6), (128, 256, 1, 2, 12, 6), (256, 256, 3, 1, 6, 6),        # res[6]
    (256, 256, 3, 1, 6, 6), (256, 256, 3, 1, 6, 6),                                  # res[7]
    (256, 128, 3, 1, 6, 6), (128, 128, 3, 1, 12, 12), (64, 128, 3, 1, 24, 24), (32, 128, 3, 1, 48, 48),   # lateral[3..0]
    (128, 128, 3, 1, 48, 48), (128, 128, 3, 1, 48, 48),                              # output Res1d
]


def plan(n_actors, np_=6, chunk=0):
    lib = _lib.load()
    info = np.zeros(3, np.int64)
    n = lib.mind_debug_actor_lw_plan(n_actors, np_, chunk, None, 0, info.ctypes.data_as(C.POINTER(C.c_longlong)))
    assert n > 0 and n == info[2]
    out = np.zeros((n, REC), np.int64)
    assert lib.mind_debug_actor_lw_plan(n_actors, np_, chunk, out.ctypes.data_as(C.POINTER(C.c_longlong)), n,
                                        info.ctypes.data_as(C.POINTER(C.c_longlong))) == n
    return out, info


def test_the_26_stages_and_their_shapes():
    out, info = plan(64)
    assert info[0] == DEFAULT_CHUNK and len(out) == 1 + 2 * 26
    assert tuple(out[0, :2]) == (-1, 0)                                   # the input split first
    convs, gns = out[1::2], out[2::2]
    assert (convs[:, 1] == 1).all() and (gns[:, 1] == 2).all()
    assert list(convs[:, 0]) == list(range(26)) and list(gns[:, 0]) == list(range(26))     # conv s, then its GroupNorm
    assert [tuple(r[8:14]) for r in convs] == STAGES and [tuple(r[8:14]) for r in gns] == STAGES
    assert list(gns[:, 15]) == [0] * 25 + [1]                             # only the last stage writes actor_feat


@pytest.mark.parametrize("np_", [6, 3, 1])
def test_grids_cover_every_output_and_the_lds_fits(np_):
    out, _ = plan(1000, np_)
    for r in out:
        stage, kind, gx, gy, block, lds, a0, n = r[:8]
        cin, cout, ksz, stride, tin, tout = r[8:14]
        assert gx >= 1 and gy >= 1 and block <= 1024 and lds <= 160 * 1024
        if kind == 1:
            cp = 16
            while cp < cin:
                cp *= 2
            ksteps = (ksz * cp + 31) // 32
            mt = 4 if cout >= 128 and 4 <= ksteps <= 12 else 2                  # 16-channel m-tiles per workgroup: four where they fit in LDS
            assert gy * mt * 16 == cout
            assert lds == mt * ksteps * 3 * 1024 and r[14] == lds // 3 * {6: 3, 3: 2, 1: 1}[np_]
            assert gx * (block // 64) <= (n * tout + 15) // 16 + block // 64          # no workgroup without a tile
        elif kind == 2:
            assert gx == n and block == 1024 and (cout // 16) * ((tout + 15) // 16) <= 2 * 16     # one actor per workgroup, <= 2 tiles per wave
        else:
            assert gx == n


@pytest.mark.parametrize("A", [1, 63, 64, DEFAULT_CHUNK - 1, DEFAULT_CHUNK, DEFAULT_CHUNK + 1, 13824])
def test_chunks_cover_every_actor_exactly_once(A):
    out, info = plan(A)
    n_chunks = (A + DEFAULT_CHUNK - 1) // DEFAULT_CHUNK
    assert len(out) == n_chunks * 53 == info[2]
    for kind, stage in [(0, -1)] + [(k, s) for s in range(26) for k in (1, 2)]:
        rows = out[(out[:, 1] == kind) & (out[:, 0] == stage)]
        assert len(rows) == n_chunks
        seen = np.zeros(A, int)
        for r in rows:
            assert 0 < r[7] <= DEFAULT_CHUNK
            seen[r[6]:r[6] + r[7]] += 1
        assert (seen == 1).all()
    # a chunk is finished before the next one starts (they share the arena)
    firsts = out[:, 6]
    assert (np.diff(firsts) >= 0).all()


def test_small_chunk_knob_and_ragged_last_chunk():
    out, info = plan(300, 6, 96)
    assert info[0] == 96 and len(out) == 4 * 53
    assert sorted(set(zip(out[:, 6], out[:, 7]))) == [(0, 96), (96, 96), (192, 96), (288, 12)]


def test_the_arena_does_not_grow_with_the_call():
    _, i1 = plan(DEFAULT_CHUNK)
    _, i2 = plan(13824)
    _, i3 = plan(1)
    assert i1[1] == i2[1] == i3[1] == DEFAULT_CHUNK * 137472
    assert i1[1] + 10 * (1 << 20) < 256 * (1 << 20)                        # with the 9.1 MB of fragments inside the 256 MiB Infinity Cache


@pytest.mark.parametrize("np_", [0, 2, 4, 5, 7, -1])
def test_unknown_arithmetic_is_einval(np_):
    lib = _lib.load()
    info = np.zeros(3, np.int64)
    assert lib.mind_debug_actor_lw_plan(64, np_, 0, None, 0, info.ctypes.data_as(C.POINTER(C.c_longlong))) == _lib.MIND_EINVAL
    assert lib.mind_debug_actor_lw_plan(0, 6, 0, None, 0, info.ctypes.data_as(C.POINTER(C.c_longlong))) == _lib.MIND_EINVAL
