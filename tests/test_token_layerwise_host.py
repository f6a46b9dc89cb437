"""CPU: the launch list of the layer-wise token stage (mind_amd/csrc/token_lw_kernels.hip) as mind_predict_batch issues it for one token
step -- mind_debug_token_lw_plan returns it without a GPU.  A step's mode picks the stages (init: 0, 5, 6; behind fusion layers 0-4:
1..6; behind the last layer: 1..4), every chunk of tokens runs them in order, the chunks cover every token exactly once per stage and
the arena is one chunk whatever the call's size."""
import ctypes as C

import numpy as np
import pytest

from mind_amd import _lib

REC = 8
DEFAULT_CHUNK = 32768
ARENA_PER_TOKEN = 640 * 4         # o 128 | x1 128 | h 256 | q 128 floats
INIT, MID, LAST = 1 | 4, 2 | 4, 2 | 8
STAGES = {INIT: [0, 5, 6], MID: [1, 2, 3, 4, 5, 6], LAST: [1, 2, 3, 4]}
GRID_Y = {0: 1, 1: 1, 2: 1, 3: 2, 4: 1, 5: 3, 6: 1}       # FFN 1: the two output halves; S / T / q: the three matrices
LLP = C.POINTER(C.c_longlong)


def plan(n_tokens, mode, chunk=0):
    lib = _lib.load()
    info = np.zeros(4, np.int64)
    n = lib.mind_debug_token_lw_plan(n_tokens, mode, chunk, None, 0, info.ctypes.data_as(LLP))
    assert n > 0 and n == info[2]
    out = np.zeros((n, REC), np.int64)
    assert lib.mind_debug_token_lw_plan(n_tokens, mode, chunk, out.ctypes.data_as(LLP), n, info.ctypes.data_as(LLP)) == n
    return out, info


@pytest.mark.parametrize("qbits", [0, 16, 48])
@pytest.mark.parametrize("mode", [INIT, MID, LAST])
def test_the_stage_list_of_each_mode_set(mode, qbits):
    out, info = plan(321, mode | qbits)
    assert info[0] == DEFAULT_CHUNK and info[3] == 1
    assert list(out[:, 0]) == STAGES[mode]
    for stage, gx, gy, block, lds, t0, n, tiles in out:
        assert (t0, n, tiles) == (0, 321, 21) and block == 256
        assert gy == GRID_Y[stage] and 1 <= gx <= tiles            # no workgroup without a tile
        assert lds <= 32 * 1024                                    # several workgroups per CU


# (n_tokens, chunk): one tile, a ragged tile, less than a tile, several chunks with a ragged last one (whole and ragged tiles inside)
CASES = [(16, 0), (31, 0), (8, 0), (155, 48), (155, 50), (1000, 96), (70000, 0), (DEFAULT_CHUNK + 1, 0), (100, 7)]


@pytest.mark.parametrize("mode", [INIT | 48, MID | 16, LAST])
@pytest.mark.parametrize("n_tokens,chunk", CASES)
def test_launches_tile_the_tokens_exactly_once_per_stage(n_tokens, chunk, mode):
    out, info = plan(n_tokens, mode, chunk)
    ch = chunk or DEFAULT_CHUNK
    n_chunks = (n_tokens + ch - 1) // ch
    stages = STAGES[mode & 15]
    assert info[0] == ch and info[3] == n_chunks and len(out) == n_chunks * len(stages)
    for s in stages:
        rows = out[out[:, 0] == s]
        assert len(rows) == n_chunks
        seen = np.zeros(n_tokens, int)
        for r in rows:
            assert 0 < r[6] <= ch and r[7] == (r[6] + 15) // 16 and 1 <= r[1] <= r[7]
            seen[r[5]:r[5] + r[6]] += 1
        assert (seen == 1).all()
    # a chunk runs all its stages, in order, before the next one starts (they share the arena)
    assert (np.diff(out[:, 5]) >= 0).all()
    for c in range(n_chunks):
        assert list(out[c * len(stages):(c + 1) * len(stages), 0]) == stages


def test_big_launches_are_sized_from_the_cu_count_not_from_the_tokens():
    out, _ = plan(70000, MID | 48)
    first = out[:6]
    assert (first[:, 7] == DEFAULT_CHUNK // 16).all()
    assert (first[:, 1] * first[:, 2] <= 4 * 256).all() and (first[:, 1] * first[:, 2] >= 256).all()     # 1 - 4 workgroups per CU, each sweeps tiles


def test_small_chunk_knob_and_ragged_last_chunk():
    out, info = plan(155, MID | 48, 48)
    assert info[0] == 48 and info[3] == 4 and len(out) == 4 * 6
    assert sorted(set(zip(out[:, 5], out[:, 6]))) == [(0, 48), (48, 48), (96, 48), (144, 11)]


def test_the_arena_depends_on_the_chunk_only():
    sizes = {plan(n, m)[1][1] for n in (1, 321, 70000) for m in (INIT, MID | 16, LAST | 48)}
    assert sizes == {DEFAULT_CHUNK * ARENA_PER_TOKEN}
    assert {plan(n, MID, 48)[1][1] for n in (5, 155, 9999)} == {48 * ARENA_PER_TOKEN}
    assert DEFAULT_CHUNK * ARENA_PER_TOKEN < 128 * (1 << 20)                # well inside the 256 MiB Infinity Cache


@pytest.mark.parametrize("n_tokens,mode,chunk,cap", [
    (0, MID, 0, 0), (-5, MID, 0, 0), (100, MID, -1, 0), (100, MID, 0, -1),
    (100, 0, 0, 0), (100, 4, 0, 0), (100, 1, 0, 0), (100, 2, 0, 0), (100, 1 | 2 | 4, 0, 0), (100, 1 | 8, 0, 0), (100, 2 | 4 | 8, 0, 0),
    (100, MID | 32, 0, 0), (100, MID | 64, 0, 0), (100, MID, 0, 4)])           # (the last: cap > 0 without a buffer)
def test_bad_arguments_are_einval(n_tokens, mode, chunk, cap):
    lib = _lib.load()
    info = np.zeros(4, np.int64)
    assert lib.mind_debug_token_lw_plan(n_tokens, mode, chunk, None, cap, info.ctypes.data_as(LLP)) == _lib.MIND_EINVAL


def test_the_stats_entry_points_refuse_a_null_context():
    lib = _lib.load()
    assert lib.mind_last_token_stats(None, None, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_last_token_stage_ms(None, None, 0) == _lib.MIND_EINVAL
