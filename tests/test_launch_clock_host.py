"""CPU: the launch clock's ring bookkeeping and reduction (mind_amd/csrc/launch_clock.h) through mind_debug_launch_clock -- the reduction over
a launch's slots, the ring's wrap with pending blocks, a read that drains nothing, a grid that outgrows its block, the tick -> ms conversion."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mind_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAKE, RUNS, DRAIN, FITS, GROW, REDUCE, MARK, COPIED = range(8)
PAIR, ACTOR, ILQR = 0, 1, 2


def run(n_blocks, block_slots, ops, stamps=None, rate_khz=100000):
    """-> [n_ops, 8] doubles: results [0..4], pending records, head block, launches dropped"""
    lib = _lib.load()
    o = np.ascontiguousarray([list(op) + [0] * (4 - len(op)) for op in ops], np.int64)
    st = np.ascontiguousarray(stamps if stamps is not None else np.zeros((0, 2)), np.uint64).reshape(-1, 2)
    out = np.zeros((len(ops), 8))
    rc = lib.mind_debug_launch_clock(n_blocks, block_slots, rate_khz, o.ctypes.data_as(C.POINTER(C.c_longlong)), len(ops),
                                     st.ctypes.data_as(C.POINTER(C.c_ulonglong)), st.shape[0], out.ctypes.data_as(C.POINTER(C.c_double)), out.size)
    assert rc == out.size, rc
    return out


def test_declared_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mind_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in (("mind_debug_launch_clock", 9), ("mind_debug_launch_times", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, re.S)
        assert m, f"{name} is not declared in include/mind_hip.h"
        fn = getattr(lib, name)
        assert len(m.group(1).split(",")) == len(fn.argtypes) == n_args and name in _lib.EXPORTS


def test_reduce_single_workgroup():
    st = np.zeros((4, 2), np.uint64)
    st[0] = (1000, 1750)
    out = run(1, 4, [(TAKE, 1, PAIR), (REDUCE, 0, 1)], st)
    assert out[1, 0] == 750 and out[1, 1] == pytest.approx(0.0075, rel=1e-12)      # 750 ticks of 10 ns


def test_reduce_unordered_stamps():
    """first workgroup in to last workgroup out, whatever the order of the slots; workgroups that did not overlap at all; a workgroup that left
    at once (t0 == t1)"""
    base = 123_456_789_000_000                                                     # (an uptime of two weeks at 100 MHz: exact in a double)
    st = np.array([(base + 900, base + 1400), (base + 100, base + 300), (base + 5000, base + 5000), (base + 350, base + 4000)], np.uint64)
    out = run(2, 4, [(REDUCE, 0, 4), (REDUCE, 0, 2), (REDUCE, 0, 0)], st)
    assert out[0, 0] == 4900 and out[1, 0] == 1300 and out[2, 0] == 0
    # stamps that run backwards (a slot never written by this launch, stale t1): 0, not a wrapped difference
    back = np.array([(2000, 10)], np.uint64)
    assert run(1, 1, [(REDUCE, 0, 1)], back)[0, 0] == 0


def test_reduce_block_larger_than_grid():
    """only the grid's slots count: the rest of the block holds an earlier, larger launch's stamps (slots are never reset)"""
    st = np.zeros((16, 2), np.uint64)
    st[8:16] = [(10_000 + 10 * i, 90_000 + i) for i in range(8)]                    # block 1: stale stamps of an 8-workgroup launch ...
    st[8:11] = [(500_000, 500_900), (500_010, 500_700), (500_020, 501_000)]         # ... overwritten by a 3-workgroup one
    out = run(2, 8, [(REDUCE, 1, 3), (REDUCE, 1, 8)], st)
    assert out[0, 0] == 1000
    assert out[1, 0] == 501_000 - 10_030                                            # (what a reader that took the whole block would get)
    # a reduce that reaches past the mirror is refused
    lib = _lib.load()
    o = np.array([[REDUCE, 1, 9, 0]], np.int64)
    res = np.zeros(8)
    rc = lib.mind_debug_launch_clock(2, 8, 100000, o.ctypes.data_as(C.POINTER(C.c_longlong)), 1, st.ctypes.data_as(C.POINTER(C.c_ulonglong)), 16,
                                     res.ctypes.data_as(C.POINTER(C.c_double)), 8)
    assert rc < 0


def test_ring_wrap_with_pending_blocks():
    ops = [(TAKE, 5, PAIR)] * 3 + [(DRAIN, 2)] + [(TAKE, 7, PAIR)] * 3 + [(RUNS, 0, 4), (RUNS, 1, 2), (RUNS, 3, 1), (TAKE, 1, ILQR), (DRAIN, 4), (TAKE, 1, ILQR), (RUNS, 0, 1)]
    out = run(4, 8, ops)
    assert list(out[0:3, 0]) == [0, 1, 2] and list(out[0:3, 5]) == [1, 2, 3]
    assert out[3, 5] == 1 and out[3, 6] == 3                                        # two drained: one pending, the head where it was
    assert list(out[4:7, 0]) == [3, 0, 1] and out[6, 5] == 4 and out[6, 6] == 2     # the ring wrapped onto the drained blocks
    assert list(out[7, 0:5]) == [2, 2, 2, 0, 2]                                     # pending blocks 2, 3, 0, 1 = runs [2, 4) and [0, 2)
    assert list(out[8, 0:5]) == [2, 3, 1, 0, 1]                                     # records 1, 2 = blocks 3, 0
    assert list(out[9, 0:5]) == [1, 1, 1, 0, 0]                                     # record 3 = block 1
    assert out[10, 0] == -1 and out[10, 7] == 1 and out[10, 5] == 4                 # every block pending: no block, nothing overwritten, one launch dropped
    assert out[11, 5] == 0 and out[11, 6] == 2
    assert out[12, 0] == 2 and list(out[13, 0:3]) == [1, 2, 1]


def test_read_that_drains_nothing():
    out = run(4, 8, [(RUNS, 0, 0), (DRAIN, 0), (DRAIN, 3), (RUNS, 0, 1), (COPIED, 0), (COPIED, 1), (TAKE, 2, ACTOR), (DRAIN, 0), (RUNS, 0, 1)])
    assert out[0, 0] == 0 and out[3, 0] == 0                                        # no runs of an empty ring, nor of a record that is not there
    assert all(out[k, 5] == 0 and out[k, 6] == 0 and out[k, 7] == 0 for k in range(6))
    assert out[4, 0] == 1 and out[5, 0] == 0                                        # "the oldest 0 records have their copy": yes; the oldest 1 of none: no
    assert out[6, 0] == 0 and out[7, 5] == 1 and list(out[8, 0:3]) == [1, 0, 1]     # a drain of nothing leaves the pending record alone


def test_copy_marks():
    out = run(4, 8, [(TAKE, 1, PAIR)] * 3 + [(COPIED, 1), (MARK, 1, 2), (COPIED, 1), (COPIED, 3), (MARK, 0, 1), (COPIED, 3), (DRAIN, 3), (TAKE, 1, PAIR), (COPIED, 1)])
    assert out[3, 0] == 0 and out[5, 0] == 0 and out[6, 0] == 0                     # records 1, 2 marked: the oldest one is not
    assert out[8, 0] == 1                                                           # all three
    assert out[11, 0] == 0                                                          # a new record starts unmarked


def test_grid_outgrows_block_and_growth():
    out = run(4, 64, [(FITS, 12, 64), (FITS, 4, 65), (FITS, 4, 64), (TAKE, 65, PAIR), (TAKE, 64, PAIR), (FITS, 4, 64), (GROW, 12, 200), (FITS, 12, 200), (TAKE, 200, PAIR),
                      (TAKE, 257, PAIR), (GROW, 3, 10)])
    assert list(out[0:3, 0]) == [0, 0, 1]
    assert out[3, 0] == -1 and out[3, 7] == 1 and out[3, 5] == 0                    # the launch runs untimed: no block, no record
    assert out[4, 0] == 0 and out[5, 0] == 0                                        # (one block taken: four more do not fit)
    assert list(out[6, 0:2]) == [16, 256]                                           # blocks double until the records fit, slots round up to 64
    assert out[6, 5] == 0 and out[6, 6] == 0 and out[7, 0] == 1 and out[8, 0] == 0
    assert out[9, 0] == -1
    assert list(out[10, 0:2]) == [16, 256]                                          # never smaller than it is
    # a ring that was never allocated hands out nothing, and grows to its first geometry
    out = run(0, 0, [(TAKE, 1, PAIR), (FITS, 1, 1), (GROW, 13, 256)])
    assert out[0, 0] == -1 and out[1, 0] == 0 and list(out[2, 0:2]) == [32, 256]


@pytest.mark.parametrize("rate_khz,ticks,ms", [(100000, 3_400, 0.034), (100000, 107_600, 1.076), (25000, 3_400, 0.136), (1_000_000, 1, 1e-6)])
def test_rate_conversion(rate_khz, ticks, ms):
    st = np.array([(7, 7 + ticks)], np.uint64)
    out = run(1, 1, [(REDUCE, 0, 1)], st, rate_khz=rate_khz)
    assert out[0, 0] == ticks and out[0, 1] == pytest.approx(ms, rel=1e-12)


def test_no_rate_no_time():
    st = np.array([(7, 1007)], np.uint64)
    assert run(1, 1, [(REDUCE, 0, 1)], st, rate_khz=0)[0, 1] == 0.0
