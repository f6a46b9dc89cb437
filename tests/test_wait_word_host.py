"""CPU: the bounded wait of mind_aime_plan's polled decisions (pl_wait_word, mind_amd/csrc/aime_book.h, through mind_debug_wait_word) over a
word and a clock of the test's own: the clock is a callback that counts its calls and advances 10 ms per look, so "late" and "never" are
numbers of looks and no test waits for real time.  The plan's caller falls back to hipStreamSynchronize when the wait returns 0."""
import ctypes as C

from mind_amd import _lib

STEP = 0.01          # seconds per look of the scripted clock
TIMEOUT = 0.25       # the plan's own bound
SPINS = 4            # misses between two looks at the clock


def _wait(word, want, on_look=None, timeout=TIMEOUT, spins=SPINS):
    lib = _lib.load()
    looks, now = [0], [100.0]

    def clock(_user):
        looks[0] += 1
        now[0] += STEP
        if on_look:
            on_look(looks[0])
        return now[0]

    cb = _lib.WAIT_CLOCK(clock)
    return lib.mind_debug_wait_word(C.byref(word), want, timeout, cb, None, spins), looks[0]


def test_a_word_that_never_changes_times_out():
    word = C.c_uint(0)
    rc, looks = _wait(word, 7)
    # the first look is the start; the wait gives up at the first look more than 0.25 s later: 25 steps of 10 ms reach it, the sum's rounding decides 26 or 27 looks
    assert rc == 0 and looks in (26, 27), (rc, looks)
    assert word.value == 0


def test_a_stale_generation_is_not_taken_for_the_new_one():
    word = C.c_uint(6)
    rc, looks = _wait(word, 7)
    assert rc == 0 and looks in (26, 27), (rc, looks)


def test_a_word_that_changes_late_is_seen():
    word = C.c_uint(0)

    def late(look):
        if look == 20:
            word.value = 7

    rc, looks = _wait(word, 7, late)
    assert rc == 1 and looks == 20, (rc, looks)


def test_a_word_that_is_already_there_needs_no_clock():
    word = C.c_uint(7)
    rc, looks = _wait(word, 7)
    assert rc == 1 and looks == 0


def test_a_word_that_arrives_after_the_bound_is_left_to_the_fallback():
    word = C.c_uint(0)

    def too_late(look):
        if look == 40:
            word.value = 7

    rc, looks = _wait(word, 7, too_late)
    assert rc == 0 and looks < 40


def test_zero_timeout_looks_once_more_and_gives_up():
    word = C.c_uint(0)
    rc, looks = _wait(word, 7, timeout=0.0)
    assert rc == 0 and looks == 2


def test_the_steady_clock_and_bad_arguments():
    lib = _lib.load()
    word = C.c_uint(3)
    none = C.cast(None, _lib.WAIT_CLOCK)
    assert lib.mind_debug_wait_word(C.byref(word), 3, 0.25, none, None, 1024) == 1
    assert lib.mind_debug_wait_word(C.byref(word), 4, 0.0, none, None, 1) == 0
    assert lib.mind_debug_wait_word(None, 3, 0.25, none, None, 1024) == _lib.MIND_EINVAL
    assert lib.mind_debug_wait_word(C.byref(word), 3, -1.0, none, None, 1024) == _lib.MIND_EINVAL
    assert lib.mind_debug_wait_word(C.byref(word), 3, 0.25, none, None, 0) == _lib.MIND_EINVAL
