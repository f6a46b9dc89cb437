"""GPU: the knob table and the context's owners with a context (tests/tuning_worker.py, a child process per test: the variables are read at
context creation, and the handle count is the process's).  What a knob must store comes from the CPU debug entry (mind_debug_tuning), which
tests/test_tuning_host.py pins to the restated rules."""
import json
import os
import subprocess
import sys

import pytest

from mind_amd import _lib
from test_tuning_host import RULES, TEXTS, restated_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _worker(mode, *args, env=None):
    base = {k: v for k, v in os.environ.items() if not k.startswith("MIND_") or k == "MIND_HIP_LIB"}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tuning_worker.py"), mode, *args], env=dict(base, **(env or {})),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_every_knob_reaches_its_field():
    # per variable the first of the pinned texts that does not leave the default in place
    texts = {}
    for name, env, default, _, _ in RULES:
        if env is not None:
            texts[name] = next(s for s in TEXTS if restated_text(name, s) != default)
    env = {e: texts[n] for n, e, _, _, _ in RULES if e is not None}
    env["MIND_PAIR_PREC"] = "bf16"
    assert len(env) == 37
    ints = [-3, 100]            # below every range; above every bounded one
    got = _worker("knobs", json.dumps(ints), env=env)
    for name, var, default, _, _ in RULES:
        want = default if var is None else _lib.knob_stored(name, text=texts[name])
        assert got["created"][name] == want and (var is None or want != default), (name, got["created"][name], want)
        for v in ints:
            assert got["set"][str(v)][name] == _lib.knob_stored(name, value=v), (name, v)
    assert got["pair_prec"] == "bf16"
    assert got["unknown_set"] == [_lib.MIND_EINVAL, "mind_set_tuning: unknown knob 'no_such_knob'"]
    assert got["unknown_get"] == [_lib.MIND_EINVAL, "mind_get_tuning: unknown knob 'no_such_knob'", -77]


def test_a_context_gives_back_everything():
    got = _worker("handles")
    base = got["base"]
    assert base == 0
    assert all(u > got["fresh"] for u in got["used"]), got           # (buffers, events, staging made at first use: the count really moves)
    assert got["after"] == [base, base], got
    assert got["fresh"] > base and got["after_fresh"] == base, got
    assert got["pending"] > got["fresh"] and got["after_pending"] == base, got


def test_the_background_switch():
    got = _worker("background")
    assert got["wgs"] == [1, 8, 1, 4, 4, 4] and got["ref_wgs"] == 8, got
    warm, full = got["want"]
    assert got["got"] == [warm, full, warm, full, warm], got
