"""Recorded values of the upstream reference for the tests that compare this package against it (tests/golden/ref_live/<test>.pkl).

A test asks for every reference value with `rec(key, fn)`: fn computes it with the imported reference (oracle/ref_harness.py).  The suite
reads the recorded value and never runs fn, so it needs nothing outside the repository; with MIND_RECORD_REF_GOLDEN=1 in a tree beside
the reference the same test runs fn, records its value and still asserts against it (`python -m pytest tests -m reference` then
rewrites the files)."""
import os
import pickle

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_live")
RECORD = os.environ.get("MIND_RECORD_REF_GOLDEN", "0") == "1"


def _plain(v):
    """torch tensors -> numpy, containers recursively (the files must load without the reference's classes)"""
    if hasattr(v, "detach"):
        return v.detach().cpu().numpy()
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(x) for x in v)
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, np.generic):
        return v.item()
    return v


class Recorded:
    def __init__(self, name):
        self.path = os.path.join(DIR, name + ".pkl")
        if RECORD:
            from oracle import ref_harness as rh
            assert rh.available(), "MIND_RECORD_REF_GOLDEN=1 needs the reference tree"
        if RECORD and not os.path.exists(self.path):
            self.data = {}
        else:                   # (recording too: the cases of a parametrised test share one file)
            with open(self.path, "rb") as f:
                self.data = pickle.load(f)

    def __call__(self, key, fn):
        if RECORD:
            self.data[key] = _plain(fn())
            os.makedirs(DIR, exist_ok=True)
            with open(self.path, "wb") as f:
                pickle.dump(self.data, f, protocol=4)
        return self.data[key]
