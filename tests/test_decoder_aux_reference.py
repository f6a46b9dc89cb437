"""CPU, beside the reference tree only: tests/golden/decoder_aux.npz is what tests/golden/gen_decoder_aux.py computes from the imported
reference today (both curve bases, every case).  Skipped where the reference tree is absent -- the fixture then stands on its own, and the
GPU tests (tests/test_gpu_decoder_aux.py) read only the file."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def reference_import():
    """the reference importable for one test: what oracle/ref_harness.install() registers (its path entry, its stand-in modules, the
    reference's top-level packages) is taken back afterwards, so that no later test sees it"""
    from oracle import ref_harness as rh
    if not rh.available():
        pytest.skip("the reference tree is not on this machine")
    path, mods, was = list(sys.path), set(sys.modules), rh._installed
    yield rh
    sys.path[:] = path
    for k in set(sys.modules) - mods:
        del sys.modules[k]
    rh._installed = was


@pytest.mark.reference
def test_committed_fixture_is_what_the_generator_computes(reference_import):
    spec = importlib.util.spec_from_file_location("gen_decoder_aux", os.path.join(ROOT, "tests", "golden", "gen_decoder_aux.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fresh = gen.generate()
    held = dict(np.load(gen.PATH))
    assert sorted(fresh) == sorted(held)
    assert len(fresh) == 2 * 3 * 5
    for k in fresh:
        assert fresh[k].shape == held[k].shape and held[k].dtype == np.float32, k
        assert np.abs(fresh[k].astype(np.float64) - held[k]).max() <= 1e-6, k
