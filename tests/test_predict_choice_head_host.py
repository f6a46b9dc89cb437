"""CPU: pred_choose's rule for the split decoder's head (k_dec_actor<2, agents per workgroup>; mind_amd/csrc/pred_choice.h) through
mind_debug_predict_choice: one agent per workgroup while the call's agents fit one workgroup per CU, else two, else four; "dec_head_ra"
forces a form (4: the head as it was); outside the split form the field is 0.  The rest of the record is tests/test_predict_choice_host.py's."""
import pytest

from mind_amd._lib import predict_choice

DEC_ONE, DEC_SPLIT, DEC_MFMA = 0, 1, 2


def _head(knobs, agents, n_cu=256, **kw):
    d = predict_choice(knobs, "bf16x6", [(a, 4) for a in agents], n_cu=n_cu, **kw)
    return d["dec_actor"], d["dec_head_ra"]


@pytest.mark.parametrize("agents, n_cu, want", [
    ([1], 256, 1), ([36], 256, 1), ([256], 256, 1),                  # one workgroup per agent fits
    ([257], 256, 2), ([512], 256, 2), ([200, 200], 256, 2),          # ... no longer; two agents per workgroup do (the call's agents, not a scene's)
    ([513], 256, 4), ([300, 300], 256, 4), ([13824], 256, 4),        # ... nor that
    ([9], 8, 2), ([16], 8, 2), ([17], 8, 4), ([8], 8, 1), ([7] * 6, 304, 1),
])
def test_head_form_follows_the_calls_agents(agents, n_cu, want):
    assert _head({}, agents, n_cu) == (DEC_SPLIT, want)


@pytest.mark.parametrize("forced", [1, 2, 4])
def test_the_knob_forces_a_form(forced):
    for agents in ([1], [36], [600]):
        assert _head({"dec_head_ra": forced}, agents) == (DEC_SPLIT, forced)


def test_other_values_mean_the_rule():
    for v in (0, 3, 5, 8, -1):
        assert _head({"dec_head_ra": v}, [36]) == (DEC_SPLIT, 1)
        assert _head({"dec_head_ra": v}, [600]) == (DEC_SPLIT, 4)


def test_no_head_form_outside_the_split_decoder():
    assert _head({"dec_overlap": 0}, [36]) == (DEC_ONE, 0)
    assert _head({}, [36], have_side=False) == (DEC_ONE, 0)
    assert _head({"dec_mfma_min": 0}, [36]) == (DEC_MFMA, 0)
    assert _head({"dec_overlap": 0, "dec_head_ra": 2}, [36]) == (DEC_ONE, 0)
