"""CPU: which kernel a small, merged token launch takes (pred_tok_form / pred_choose, mind_amd/csrc/pred_choice.h, read through
mind_debug_token_form with no context): by rule the small-launch form k_token_s -- on two tokens per workgroup while every workgroup still
gets a CU of its own, (n_tok + 1) / 2 <= n_cu, else on four -- and, forced for A/B, k_token_m or either k_token_s.  Runs that are not small
and merged are no business of the setting, and the rows of mind_debug_predict_choice keep their six fields and their values."""
import pytest

from mind_amd._lib import MIND_EINVAL, TOKEN_FORMS, load, predict_choice, token_form

M, S4, S2 = (TOKEN_FORMS.index(n) for n in ("k_token_m", "k_token_s<4>", "k_token_s<2>"))
COUNTS = (1, 2, 92, 460, 511, 512, 513, 2048, 2049)


def expected(n_tok, n_cu, small_max=2048):
    if n_tok > small_max:
        return 0                                      # eight tokens per workgroup: k_token<8>
    return S2 if (n_tok + 1) // 2 <= n_cu else S4


@pytest.mark.parametrize("n_cu", [256, 64])
def test_rule_at_the_listed_token_counts(n_cu):
    got = {n: token_form(0, n, n_cu) for n in COUNTS}
    assert got == {n: expected(n, n_cu) for n in COUNTS}, got
    # spelled out, so that the helper above cannot hide a wrong rule
    if n_cu == 256:
        assert got == {1: S2, 2: S2, 92: S2, 460: S2, 511: S2, 512: S2, 513: S4, 2048: S4, 2049: 0}
    else:
        assert got == {1: S2, 2: S2, 92: S2, 460: S4, 511: S4, 512: S4, 513: S4, 2048: S4, 2049: 0}
    # both sides of the rule's edge on this device size
    assert (token_form(0, 2 * n_cu, n_cu), token_form(0, 2 * n_cu + 1, n_cu)) == (S2, S4)
    assert (token_form(0, 2 * n_cu - 1, n_cu), token_form(0, 2 * n_cu + 2, n_cu)) == (S2, S4)


@pytest.mark.parametrize("n_cu", [256, 64])
def test_forced_forms_hold_for_every_small_run_and_for_no_other(n_cu):
    for form in (M, S4, S2):
        for n in COUNTS:
            assert token_form(form, n, n_cu) == (form if n <= 2048 else 0), (form, n)
        assert token_form(form) == form               # no token count: the setting itself


def test_bad_arguments_are_rejected():
    lib = load()
    for form, n_tok, n_cu in ((-1, 92, 256), (4, 92, 256), (0, -1, 256), (0, 92, 0), (0, 92, -3)):
        assert lib.mind_debug_token_form(None, form, n_tok, n_cu) == MIND_EINVAL, (form, n_tok, n_cu)
        assert token_form(form, n_tok, n_cu) is None
    assert lib.mind_debug_token_form(None, 0, 0, 0) == 0      # (no token count: n_cu is not read)


def test_choice_record_rows_keep_their_fields_and_values():
    """the cases tests/test_predict_choice_host.py pins, unchanged by the new form (which is no field of the row)"""
    ONE = [(3, 4)]
    two = [(3, 4), (20, 27)]

    def scenes_of(*tokens):
        return [(1, n - 2) for n in tokens]

    for prec in ("f32", "bf16x3", "bf16", "bf16x6"):
        assert predict_choice({}, prec, ONE)["runs"] == [(0, 8, 0, 0, 1, 1)]
        assert predict_choice({"tok_merge": 0}, prec, ONE)["runs"] == [(0, 8, 0, 0, 1, 0)]
    assert predict_choice({}, "bf16x6", scenes_of(1024, 1024))["runs"] == [(0, 2048, 0, 0, 1, 1)]
    assert predict_choice({}, "bf16x6", scenes_of(1024, 1025))["runs"] == [(0, 2049, 0, 0, 0, 0)]
    assert predict_choice({"tok_small_max": 7}, "bf16x6", ONE)["runs"] == [(0, 8, 0, 0, 0, 0)]
    assert predict_choice({"tok_small_max": 8}, "bf16x6", ONE)["runs"] == [(0, 8, 0, 0, 1, 1)]
    assert predict_choice({"tok_bf_min_n": 40}, "bf16x3", two)["runs"] == [(0, 8, 0, 0, 1, 1), (8, 48, 2, 0, 0, 0)]
    assert predict_choice({"tok_bf_min_n": 40}, "bf16x6", two)["runs"] == [(0, 56, 0, 0, 1, 1)]
    for n_cu in (256, 64):
        d = predict_choice({}, "bf16x6", [(36, 55)] * 5, n_cu=n_cu)
        assert d["runs"] == [(0, 460, 0, 0, 1, 1)] and all(len(r) == 6 for r in d["runs"])
