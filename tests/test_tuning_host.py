"""CPU: the knob table (mind_amd/csrc/tuning.h) against a restatement of the rules the library had before there was a table -- the three
setters' if-chains and the getenv lines of mind_ctx_create, copied by hand: names, variables, defaults, what an int becomes, what a
variable's text becomes.  The table is read through mind_debug_tuning (no GPU, no context).  tests/test_gpu_tuning.py checks the same
restatement against a context."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

from mind_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mind_amd", "csrc")

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
NEVER = 1 << 30


# ---- what an int becomes (the setters' expressions)
def any_int(v): return v
def flag(v): return int(v != 0)
def min0(v): return 0 if v < 0 else v
def min1(v): return 1 if v < 1 else v
def wgs(v): return 1 if v < 1 else (32 if v > 32 else v)
def slots(v): return 1 if v < 1 else (12 if v > 12 else v)
def clock(v): return 0 if v < 0 else (2 if v > 2 else v)
def split(v): return 3 if v == 3 else 6
def head_ra(v): return v if v in (1, 2, 4) else 0


def pow2_64(v):
    s, b = 0, 1
    while b <= 64 and v > 0:
        if b <= v:
            s = b
        b <<= 1
    return s


def atoi(s):
    """C's atoi for texts whose value fits an int: optional white space, an optional sign, decimal digits; 0 when there is none"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


# ---- what a variable's text becomes: the int the knob's rule is then applied to, or None = the knob is left alone
def t_atoi(s): return atoi(s)                       # atoi(text), through the setter's rule
def t_char(s): return int(not s[:1] == "0")         # !(text[0] == '0')
def t_flag(s): return int(atoi(s) != 0)             # atoi(text) != 0
def t_pos(s): return atoi(s) if atoi(s) > 0 else None      # ignored unless > 0


# (name, variable or None, default, int rule, text rule), in the table's order: pred_tuning_set, ilqr_tuning_set, the tail of mind_set_tuning
RULES = (
    ("dec_mfma_min", "MIND_DEC_MFMA_MIN", NEVER, any_int, t_atoi),
    ("enc_mfma", "MIND_ENC_MFMA", 1, flag, t_char),
    ("actor_f32", "MIND_ACTOR_F32", 1, flag, t_char),
    ("actor_f32_min", "MIND_ACTOR_F32_MIN", NEVER, any_int, t_atoi),
    ("actor_f32_pair_min", None, NEVER, any_int, None),
    ("actor_lw_min", "MIND_ACTOR_LW_MIN", NEVER, any_int, t_atoi),
    ("actor_lw_chunk", None, 0, min0, None),
    ("actor_split", "MIND_ACTOR_SPLIT", 6, split, t_atoi),
    ("xcd_order", "MIND_XCD_ORDER", 1, flag, t_char),
    ("pair_tile", "MIND_PAIR_TILE", 1, flag, t_char),
    ("dec_overlap", "MIND_DEC_OVERLAP", 1, flag, t_char),
    ("dec_head_ra", "MIND_DEC_HEAD_RA", 0, head_ra, t_atoi),
    ("tok_mfma", "MIND_TOK_MFMA", 0, flag, t_char),
    ("tok_small_max", "MIND_TOK_SMALL_MAX", 2048, any_int, t_atoi),
    ("tok_merge", "MIND_TOK_MERGE", 1, flag, t_char),
    ("dec_mw", "MIND_DEC_MW", 0, flag, t_char),
    ("dec_cls_side", "MIND_DEC_CLS_SIDE", 0, flag, t_char),
    ("tok_bf_min_n", "MIND_TOK_BF_MIN_N", 0, any_int, t_atoi),
    ("tok_lw_min_n", "MIND_TOK_LW_MIN_N", NEVER, any_int, t_atoi),
    ("tok_lw_min", "MIND_TOK_LW_MIN", NEVER, any_int, t_atoi),
    ("tok_lw_chunk", None, 0, min0, None),
    ("tgt_side", "MIND_TGT_SIDE", 1, flag, t_char),
    ("ilqr_chunk", "MIND_ILQR_CHUNK", 0, min0, t_atoi),
    ("ilqr_wgs", "MIND_ILQR_WGS", 16, wgs, t_atoi),
    ("ilqr_multi_min", None, 192, any_int, None),
    ("ilqr_wgs_big", None, 32, wgs, None),
    ("ilqr_big_min", None, 12288, any_int, None),
    ("ilqr_slots", "MIND_ILQR_SLOTS", 10, slots, t_atoi),
    ("ilqr_spec_deriv", "MIND_ILQR_SPEC_DERIV", 1, flag, t_flag),
    ("ilqr_host_out_max", "MIND_ILQR_HOST_OUT_MAX", 4096, min0, t_atoi),
    ("ilqr_score_block", None, 0, pow2_64, None),
    ("ilqr_test_starve", None, 0, flag, None),
    ("plan_chunk_mb", "MIND_PLAN_CHUNK_MB", 96 * 1024, min1, t_pos),
    ("pl_tab_side", "MIND_PL_TAB_SIDE", 0, flag, t_char),
    ("tab_small", "MIND_TAB_SMALL", 1, flag, t_flag),
    ("tab_host_max", "MIND_TAB_HOST_MAX", 4096, min0, t_atoi),
    ("early_eval", "MIND_EARLY_EVAL", 1, flag, t_flag),
    ("glue_fused", "MIND_GLUE_FUSED", 1, flag, t_flag),
    ("dec_mirror", "MIND_DEC_MIRROR", 1, flag, t_flag),
    ("dec_poll", "MIND_DEC_POLL", 1, flag, t_flag),
    ("root_head", "MIND_ROOT_HEAD", 1, flag, t_flag),
    ("round_head", "MIND_ROUND_HEAD", 1, flag, t_flag),
    ("upload_kernel_max", "MIND_UPLOAD_KERNEL_MAX", 1 << 20, min0, t_atoi),
    ("prof_clock", "MIND_PROF_CLOCK", 1, clock, t_atoi),
)
INTS = (INT_MIN, -3, -1, 0, 1, 2, 3, 4, 5, 12, 13, 32, 33, 63, 64, 65, 100, 4096, 2 ** 30, INT_MAX)
TEXTS = ("", "0", "1", "00", "01", "-1", "x", " 1", "2", "3", "4", "13", "99", "-0")


def restated_text(name, s):
    """what a fresh record holds after the knob's variable was read with the text s"""
    _, env, default, rule, text = next(r for r in RULES if r[0] == name)
    v = text(s)
    return default if v is None else rule(v)


def test_the_restatement_counts():
    assert len(RULES) == 44 and len({r[0] for r in RULES}) == 44
    assert sum(r[1] is None for r in RULES) == 8 and all((r[1] is None) == (r[4] is None) for r in RULES)
    assert len({r[1] for r in RULES if r[1]}) == 36
    assert [sum(r[0].startswith("ilqr_") for r in RULES), len(RULES[32:])] == [10, 12]


def test_header_compiles_alone(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "hipcc") if c and shutil.which(c)), "/opt/rocm/bin/hipcc")
    src = tmp_path / "tuning_probe.cpp"
    src.write_text('#include "tuning.h"\nint main() { PredTuning t; TnRefs r; r.pt = &t; int v = 0; return tn_set(r, "dec_mw", 1) && tn_get(r, "dec_mw", &v) && v == 1 ? 0 : 1; }\n')
    exe = str(tmp_path / "tuning_probe")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    assert subprocess.run([exe]).returncode == 0


def test_names_variables_and_defaults():
    assert _lib.knobs() == [(name, env, default) for name, env, default, _, _ in RULES]


def test_every_int_is_stored_as_restated():
    for name, _, _, rule, _ in RULES:
        for v in INTS:
            assert _lib.knob_stored(name, value=v) == rule(v), (name, v)


def test_every_text_is_read_as_restated():
    for name, env, _, _, _ in RULES:
        for s in TEXTS:
            got = _lib.knob_stored(name, text=s)
            if env is None:
                assert got is None, (name, s)         # a knob without a variable: MIND_EINVAL
            else:
                assert got == restated_text(name, s), (name, s, got)


def test_the_two_flag_readings_differ_where_they_did():
    # "x" and "" switch a first-character flag on and an atoi flag off, "-0" likewise; "00" is off and " 1" on for both
    assert [_lib.knob_stored("dec_mw", text=s) for s in ("x", "", "00", "-0", " 1")] == [1, 1, 0, 1, 1]
    assert [_lib.knob_stored("dec_poll", text=s) for s in ("x", "", "00", "-0", " 1")] == [0, 0, 0, 0, 1]
    assert _lib.knob_stored("plan_chunk_mb", text="0") == 96 * 1024 and _lib.knob_stored("plan_chunk_mb", value=0) == 1


def test_unknown_names_and_rows_are_rejected():
    lib = _lib.load()
    v = C.c_int()
    assert _lib.knob_stored("no_such_knob", value=1) is None and _lib.knob_stored("no_such_knob", text="1") is None
    for i in (-1, len(RULES), INT_MAX):
        assert lib.mind_debug_tuning(i, None, None, 0, None, None, C.byref(v)) == _lib.MIND_EINVAL
    assert lib.mind_debug_tuning(0, None, None, 0, None, None, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_tuning(0, None, None, 0, None, None, C.byref(v)) == len(RULES)


def test_the_choice_entries_keep_to_their_own_knobs():
    scenes = [(4, 10)]
    assert _lib.predict_choice({"dec_mw": 1}, "bf16x6", scenes) is not None
    assert _lib.predict_choice({"ilqr_wgs": 8}, "bf16x6", scenes) is None
    assert _lib.predict_choice({"dec_mirror": 0}, "bf16x6", scenes) is None
    assert _lib.ilqr_plan({"ilqr_wgs": 8}, [[-1, 0, 1]]) is not None
    assert _lib.ilqr_plan({"pair_tile": 0}, [[-1, 0, 1]]) is None
    assert _lib.ilqr_plan({"dec_mirror": 0}, [[-1, 0, 1]]) is None


def test_the_header_lists_every_knob_and_variable():
    txt = open(os.path.join(ROOT, "include", "mind_hip.h")).read()
    for name, env, _, _, _ in RULES:
        assert f'"{name}"' in txt, name
        assert env is None or re.search(rf"\b{env}\b", txt), env


def test_no_handle_is_live_in_a_process_that_created_nothing():
    # (a process of its own: this one may hold a context of an earlier test)
    code = "import sys; sys.path.insert(0, sys.argv[1]); from mind_amd import _lib; print(_lib.load().mind_debug_live_handles())"
    out = subprocess.run([sys.executable, "-c", code, ROOT], check=True, capture_output=True, text=True)
    assert out.stdout.split() == ["0"], out.stdout
