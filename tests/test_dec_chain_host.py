"""CPU: the index rules of the decoder scene part's launch chain (mind_amd/csrc/dec_chain.h) and the rule that picks it.

tests/dec_chain_host_check.cpp includes the header the kernels and pred_choose read and checks, for G = 8 / 16 / 32 workgroups per scene and
the three stage shapes (c3 384 -> 768 on one row, l1 128 -> 1536 and l2 1536 -> 128 on six): every (K part, row, output) item is produced
exactly once; a workgroup's l2 parts read only its own l1 slice; the K split the header assumes is dense_quads' for 1 024 threads and 24 576
partial floats; the G rule at 1, 5, 8, 9, 32 and 33 scenes on 256 and 32 compute units.  The program is built with the host compiler and run
plain and under ASan + UBSan (a stand-alone program: nothing loaded into Python is run under a sanitizer).  The record of pred_choose must
carry the same G, and 0 under the two knobs that keep the one-launch kernels."""
import os
import re
import shutil
import subprocess

import pytest

from mind_amd._lib import predict_choice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dec_chain_host_check.cpp")


def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, SRC, "-o", exe]
    # (the sanitizer runtimes linked statically where the compiler has them: the program then does not care what else the process loads first)
    if not flags or subprocess.call(cmd + ["-static-libasan", "-static-libubsan"], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    return r


@pytest.mark.parametrize("name,flags", [("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])])
def test_index_rules_of_the_chain(tmp_path, name, flags):
    r = _build_and_run(tmp_path, "dec_chain_host_check_" + name, flags)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"checks (\d+) failures (\d+)", r.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) == 0, r.stdout
    assert "FAILED" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


ONE = [(3, 4)]


def test_choice_record_carries_the_chain_by_rule():
    want256 = {1: 32, 5: 32, 8: 32, 9: 16, 16: 16, 17: 8, 32: 8, 33: 0, 40: 0}
    for n, g in want256.items():
        d = predict_choice({}, "bf16x6", ONE * n)
        assert d["dec_chain_g"] == g, (n, d["dec_chain_g"])
        assert d["want_mw"] == 0 and d["cls_on_side"] == 0
    for n, g in {1: 32, 2: 16, 4: 8, 5: 0, 8: 0, 9: 0, 32: 0, 33: 0}.items():
        assert predict_choice({}, "bf16x6", ONE * n, n_cu=32)["dec_chain_g"] == g, n
    # every arithmetic, with or without the side stream or the split actor part: the scene part does not depend on them
    for prec in ("f32", "bf16x3", "bf16", "bf16x6"):
        assert predict_choice({}, prec, ONE * 5)["dec_chain_g"] == 32
    assert predict_choice({}, "bf16x6", ONE, have_side=False)["dec_chain_g"] == 32
    assert predict_choice({"dec_overlap": 0}, "bf16x6", ONE)["dec_chain_g"] == 32
    assert predict_choice({"dec_mfma_min": 0}, "bf16x6", ONE)["dec_chain_g"] == 32


def test_the_two_knobs_keep_the_one_launch_kernels():
    for n in (1, 5, 32, 33):
        d = predict_choice({"dec_mw": 1}, "bf16x6", ONE * n)
        assert d["dec_chain_g"] == 0 and d["want_mw"] == int(n <= 32) and d["mw_blocks"] == (n + 7) // 8 * 64
        d = predict_choice({"dec_cls_side": 1}, "bf16x6", ONE * n)
        assert d["dec_chain_g"] == 0 and d["cls_on_side"] == 1 and d["want_mw"] == 0
    # the knob alone decides, also where the two-launch form itself is not possible
    assert predict_choice({"dec_cls_side": 1, "dec_overlap": 0}, "bf16x6", ONE)["dec_chain_g"] == 0
    assert predict_choice({"dec_mw": 1}, "bf16x6", ONE, n_cu=32)["dec_chain_g"] == 0
