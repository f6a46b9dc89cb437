"""tools/asm_compare.py on two short synthetic listings: the per-kernel metadata and mnemonic histogram, the allowed set (register moves, s_nop,
s_waitcnt, .sgpr_count), and the exit status."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import asm_compare  # noqa: E402


def listing(body_a, body_b, vgpr_a=12, sgpr_a=20, lds_b=1024):
    def fn(name, body):
        return (f"\t.protected\t{name}\n\t.globl\t{name}\n\t.type\t{name},@function\n{name}:                                   ; @{name}\n; %bb.0:\n"
                + "".join(f"\t{line}\n" for line in body)
                + f".LBB0_1:                                ; %loop\n\ts_endpgm\n\t.section\t.rodata\n\t.amdhsa_kernel {name}\n\t\t.amdhsa_next_free_vgpr 12\n"
                  f"\t.end_amdhsa_kernel\n\t.text\n.Lfunc_end_{name}:\n\t.size\t{name}, .Lfunc_end_{name}-{name}\n; NumVgprs: 12\n")

    def meta(name, vgpr, sgpr, lds):
        return (f"  - .agpr_count:     0\n    .args:\n      - .address_space:  global\n        .name:           not_a_kernel\n        .offset:         0\n"
                f"    .group_segment_fixed_size: {lds}\n    .name:           {name}\n    .private_segment_fixed_size: 0\n    .sgpr_count:     {sgpr}\n"
                f"    .sgpr_spill_count: 0\n    .symbol:         {name}.kd\n    .vgpr_count:     {vgpr}\n    .vgpr_spill_count: 0\n")
    return ("\t.text\n\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + fn("k_a", body_a) + fn("k_b", body_b)
            + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + meta("k_a", vgpr_a, sgpr_a, 0) + meta("k_b", 40, 30, lds_b)
            + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\n\t.end_amdgpu_metadata\n")


A = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v1, 0", "v_add_u32_e32 v0, v0, v1", "global_store_dword v1, v0, s[0:1]"]
B = ["ds_read_b128 v[0:3], v4", "s_waitcnt lgkmcnt(0)", "v_mfma_f32_16x16x32_bf16 v[0:3], v[4:7], v[8:11], v[0:3]", "s_nop 7"]


def run(x, y, **kw):
    out = io.StringIO()
    bad = asm_compare.compare(x, y, out=out, **kw)
    return bad, out.getvalue()


def test_parse_reads_histogram_and_metadata():
    hist, meta = asm_compare.parse(listing(A, B))
    assert set(hist) == {"k_a", "k_b"} and set(meta) == {"k_a", "k_b"}           # the argument called not_a_kernel is not a kernel
    assert hist["k_a"] == {"s_load_dwordx2": 1, "s_waitcnt": 1, "v_mov_b32_e32": 1, "v_add_u32_e32": 1, "global_store_dword": 1, "s_endpgm": 1}
    assert hist["k_b"]["v_mfma_f32_16x16x32_bf16"] == 1 and hist["k_b"]["s_nop"] == 1
    assert meta["k_a"][".vgpr_count"] == "12" and meta["k_b"][".group_segment_fixed_size"] == "1024" and meta["k_a"][".agpr_count"] == "0"


def test_identical_listings_pass():
    bad, text = run(listing(A, B), listing(A, B))
    assert bad == 0 and "k_a: identical" in text and "k_b: identical" in text


def test_moves_waits_and_the_sgpr_count_are_allowed():
    a2 = A[:2] + ["v_mov_b32_e32 v2, v1", "s_mov_b64 s[2:3], s[0:1]", "s_nop 0"] + A[2:]
    b2 = [B[0], B[2], B[3]]                                                      # one s_waitcnt fewer
    bad, text = run(listing(A, B), listing(a2, b2, sgpr_a=21))
    assert bad == 0 and "k_a: allowed differences only" in text and "sgpr_count 20 -> 21" in text and "v_mov_b32_e32 1 -> 2" in text
    assert "k_b: allowed differences only" in text and "s_waitcnt 1 -> 0" in text


def test_anything_else_fails():
    assert run(listing(A, B), listing(A + ["v_add_u32_e32 v0, v0, v0"], B))[0] == 1      # an instruction of substance
    assert run(listing(A, B), listing(A, B, vgpr_a=13))[0] == 1                            # a VGPR
    assert run(listing(A, B), listing(A, B, lds_b=2048))[0] == 1                           # LDS
    bad, text = run(listing(A, B), listing(A, B).replace("k_b", "k_c"))
    assert bad == 2 and "ONLY IN" in text                                                  # a kernel that exists on one side only


def test_relaxed_pattern_limits_where_the_allowed_set_applies():
    a2 = A + ["v_mov_b32_e32 v2, v1"]
    assert run(listing(A, B), listing(a2, B), relaxed="k_a")[0] == 0
    assert run(listing(A, B), listing(a2, B), relaxed="k_b")[0] == 1             # k_a must then be identical


def test_command_line_exit_status(tmp_path):
    x, y = tmp_path / "x.s", tmp_path / "y.s"
    x.write_text(listing(A, B))
    y.write_text(listing(A, B, vgpr_a=13))
    assert asm_compare.main([str(x), str(x)]) == 0 and asm_compare.main([str(x), str(y)]) == 1
