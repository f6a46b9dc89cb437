#!/usr/bin/env python3
"""Compare two device-only assembly listings (hipcc ... --cuda-device-only -S) kernel by kernel.

    python tools/asm_compare.py before.s after.s [--relaxed REGEX]

Per function symbol: the resource metadata of the code object (registers, spills, scratch, LDS) and the histogram of instruction
mnemonics (first token of every instruction line).  A refactor that only moves text must leave both alone; what the register allocator
and the scheduler may shuffle without changing what the kernel does -- register moves, s_nop, s_waitcnt, and the SGPR count -- is the
ALLOWED set, tolerated in the symbols that match --relaxed (default: every symbol; give the kernels that were touched, every other
one must then be identical).  Exit status 1 when anything else differs, or a symbol exists in one file only."""
import argparse
import collections
import re
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
             ".group_segment_fixed_size")
ALLOWED_META = {".sgpr_count"}
ALLOWED_MNEMONIC = re.compile(r"^(s_mov_b32|s_mov_b64|v_mov_b32\w*|v_accvgpr_\w+|s_nop|s_waitcnt)$")


def parse(text):
    """-> ({symbol: Counter of mnemonics}, {kernel symbol: {metadata key: value}})"""
    hist, meta = {}, []
    cur = None
    in_meta = False
    entry = None
    for line in text.splitlines():
        if in_meta:
            if line.startswith("\t.end_amdgpu_metadata") or line.strip() == ".end_amdgpu_metadata":
                in_meta = False
                continue
            m = re.match(r"^  - (\.\w+):\s*(.*)$", line)
            if m:
                entry = {}
                entry[m.group(1)] = m.group(2).strip()
                meta.append(entry)
                continue
            m = re.match(r"^    (\.\w+):\s*(.*)$", line)
            if m and entry is not None:
                entry[m.group(1)] = m.group(2).strip()
            continue
        s = line.strip()
        if s.startswith(".amdgpu_metadata"):
            in_meta, entry = True, None
            continue
        m = re.match(r"^\s*\.type\s+([^\s,]+),@function", line)
        if m:
            cur = m.group(1)
            hist[cur] = collections.Counter()
            continue
        if s.startswith(".Lfunc_end") or s.startswith(".end_amdhsa_kernel"):
            if s.startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None or not s or s[0] in ".;" or not line[0].isspace():
            continue
        tok = s.split()[0]
        if tok.endswith(":"):
            continue
        hist[cur][tok] += 1
    kernels = {}
    for e in meta:
        if ".name" in e and ".symbol" in e:
            kernels[e[".name"]] = {k: e.get(k, "0") for k in META_KEYS}
    return hist, kernels


def compare(a_text, b_text, relaxed=".*", out=sys.stdout, histogram=False):
    """prints the report (with the full histogram of the relaxed symbols if asked), returns the number of symbols that differ outside
    the allowed set"""
    ha, ma = parse(a_text)
    hb, mb = parse(b_text)
    rx = re.compile(relaxed)
    bad = 0
    for name in sorted(set(ha) | set(hb)):
        if name not in ha or name not in hb:
            print(f"{name}\n  ONLY IN {'the first' if name in ha else 'the second'} file", file=out)
            bad += 1
            continue
        loose = rx.search(name) is not None
        lines, fail = [], False
        if name in ma or name in mb:
            x, y = ma.get(name, {}), mb.get(name, {})
            lines.append("  " + "  ".join(f"{k[1:]} {x.get(k, '?')}" + ("" if x.get(k) == y.get(k) else f" -> {y.get(k, '?')}") for k in META_KEYS))
            for k in META_KEYS:
                if x.get(k) != y.get(k) and not (loose and k in ALLOWED_META):
                    fail = True
        n_a, n_b = sum(ha[name].values()), sum(hb[name].values())
        diff = {t: (ha[name][t], hb[name][t]) for t in sorted(set(ha[name]) | set(hb[name])) if ha[name][t] != hb[name][t]}
        for t in diff:
            if not (loose and ALLOWED_MNEMONIC.match(t)):
                fail = True
        lines.append(f"  {n_a} instructions, {len(ha[name])} mnemonics" + ("" if n_a == n_b else f" -> {n_b} instructions"))
        if diff:
            lines.append("  differ: " + ", ".join(f"{t} {x} -> {y}" for t, (x, y) in diff.items()))
        status = "DIFFERENT" if fail else ("allowed differences only" if diff or lines[0].find("->") >= 0 else "identical")
        print(f"{name}: {status}", file=out)
        for l in lines:
            print(l, file=out)
        if histogram and loose:
            both = sorted(set(ha[name]) | set(hb[name]))
            print("  histogram: " + ", ".join(f"{t} {ha[name][t]}" + ("" if ha[name][t] == hb[name][t] else f" -> {hb[name][t]}") for t in both), file=out)
        bad += fail
    print(f"{len(set(ha) | set(hb))} symbols, {bad} outside the allowed set", file=out)
    return bad


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--relaxed", default=".*", help="regex of the symbols in which the allowed set is tolerated (every other one must be identical)")
    ap.add_argument("--histogram", action="store_true", help="also print the whole mnemonic histogram of the relaxed symbols")
    a = ap.parse_args(argv)
    with open(a.before) as f, open(a.after) as g:
        return 1 if compare(f.read(), g.read(), a.relaxed, histogram=a.histogram) else 0


if __name__ == "__main__":
    sys.exit(main())
