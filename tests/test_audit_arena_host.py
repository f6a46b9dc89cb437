"""CPU: the typed scratch arena of the audit / forecast entries (mind_amd/csrc/audit_arena.h), compiled alone with the host compiler into a
small program that declares fields and prints what their handles say -- alignment, no overlap, a field of no element, the total, the bytes of
every declared element type, and the read-back entry a handle makes."""
import json
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mind_amd", "csrc")

# (name, element type, bytes of one element, count); "none" holds no element, between two neighbours and once more at the end
FIELDS = (("d", "double", 8, 3), ("i", "int", 4, 5), ("none", "float", 4, 0), ("f", "float", 4, 7), ("u", "uint8_t", 1, 33), ("p", "Pair", 8, 9),
          ("one", "uint8_t", 1, 1), ("d2", "double", 8, 1), ("tail", "int", 4, 0))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include "audit_arena.h"
struct Pair { int a, b; };
template <class T> static void show(const char *name, const ArField<T> &f, size_t top) {
  char base[1];
  static_assert(std::is_same<decltype(f.at(base)), T *>::value, "the handle hands out a pointer to its own element type");
  const ArBack b((T *)nullptr, f);
  printf("{\"name\": \"%s\", \"off\": %zu, \"n\": %zu, \"bytes\": %zu, \"end\": %zu, \"top\": %zu, \"at\": %zu, \"back\": [%zu, %zu]},\n", name, f.off, f.n,
         f.bytes(), f.end(), top, (size_t)((char *)f.at(base) - base), b.off, b.bytes);
}
int main() {
  printf("{\"align\": %zu, \"with\": [\n", AR_ALIGN);
  Arena a;
  @WITH@
  printf("null], \"top\": %zu, \"without\": [\n", a.top);
  Arena w;
  @WITHOUT@
  printf("null], \"top_without\": %zu}\n", w.top);
  return 0;
}
"""


def _takes(arena, fields):
    return "\n  ".join(f'{{ const auto f = {arena}.take<{ty}>({n}); show("{name}", f, {arena}.top); }}' for name, ty, _, n in fields)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "hipcc") if c and shutil.which(c)), "/opt/rocm/bin/hipcc")
    d = tmp_path_factory.mktemp("arena")
    src, exe = str(d / "arena_probe.cpp"), str(d / "arena_probe")
    with open(src, "w") as f:
        f.write(PROGRAM.replace("@WITH@", _takes("a", FIELDS)).replace("@WITHOUT@", _takes("w", [x for x in FIELDS if x[3] > 0])))
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe], check=True, capture_output=True, text=True)
    out = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    out["with"].pop(), out["without"].pop()
    return out


def test_fields_are_aligned_and_disjoint(report):
    assert report["align"] == 16
    rows = report["with"]
    assert [r["name"] for r in rows] == [f[0] for f in FIELDS]
    end = 0
    for r in rows:
        assert r["off"] % 16 == 0 and r["off"] >= end, r                 # on the boundary, behind everything before it
        assert r["off"] - end < 16, r                                     # ... and no further than the boundary asks
        assert r["at"] == r["off"] and r["end"] == r["off"] + r["bytes"] and r["top"] == r["end"], r
        end = r["end"]
    assert rows[0]["off"] == 0


def test_bytes_are_count_times_the_declared_element(report):
    for r, (name, ty, size, n) in zip(report["with"], FIELDS):
        assert r["n"] == n and r["bytes"] == n * size, (name, ty, r)
        assert r["back"] == [r["off"], r["bytes"]], (name, r)             # the read-back copies exactly the field


def test_a_field_of_no_element(report):
    by = {r["name"]: r for r in report["with"]}
    assert by["none"]["bytes"] == 0 and by["none"]["end"] == by["none"]["off"] and by["tail"]["bytes"] == 0
    without = {r["name"]: r for r in report["without"]}
    assert set(without) == set(by) - {"none", "tail"}
    for name, r in without.items():                                       # its neighbours lie where they lie without it
        assert (r["off"], r["bytes"]) == (by[name]["off"], by[name]["bytes"]), name


def test_total_is_the_end_of_the_last_field(report):
    assert report["top"] == report["with"][-1]["end"] == report["with"][-1]["off"]          # (the last field here is the empty one)
    assert report["top_without"] == report["without"][-1]["end"] == report["without"][-1]["off"] + 8
