"""How a tree-iLQR call launches and which index tables it uploads, checked on the host -- no GPU needed.

The solver decides in il_choose and builds a tree's tables in il_tree_tables (mind_amd/csrc/ilqr_choice.h); mind_debug_ilqr_plan calls the
same two functions for a set of knobs, a device size and a list of parent arrays.  Every launch form gives the same bits, so a wrong choice
changes no result, only speed or residency: these are the rules themselves.  n_cu is 256 unless a case says otherwise.  The knobs reach the
record through tn_set (mind_amd/csrc/tuning.h), the function mind_set_tuning and the MIND_ILQR_* variables go through (with a context, hence a GPU:
test_gpu_ilqr.py::test_context_knobs_reach_the_launch_choice)."""
import pytest

from mind_amd._lib import ilqr_plan

TREE7 = [-1, 0, 1, 1, 2, 3, 4]
IL_SPEC, IL_SLOTS = 4, 12


def chain(m):
    return [-1] + list(range(m - 1))


def choice(knobs, n_trees, nodes, **kw):
    d = ilqr_plan(knobs, [chain(nodes)] * n_trees, **kw)
    return {k: v for k, v in d.items() if k != "trees"}


def items(tree):
    return [tuple(tree["fstep_items"][8 * i:8 * i + 5]) for i in range(len(tree["fstep_q1"]))]


def test_tables_of_the_seven_node_tree():
    t = ilqr_plan({}, [TREE7])["trees"][0]
    assert (t["M"], t["nl"], t["nseg"], t["nsl"], t["maxls"], t["nfs"]) == (7, 5, 3, 2, 2, 2)
    assert t["seg_start"] == [0, 2, 5, 7] and t["seg_nodes"] == [0, 1, 2, 4, 6, 3, 5]
    assert t["slevel_start"] == [0, 1, 3] and t["slevel_segs"] == [0, 1, 2]
    assert t["level_start"] == [0, 1, 2, 4, 6, 7] and t["level_nodes"] == [0, 1, 2, 3, 4, 5, 6]
    assert t["child_start"] == [0, 1, 3, 4, 5, 6, 6, 6] and t["child_list"] == [1, 2, 3, 4, 5, 6, 0]
    rec = t["seg_rec"]
    assert len(rec) == 3 * 16
    assert rec[:7] == [0, 2, 1, 0, 0, 2, 1] and rec[8:10] == [2, 3] and rec[10:16] == [0] * 6
    assert rec[16:23] == [2, 5, 6, 2, 4, 0, 6] and rec[32:39] == [5, 7, 5, 3, 3, 0, 6]      # leaves: no children
    assert t["fstep_start"] == [0, 1, 3] and t["fstep_nstart"] == [0, 2, 7] and t["fstep_nodes"] == t["seg_nodes"]
    assert items(t) == [(0, 2, 0, 1, -1), (2, 5, 2, 4, 1), (5, 7, 3, 5, 1)] and t["fstep_q1"] == [2, 5, 7]
    assert all(t["fstep_items"][8 * i + 5:8 * i + 8] == [0, 0, 0] for i in range(3))


def test_forward_steps_in_chunks():
    whole, t = ilqr_plan({}, [TREE7])["trees"][0], ilqr_plan({"ilqr_chunk": 2}, [TREE7])["trees"][0]
    assert t["nfs"] == 3 and t["fstep_start"] == [0, 1, 3, 4] and t["fstep_nodes"] == [0, 1, 2, 4, 3, 5, 6] and t["fstep_nstart"] == [0, 2, 6, 7]
    assert items(t) == [(0, 2, 0, 1, -1), (2, 4, 2, 4, 1), (5, 7, 3, 5, 1), (4, 5, 6, 6, 4)]
    for k in ("level_start", "level_nodes", "child_start", "child_list", "seg_start", "seg_nodes", "slevel_start", "slevel_segs", "seg_rec"):
        assert t[k] == whole[k]                                   # the chunk size touches the forward steps only
    assert ilqr_plan({"ilqr_chunk": -3}, [TREE7])["trees"][0] == whole              # clamped to 0
    assert ilqr_plan({"ilqr_chunk": 100}, [TREE7])["trees"][0]["nfs"] == 2


def test_single_node_and_chain():
    t = ilqr_plan({}, [[-1]])["trees"][0]
    assert (t["M"], t["nl"], t["nseg"], t["nsl"], t["maxls"], t["nfs"]) == (1, 1, 1, 1, 1, 1)
    assert t["level_start"] == [0, 1] and t["child_start"] == [0, 0] and t["child_list"] == [0] and t["seg_start"] == [0, 1]
    assert t["seg_rec"] == [0, 1, 0, 0, 0, 0, 0] + [0] * 9 and items(t) == [(0, 1, 0, 0, -1)]
    t = ilqr_plan({}, [chain(3)])["trees"][0]
    assert (t["nl"], t["nseg"], t["nsl"], t["maxls"], t["nfs"]) == (3, 1, 1, 1, 1)
    assert t["seg_nodes"] == [0, 1, 2] and t["seg_rec"][:7] == [0, 3, 2, 0, 1, 0, 2] and items(t) == [(0, 3, 0, 1, -1)]
    t = ilqr_plan({"ilqr_chunk": 2}, [chain(3)])["trees"][0]
    assert t["nfs"] == 2 and items(t) == [(0, 2, 0, 1, -1), (2, 3, 2, 2, 1)]


def test_wide_level_is_not_chunked_and_record_holds_six_children():
    star = [-1] + [0] * 7 + list(range(1, 8))        # a root with seven children, each the head of a two-node chain
    for knobs in ({}, {"ilqr_chunk": 1}):
        t = ilqr_plan(knobs, [star])["trees"][0]
        assert (t["nseg"], t["nsl"], t["maxls"], t["nfs"]) == (8, 2, 7, 2)            # widest level 7 > 6: whole segments even with a chunk size
        assert t["fstep_start"] == [0, 1, 8]
        assert t["seg_rec"][:8] == [0, 1, 0, 0, 0, 7, 0, 0] and t["seg_rec"][8:16] == [1, 2, 3, 4, 5, 6, 0, 0]      # seven children, six recorded
        assert t["child_list"][:7] == [1, 2, 3, 4, 5, 6, 7]
    six = [-1] + [0] * 6 + list(range(1, 7))
    assert ilqr_plan({"ilqr_chunk": 1}, [six])["trees"][0]["nfs"] == 3               # widest level 6: chunked


def test_bad_parent_is_reported_at_its_node():
    assert ilqr_plan({}, [[-1, 0, 2]]) == {"bad": (0, 2)}
    assert ilqr_plan({}, [TREE7, [-1, 0, 0, 5, 1]]) == {"bad": (1, 3)}
    assert ilqr_plan({}, [[0]]) == {"bad": (0, 0)} and ilqr_plan({}, [[-1, -1]]) == {"bad": (0, 1)}


@pytest.mark.parametrize("n_trees,nodes,want", [
    (1, 50, dict(form=2, GS=10, spec=1, grid=88, workgroups_per_tree=11)),
    (1, 200, dict(form=1, G=16, GS=1, spec=0, grid=128, workgroups_per_tree=16)),
    (9, 50, dict(form=2, GS=10, spec=1, grid=176)),
    (17, 50, dict(form=2, GS=10, spec=0, grid=240, workgroups_per_tree=10)),
    (33, 50, dict(form=2, GS=6, spec=0, grid=240)),
    (1, 12288, dict(form=1, G=32, grid=256)),
    (1, 12287, dict(form=1, G=16))])
def test_launch_choice_defaults(n_trees, nodes, want):
    d = choice({}, n_trees, nodes)
    assert {k: d[k] for k in want} == want


def test_launch_choice_knobs_and_modes():
    assert choice({"ilqr_test_starve": 1}, 1, 200)["grid"] == 120
    d = choice({"ilqr_test_starve": 1}, 1, 50)
    assert (d["grid"], d["starve_followers"]) == (88, 1) and choice({}, 1, 50)["starve_followers"] == 0
    assert choice({}, 1, 12288, n_cu=64)["G"] == 8
    assert choice({}, 1, 191)["form"] == 2 and choice({}, 1, 192)["form"] == 1
    assert choice({"ilqr_multi_min": 8, "ilqr_wgs": 4}, 1, 19)["workgroups_per_tree"] == 4
    for n_trees, nodes in ((1, 50), (3, 300), (40, 250)):
        d = choice({"ilqr_wgs": 1}, n_trees, nodes)
        assert (d["form"], d["G"], d["GS"], d["grid"], d["workgroups_per_tree"]) == (0, 1, 1, n_trees, 1)
        for mode in (dict(generic=True), dict(evaluate=True), dict(generic=True, evaluate=True)):
            d = choice({}, n_trees, nodes, **mode)
            assert (d["form"], d["G"], d["GS"], d["spec"], d["grid"], d["nslot"]) == (0, 1, 1, 0, n_trees, IL_SPEC)
            assert d["early"] == 0 and (d["host_out"] == 0 if "evaluate" in mode else True)
    assert choice({"ilqr_slots": 1}, 1, 50)["form"] == 0
    assert choice({}, 1, 50, two_fits=True) == choice({}, 1, 50)
    assert choice({"ilqr_spec_deriv": 0}, 1, 50)["workgroups_per_tree"] == 10


def test_slot_sets_host_output_and_early_marks():
    assert choice({}, 1, 50)["nslot"] == 10 and choice({"ilqr_slots": 2}, 1, 50)["nslot"] == IL_SPEC and choice({"ilqr_slots": 12}, 1, 50)["nslot"] == 12
    assert choice({"ilqr_slots": 1}, 1, 50)["nslot"] == IL_SPEC and choice({}, 1, 200)["nslot"] == IL_SPEC
    assert choice({}, 33, 50)["nslot"] == 6                       # GS after the residency loop
    d = ilqr_plan({}, [chain(4000), chain(96)])
    assert (d["form"], d["host_out"], d["early"]) == (1, 1, 0)                        # total_nodes == ilqr_host_out_max; wide: no early marks
    assert ilqr_plan({}, [chain(4000), chain(97)])["host_out"] == 0
    d = ilqr_plan({"ilqr_multi_min": 1 << 20}, [chain(4000), chain(96)])
    assert (d["form"], d["host_out"], d["early"]) == (2, 1, 1)
    assert ilqr_plan({"ilqr_multi_min": 1 << 20}, [chain(4000), chain(97)])["early"] == 0
    d = choice({"ilqr_host_out_max": 0}, 1, 50)
    assert (d["host_out"], d["early"]) == (0, 0)
    assert choice({"ilqr_host_out_max": 50}, 1, 50)["host_out"] == 1 and choice({"ilqr_host_out_max": 49}, 1, 50)["host_out"] == 0


def test_knob_clamps():
    """each ilqr_* knob as mind_set_tuning clamped it"""
    big = 1 << 20
    assert choice({"ilqr_wgs": 99}, 1, 200, n_cu=big)["G"] == 32 and choice({"ilqr_wgs": 0}, 1, 200)["form"] == 0 and choice({"ilqr_wgs": -5}, 1, 50)["GS"] == 1
    assert choice({"ilqr_wgs": 2, "ilqr_wgs_big": 99}, 1, 13000, n_cu=big)["G"] == 32
    assert choice({"ilqr_wgs": 2, "ilqr_wgs_big": 0}, 1, 13000, n_cu=big)["G"] == 2          # clamped to 1: not above ilqr_wgs, unused
    assert choice({"ilqr_big_min": 100}, 1, 200, n_cu=big)["G"] == 32 and choice({"ilqr_multi_min": -1}, 1, 1)["form"] == 1        # (thresholds: unclamped)
    assert choice({"ilqr_slots": 99}, 1, 50)["GS"] == IL_SLOTS and choice({"ilqr_slots": 0}, 1, 50)["GS"] == 1 and choice({"ilqr_slots": -2}, 1, 50)["form"] == 0
    assert choice({"ilqr_spec_deriv": 7}, 1, 50)["spec"] == 1 and choice({"ilqr_spec_deriv": -1}, 1, 50)["spec"] == 1 and choice({"ilqr_spec_deriv": 0}, 1, 50)["spec"] == 0
    assert choice({"ilqr_host_out_max": -9}, 1, 50)["host_out"] == 0
    assert choice({"ilqr_test_starve": 5}, 1, 200)["grid"] == 120 and choice({"ilqr_test_starve": 0}, 1, 200)["grid"] == 128
    assert ilqr_plan({"ilqr_chunk": -1}, [TREE7])["trees"][0]["nfs"] == 2


def test_rejects_and_truncation():
    assert ilqr_plan({"no_such_knob": 1}, [TREE7]) is None
    assert ilqr_plan({"dec_mw": 1}, [TREE7]) is None and ilqr_plan({"upload_kernel_max": 0}, [TREE7]) is None      # knobs of the predictor / the context
    assert ilqr_plan({}, [TREE7], n_cu=0) is None and ilqr_plan({}, [TREE7, []]) is None
    import ctypes as C
    from mind_amd import _lib
    lib = _lib.load()
    nn, par, out = (C.c_int * 1)(7), (C.c_int32 * 7)(*TREE7), (C.c_longlong * 4)(-7, -7, -7, -7)
    n = lib.mind_debug_ilqr_plan(None, None, 0, 256, 0, 1, nn, par, out, 3, None)
    assert n == 16 + 20 + sum(len(v) for k, v in ilqr_plan({}, [TREE7])["trees"][0].items() if isinstance(v, list))
    assert list(out) == [16, 1, 2, -7]                             # ... of which cap were written
    assert lib.mind_debug_ilqr_plan(None, None, 0, 256, 0, 1, None, par, out, 3, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_ilqr_plan(None, None, 0, 256, 0, 1, nn, par, None, 3, None) == _lib.MIND_EINVAL
    assert lib.mind_debug_ilqr_plan(None, None, 0, 256, 8, 1, nn, par, out, 3, None) == _lib.MIND_EINVAL
