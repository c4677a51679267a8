"""The partition decision without a GPU: tests/golden/part_pick_ref.npz -- encode_partition_bottomup and
rdo_partition_decision executed from the reference's text (tests/golden/gen_part_pick_ref.py) -- against the host
statements r1_rd_partition_pick_batch is held to (rdo_glue.partition_pick_bottomup / partition_pick_topdown); the
layout of R1PartPick; PartitionType's values; the mutation checks of docs/PARITY.md."""
import os
import subprocess

import numpy as np
import pytest

import part_pick_util as U
from rav1e_amd import rdo_glue
from rav1e_amd.types import PART_BOTTOMUP, PART_PICK, PART_TOPDOWN, RD_PICK, BlockSize, PartitionType

ROOT = U.ROOT


@pytest.fixture(scope="module")
def ref():
    return U.load()


def family_of(ref, names):
    fam = dict(zip((str(n) for n in ref["c_names"]), (str(f) for f in ref["c_family"])))
    return {fam[n] for n in names}


# ---------------------------------------------------------------- the fixture through the host statements
# lower bounds on what the file holds of each kind the feature is about (the counts the generator printed)
COUNTS = {"trials": 1000, "cases": 130, "nodes": 800, "trees_64_to_8": 4, "must_split": 70, "absent_child": 90,
          "td_absent_refused": 6, "cs422_nodes_without_vert": 3, "tie": 70, "exit_best": 15, "exit_ref": 40,
          "exit_topdown": 7, "noexit_twins": 350, "child_max": 20, "lambda0": 80, "order_differs": 12,
          "fused_differs": 12, "rate_none_arm": 200}


def test_fixture_holds_the_cases_the_feature_is_about(ref):
    for k, low in COUNTS.items():
        assert int(ref["count_" + k]) >= low, (k, int(ref["count_" + k]))
    assert int(ref["count_trials"]) == len(ref["t_case"]) < 2000
    assert {str(f) for f in ref["c_family"]} == {"tree", "tie", "exit", "max", "lambda0", "order", "fused"}
    assert {int(v) for v in ref["t_partition"]} == {0, 1, 2, 3} and {int(v) for v in ref["t_rule"]} == {0, 1}
    # 4:2:2: HORZ is tried, VERT never
    t422 = np.array(["422" in str(ref["c_names"][c]) for c in ref["t_case"]])
    assert (ref["t_partition"][t422] == 1).any() and not (ref["t_partition"][t422] == 2).any()
    # the order tuples: the same numbers, two results
    names = [str(n) for n in ref["c_names"]]
    roots = dict(zip(names, ref["n_rd"][ref["c_root"]]))
    k = 0
    while "order_%d_bottomup" % k in roots:
        assert U.bits(roots["order_%d_bottomup" % k]) != U.bits(roots["order_%d_topdown" % k])
        k += 1
    assert k == int(ref["count_order_differs"])
    # the fused tuples: what a multiply-add in one rounding would give is not what was recorded
    fused = [i for i in range(len(ref["t_case"])) if str(ref["c_family"][ref["t_case"][i]]) == "fused"]
    assert len(fused) == 2 * int(ref["count_fused_differs"])
    for i in fused:
        assert U.model_trial(ref, i, fuse=True)[1] != float(ref["t_best_rd"][i])
    # every early exit has a twin with the exit switched off
    assert {n + "_noexit" for n in names if n.startswith(("exit_", "tie_", "td_exit", "td_tie")) and not n.endswith("_noexit")} <= set(names)


def test_partition_pick_statements_reproduce_every_trial_bit_for_bit(ref):
    def glue(i):
        args = (float(ref["t_best_in"][i]), int(ref["t_partition"][i]), float(ref["t_lam"][i]), U.rate(ref, i), U.children(ref, i))
        if int(ref["t_rule"][i]) == PART_BOTTOMUP:
            return rdo_glue.partition_pick_bottomup(*args, must_split=bool(ref["t_must"][i]), ref_rd=float(ref["t_ref"][i]),
                                                    enable_early_exit=bool(ref["t_ee"][i]))
        assert int(ref["t_rule"][i]) == PART_TOPDOWN
        return rdo_glue.partition_pick_topdown(*args, enable_early_exit=bool(ref["t_ee"][i]))
    assert U.replay(ref, glue) == set()


def test_trials_of_a_node_carry_its_state(ref):
    held = {}
    for i in range(len(ref["t_case"])):
        node = int(ref["t_node"][i])
        assert bool(ref["t_first"][i]) == (node not in held)
        if node in held:
            assert U.bits(ref["t_best_in"][i]) == U.bits(held[node][0])
        elif int(ref["t_rule"][i]) == 0:
            assert float(ref["t_best_in"][i]) == U.F64_MAX
        held[node] = (float(ref["t_best_rd"][i]), int(ref["t_best_part"][i]))
    # what a node returned is what its last trial left
    for node, (rd, part) in held.items():
        assert U.bits(ref["n_rd"][node]) == U.bits(rd) and int(ref["n_part"][node]) == part


def test_recorded_encodes_are_the_block_map_of_the_decisions(ref):
    """bottom-up: the last encode_block_with_modes call over each 4x4 cell is the block the nodes' final partitions put
    there -- what the selects have to leave in the live state"""
    dims = {int(b): b.dims for b in BlockSize}
    by_key = {}
    for row in range(len(ref["n_case"])):
        by_key[(int(ref["n_case"][row]), int(ref["n_bsize"][row]), int(ref["n_x"][row]), int(ref["n_y"][row]))] = row
    sub = {(1, 64, 64): (64, 32), (2, 64, 64): (32, 64), (1, 32, 32): (32, 16), (2, 32, 32): (16, 32), (1, 16, 16): (16, 8),
           (2, 16, 16): (8, 16), (1, 8, 8): (8, 4), (2, 8, 8): (4, 8)}
    size = {v: int(b) for b, v in dims.items()}
    n_checked = 0
    for case in range(len(ref["c_names"])):
        if int(ref["c_rule"][case]) != 0:
            continue
        mw, mh = int(ref["c_mi_w"][case]), int(ref["c_mi_h"][case])
        want = {}

        def walk(bs, x, y):
            if x >= mw or y >= mh:
                return
            part = int(ref["n_part"][by_key[(case, bs, x, y)]])
            w, h = dims[bs]
            if part == 0:
                for cy in range(y, min(y + h // 4, mh)):
                    for cx in range(x, min(x + w // 4, mw)):
                        want[(cx, cy)] = (bs, x, y)
                return
            sw, sh = (w // 2, h // 2) if part == 3 else sub[(part, w, h)]
            for k in range(4):
                ox, oy = (k & 1) * (sw // 4), (k >> 1) * (sh // 4)
                if (part == 1 and k & 1) or (part == 2 and k >> 1):
                    continue
                walk(size[(sw, sh)], x + ox, y + oy)
        root = int(ref["c_root"][case])
        walk(int(ref["n_bsize"][root]), int(ref["n_x"][root]), int(ref["n_y"][root]))
        got = {}
        for e in np.nonzero(ref["e_case"] == case)[0]:
            bs, x, y = int(ref["e_bsize"][e]), int(ref["e_x"][e]), int(ref["e_y"][e])
            w, h = dims[bs]
            for cy in range(y, min(y + h // 4, mh)):
                for cx in range(x, min(x + w // 4, mw)):
                    got[(cx, cy)] = (bs, x, y)
        assert got == want, str(ref["c_names"][case])
        n_checked += 1
    assert n_checked >= 60


# ---------------------------------------------------------------- the mutation checks (docs/PARITY.md)
def moved(ref, **kw):
    return U.replay(ref, lambda i: U.model_trial(ref, i, **kw))


def test_the_model_copy_is_the_model(ref):
    assert moved(ref) == set()


def test_early_exit_on_greater_only_moves_the_tie_cases(ref):
    m = moved(ref, ge=False)
    # the ties that fall on a trial's LAST child must move (the flag changes); one that falls on an earlier child is
    # followed by children the reference never evaluated, whose stand-in cost ends the mutated trial as well
    assert {"tie_split_equals_none", "tie_horz_equals_none", "tie_vert_equals_horz", "tie_lambda0"} <= m
    assert family_of(ref, m) == {"tie"}, sorted(m)


def test_swapped_addition_order_moves_the_order_cases(ref):
    m = moved(ref, swap=True)
    assert len(m) == 2 * int(ref["count_order_differs"]) and family_of(ref, m) == {"order"}, sorted(m)


def test_fused_cost_moves_the_fused_cases(ref):
    m = moved(ref, fuse=True)
    assert len(m) == 2 * int(ref["count_fused_differs"]) and family_of(ref, m) == {"fused"}, sorted(m)


# ---------------------------------------------------------------- R1PartPick and PartitionType as C and the reference see them
def test_part_pick_layout_equals_the_header_compiled_as_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rav1e_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(R1PartPick));']
    lines += ['  printf("%s %%zu\\n", offsetof(R1PartPick, %s));' % (f, f) for f in PART_PICK.names]
    lines += ['  printf("rd_pick_best_rd %zu\\n", offsetof(R1RdPick, best_rd));',
              '  printf("rules %d %d\\n", R1_PART_BOTTOMUP, R1_PART_TOPDOWN);',
              '  printf("partitions %d %d %d %d %d\\n", R1_PARTITION_NONE, R1_PARTITION_HORZ, R1_PARTITION_VERT, R1_PARTITION_SPLIT, R1_PARTITION_INVALID);',
              '  return 0;', '}']
    src, exe = tmp_path / "part_pick_layout.c", tmp_path / "part_pick_layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == PART_PICK.itemsize == 16
    assert PART_PICK.names == ("best_rd", "best_partition", "best_call", "early_exit", "reserved")
    for f in PART_PICK.names:
        assert int(got[f]) == PART_PICK.fields[f][1], f
    assert [PART_PICK.fields[f][1] for f in PART_PICK.names] == [0, 8, 9, 10, 11]
    # a child's cost is read from either struct: best_rd leads both
    assert int(got["rd_pick_best_rd"]) == RD_PICK.fields["best_rd"][1] == PART_PICK.fields["best_rd"][1] == 0
    assert got["rules"].split() == [str(PART_BOTTOMUP), str(PART_TOPDOWN)] == ["0", "1"]
    assert [int(v) for v in got["partitions"].split()] == [int(PartitionType.PARTITION_NONE), int(PartitionType.PARTITION_HORZ),
                                                          int(PartitionType.PARTITION_VERT), int(PartitionType.PARTITION_SPLIT),
                                                          int(PartitionType.PARTITION_INVALID)]


def test_partition_type_values_are_the_references(ref):
    """src/partition.rs:114-126 as the generator read it: the four the encoder tries lead the enum in this order"""
    decl = dict(zip((str(n) for n in ref["enum_partition_names"]), (int(d) for d in ref["enum_partition_discs"])))
    for p in (PartitionType.PARTITION_NONE, PartitionType.PARTITION_HORZ, PartitionType.PARTITION_VERT, PartitionType.PARTITION_SPLIT):
        assert decl[p.name] == int(p)
    assert [str(n) for n in ref["enum_partition_names"]][:4] == ["PARTITION_NONE", "PARTITION_HORZ", "PARTITION_VERT", "PARTITION_SPLIT"]
    assert decl["PARTITION_INVALID"] == 10 and int(PartitionType.PARTITION_INVALID) == -1   # the state's own "none"
