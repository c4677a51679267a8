"""The compile-time plan of the fused candidate kernel (rav1e_amd/csrc/rdo_cand_plan.hpp) against the built library,
without a device: a host program (tests/c/rdo_plan_list.cpp, the host compiler alone) lists every instantiation the
plan names with its LDS bytes; the library's code objects (read the way tools/kres.py reads them: kernel names and the
LDS-size note, no instructions) must hold exactly those k_rdo_cand kernels with exactly those sizes."""
import collections
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "rav1e_amd", "librav1e_hip.so")
# k_rdo_cand<BD, WL, HL, CT, QM, MT, PS> in its mangled form (CT: s = int16_t, i = int32_t)
KERNEL = re.compile(r"10k_rdo_candILi(\d+)ELi(\d+)ELi(\d+)E([si])Li(\d+)ELb([01])ELi(\d+)EE")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """{(BD, WL, HL, QM, MT, PS): LDS bytes} as the host compiler evaluates the plan"""
    exe = str(tmp_path_factory.mktemp("rdo_plan") / "rdo_plan_list")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "rav1e_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "rdo_plan_list.cpp")])
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([exe], text=True).splitlines()]
    out = {r[:6]: r[6] for r in rows}
    assert len(out) == len(rows)
    return out


@pytest.fixture(scope="module")
def built():
    """{(BD, WL, HL, QM, MT, PS): LDS bytes} of the k_rdo_cand kernels of the built library"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kres import kernel_notes
    out = {}
    for name, field in kernel_notes(SO):
        m = KERNEL.search(name)
        if not m:
            assert "k_rdo_cand" not in name, name
            continue
        bd, wl, hl, ct, qm, mt, ps = m.groups()
        assert ct == ("s" if bd == "8" else "i"), name
        key = (int(bd), int(wl), int(hl), int(qm), int(mt), int(ps))
        assert key not in out, name
        out[key] = int(field("group_segment_fixed_size"))
    return out


def test_plan_names_exactly_the_kernels_of_the_library(plan, built):
    assert sorted(set(plan) - set(built)) == [], "named by the plan, not in the library"
    assert sorted(set(built) - set(plan)) == [], "in the library, not named by the plan"


def test_counts_by_prediction_source_and_type_search(plan, built):
    for keys in (plan, built):
        n = collections.Counter((k[5], k[4]) for k in keys)      # (PS, MT)
        assert (n[0, 0], n[0, 1], n[1, 0] + n[1, 1]) == (171, 54, 105), n
        assert len(keys) == 330


def test_lds_bytes_of_every_kernel_equal_the_plan(plan, built):
    diff = {k: (plan[k], built[k]) for k in plan if k in built and plan[k] != built[k]}
    assert diff == {}, "(plan, library) LDS bytes"
    # four of them as plain numbers (tools/kres.py on the library)
    assert (plan[8, 3, 3, 2, 0, 0], plan[8, 6, 6, 2, 0, 0], plan[10, 6, 6, 2, 0, 0], plan[10, 2, 2, 2, 1, 1]) == \
        (2944, 9216, 10224, 2720)


def test_intra_kernels_need_no_more_lds_than_their_inter_twins(plan, built):
    for lds in (plan, built):
        intra = [k for k in lds if k[5] == 1]
        assert len(intra) == 105
        for k in intra:
            assert lds[k] <= lds[k[:5] + (0,)], k
