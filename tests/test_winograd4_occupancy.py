"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the F(4,3) Winograd convolution tile, which is
built into an object directory of its own (mvlm_amd/csrc/build/wino4/) and recorded in a table of its own
(tests/golden/kernel_occupancy_wino4.json, tools/kernel_occupancy.py --write): no fewer waves per SIMD, no more spilled
registers than recorded, no kernel missing from the table, none spills at all - and neither the main table's objects nor
build/wino/ hold an F(4,3) kernel (their Cfg<> carries 34 in the kernel-size position)."""
import importlib.util
import json
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
WINO4_CFG = re.compile(r"3CfgILi\d+ELi\d+ELi\d+ELi\d+ELi34ELi\d+ELb[01]EEE")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_winograd4_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "wino4"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.WINO4_TABLE.read_text())
    got = ko.build_table(objdir)
    assert got and all(WINO4_CFG.search(k) for k in got), sorted(got)
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    missing = sorted(set(want) - set(got))
    assert not missing, f"kernels of the table that the build does not have: {missing}"
    assert all(v["spilled"] == 0 for v in got.values())
    assert all(v["waves_per_simd"] >= 2 for v in got.values())  # two workgroups per CU: one's staging under the other's MFMAs


def test_the_other_tables_do_not_see_the_winograd4_kernels():
    ko = _tool()
    if not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    for objdir in (ko.BUILD, ko.BUILD / "wino"):
        table = ko.build_table(objdir)
        assert not [k for k in table if WINO4_CFG.search(k)]
        assert [k for k in table if "conv_mfma_kernel" in k]
