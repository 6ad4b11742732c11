"""The occupancy guard of tests/test_winograd4_occupancy.py for the F(4,3) Winograd tile's wide workgroup shape, which is built into
an object directory of its own (mvlm_amd/csrc/build/wino4w/) and recorded in a table of its own
(tests/golden/kernel_occupancy_wino4w.json, tools/kernel_occupancy.py --write): every kernel of the directory is in the table and
is the 64-channel F(4,3) Cfg, no fewer waves per SIMD and no more spilled registers than recorded, none spills at all, and two
workgroups stay resident per CU - one's prologue and epilogue under the other's MFMAs."""
import importlib.util
import json
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
WIDE_CFG = re.compile(r"3CfgILi64ELi\d+ELi\d+ELi\d+ELi34ELi\d+ELb[01]EEE")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_winograd4_wide_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "wino4w"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.WINO4W_TABLE.read_text())
    got = ko.build_table(objdir)
    assert got and all(WIDE_CFG.search(k) for k in got), sorted(got)
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    missing = sorted(set(want) - set(got))
    assert not missing, f"kernels of the table that the build does not have: {missing}"
    worse = {k: (want[k], v) for k, v in got.items()
             if v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"]}
    assert not worse, worse
    assert all(v["spilled"] == 0 for v in got.values())
    assert all(v["waves_per_simd"] >= 2 for v in got.values())


def test_the_narrow_shape_directory_does_not_see_the_wide_kernel():
    ko = _tool()
    if not any((ko.BUILD / "wino4").glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    assert not [k for k in ko.build_table(ko.BUILD / "wino4") if WIDE_CFG.search(k)]
