"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the multisampled rasteriser's kernels, which
are built into an object directory of their own (mvlm_amd/csrc/build/msaa/) and recorded in a table of their own
(tests/golden/kernel_occupancy_msaa.json, tools/kernel_occupancy.py --write): no fewer waves per SIMD, no more spilled
registers than recorded, no kernel missing from the table, and none spills at all."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_msaa_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "msaa"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.MSAA_TABLE.read_text())
    got = ko.build_table(objdir)
    assert {k for k in got if "_ms_kernel" in k} == set(got) and len(got) == 3, sorted(got)
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 for v in got.values())


def test_the_main_table_does_not_see_the_msaa_kernels():
    """the one-sample rasteriser's kernels stay in the main table's objects, the multisampled ones in their own"""
    ko = _tool()
    if not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    main = ko.build_table()
    assert not [k for k in main if "_ms_kernel" in k]
    assert [k for k in main if "tile_kernel" in k] and [k for k in main if "classify_kernel" in k]
