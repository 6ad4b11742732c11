"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the landmark view's kernels
(mvlm_render_landmark_view), which are built into an object directory of their own (mvlm_amd/csrc/build/view/) and recorded in a
table of their own (tests/golden/kernel_occupancy_view.json, tools/kernel_occupancy.py --write): exactly these six kernels, no
fewer waves per SIMD and no more spilled registers than recorded, none spills or uses scratch memory at all - and none of them
in the main, multisampling or vertex-colour tables."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
KERNELS = ("view_transform_kernel", "view_classify_kernel", "view_scan_kernel", "view_bin_fill_kernel", "view_project_kernel",
           "view_tile_kernel")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_view_kernel_occupancy_table():
    ko = _tool()
    want = json.loads(ko.VIEW_TABLE.read_text())
    assert len(want) == len(KERNELS) and all([k for k in want if name in k] for name in KERNELS), sorted(want)
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in want.values()), want
    objdir = ko.BUILD / "view"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    got = ko.build_table(objdir)
    assert len(got) == len(KERNELS), sorted(got)
    for name in KERNELS:
        assert len([k for k in got if name in k]) == 1, (name, sorted(got))
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in got.values()), got


def test_the_other_tables_do_not_see_the_view_kernels():
    ko = _tool()
    for table in (ko.TABLE, ko.MSAA_TABLE, ko.VCOLOR_TABLE):
        assert not [k for k in json.loads(table.read_text()) if any(n in k for n in KERNELS)], table
    if not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    for objdir in (ko.BUILD, ko.BUILD / "msaa", ko.BUILD / "vcolor"):
        assert not [k for k in ko.build_table(objdir) if any(n in k for n in KERNELS)], objdir
