"""The occupancy guard of tests/test_rays_occupancy.py for the PNG encoder's kernels (mvlm_png_encode), which are built into an
object directory of their own (mvlm_amd/csrc/build/png/) and recorded in a table of their own
(tests/golden/kernel_occupancy_png.json, tools/kernel_occupancy.py --write): exactly these four kernels, no fewer waves per SIMD
and no more spilled registers than recorded, none spills or uses scratch memory at all - and none of them in another table."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
KERNELS = ("png_filter_kernel", "png_deflate_kernel", "png_offsets_kernel", "png_gather_kernel")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def _other_tables(ko):
    return ((ko.TABLE, ko.BUILD), (ko.MSAA_TABLE, ko.BUILD / "msaa"), (ko.VCOLOR_TABLE, ko.BUILD / "vcolor"),
            (ko.WINO_TABLE, ko.BUILD / "wino"), (ko.WINO4_TABLE, ko.BUILD / "wino4"), (ko.REPORT_TABLE, ko.BUILD / "report"),
            (ko.VIEW_TABLE, ko.BUILD / "view"), (ko.RAYS_TABLE, ko.BUILD / "rays"))


def test_png_kernel_occupancy_table():
    ko = _tool()
    want = json.loads(ko.PNG_TABLE.read_text())
    assert len(want) == len(KERNELS) and all([k for k in want if name in k] for name in KERNELS), sorted(want)
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in want.values()), want
    objdir = ko.BUILD / "png"
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


def test_the_other_tables_do_not_see_the_png_kernels():
    ko = _tool()
    own = json.loads(ko.PNG_TABLE.read_text())   # the table that does hold them
    assert all(len([k for k in own if n in k]) == 1 for n in KERNELS), sorted(own)
    for table, _ in _other_tables(ko):
        assert not [k for k in json.loads(table.read_text()) if any(n in k for n in KERNELS)], table
    if not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    for _, objdir in _other_tables(ko):
        assert not [k for k in ko.build_table(objdir) if any(n in k for n in KERNELS)], objdir
