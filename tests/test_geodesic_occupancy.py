"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the kernels of the surface distances between
landmarks (geodesic.hip), which are built into an object directory of their own (mvlm_amd/csrc/build/geodesic/) and recorded in a
table of their own (tests/golden/kernel_occupancy_geodesic.json, tools/kernel_occupancy.py --write): exactly these kernels, no
fewer waves per SIMD and no more spilled registers than recorded, none spills, none uses scratch memory (the sweep keeps its
sources' values in registers, not in a private array) - and none of them in any other object directory."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
KERNELS = ("geodesic_count_kernel", "geodesic_scan_sums_kernel", "geodesic_scan_top_kernel", "geodesic_scan_apply_kernel",
           "geodesic_fill_kernel", "geodesic_attached_kernel", "geodesic_init_kernel", "geodesic_ring_kernel", "geodesic_sweep_kernel",
           "geodesic_settle_kernel", "geodesic_target_kernel", "geodesic_euclid_kernel", "geodesic_finish_kernel")
FOREIGN = ("points_", "normals_", "sheet_", "heat_", "backproject_", "cloudmesh_", "tile_kernel", "classify_kernel", "_ms_kernel", "tile_vc")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_the_table_names_exactly_the_kernels():
    """(needs no build: the committed table itself)"""
    want = json.loads(_tool().GEODESIC_TABLE.read_text())
    assert len(want) == len(KERNELS)
    for name in KERNELS:
        assert len([k for k in want if name in k]) == 1, (name, sorted(want))
    assert all(v["spilled"] == 0 and v["scratch"] == 0 and v["waves_per_simd"] >= 1 for v in want.values()), want


def test_geodesic_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "geodesic"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.GEODESIC_TABLE.read_text())
    got = ko.build_table(objdir)
    assert len(got) == len(KERNELS) and len(want) == len(KERNELS), sorted(got)
    for name in KERNELS:
        assert len([k for k in got if name in k]) == 1, (name, sorted(got))
    assert all("geodesic_" in k for k in got), sorted(got)
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"]
                               or v["scratch"] > want[k]["scratch"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in got.values()), got
    assert not [k for k in got if any(f in k for f in FOREIGN)]


def test_the_geodesic_kernels_live_in_their_own_object_directory():
    ko = _tool()
    if not any((ko.BUILD / "geodesic").glob("*.o")) or not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    elsewhere = dict(ko.build_table())
    for sub in ("points", "normals", "cloudmesh", "msaa", "vcolor", "view", "rays", "sheet", "heat", "backproject", "report", "png"):
        elsewhere.update(ko.build_table(ko.BUILD / sub))
    assert not [k for k in elsewhere if "geodesic_" in k]
