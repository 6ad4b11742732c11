"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the kernels of a point cloud's normals
(cloud_normals.hip: the estimate - bounds, grid, count, the three scan kernels, scatter, search in its plain and its counting form, solve - and the tile stage that
shades a cloud's splats with them), which are built into an object directory of their own (mvlm_amd/csrc/build/normals/) and
recorded in a table of their own (tests/golden/kernel_occupancy_normals.json, tools/kernel_occupancy.py --write): exactly these
kernels, no fewer waves per SIMD and no more spilled registers than recorded, none spills, none uses scratch memory (the
search keeps its 16 best neighbours in LDS, not in a private array) - and none of them in any other object directory."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
KERNELS = ("normals_bounds_kernel", "normals_grid_kernel", "normals_count_kernel", "normals_scan_sums_kernel",
           "normals_scan_top_kernel", "normals_scan_apply_kernel", "normals_scatter_kernel", "normals_search_kernelILb0E",
           "normals_search_kernelILb1E", "normals_solve_kernel", "normals_tile_kernel")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_normals_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "normals"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.NORMALS_TABLE.read_text())
    got = ko.build_table(objdir)
    assert len(got) == len(KERNELS) and len(want) == len(KERNELS), sorted(got)
    for name in KERNELS:
        assert len([k for k in got if name in k]) == 1, (name, sorted(got))
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"]
                               or v["scratch"] > want[k]["scratch"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in got.values()), got
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in want.values()), want
    assert not [k for k in got if "points_" in k]          # (the point kernels' own directory keeps exactly its five)


def test_the_normals_kernels_live_in_their_own_object_directory():
    ko = _tool()
    if not any((ko.BUILD / "normals").glob("*.o")) or not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    elsewhere = dict(ko.build_table())
    for sub in ("points", "msaa", "vcolor", "view", "rays", "sheet", "heat"):
        elsewhere.update(ko.build_table(ko.BUILD / sub))
    assert not [k for k in elsewhere if "normals_" in k]
