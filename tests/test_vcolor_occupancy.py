"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the tile kernels that shade with per-vertex
colours, which are built into an object directory of their own (mvlm_amd/csrc/build/vcolor/) and recorded in a table of their
own (tests/golden/kernel_occupancy_vcolor.json, tools/kernel_occupancy.py --write): exactly these two kernels, no fewer waves
per SIMD and no more spilled registers than recorded, none spills at all - and no fewer waves than the uncoloured tile kernels
whose bodies they share (raster_tile.h)."""
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


def test_vcolor_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "vcolor"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.VCOLOR_TABLE.read_text())
    got = ko.build_table(objdir)
    assert len(got) == 2 and len(want) == 2, sorted(got)
    assert [k for k in got if "tile_vc_kernel" in k] and [k for k in got if "tile_vc_ms_kernelILi4E" in k], sorted(got)
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 for v in got.values())


def test_the_coloured_tile_kernels_keep_the_occupancy_of_the_uncoloured_ones():
    ko = _tool()
    if not any((ko.BUILD / "vcolor").glob("*.o")) or not any(ko.BUILD.glob("*.o")) or not any((ko.BUILD / "msaa").glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    vc = ko.build_table(ko.BUILD / "vcolor")
    main = {k: v for k, v in ko.object_kernels(ko.BUILD / "raster.o").items() if "tile_kernel" in k}
    ms = {k: v for k, v in ko.build_table(ko.BUILD / "msaa").items() if "tile_ms_kernel" in k}
    assert len(main) == 1 and len(ms) == 1
    assert not [k for k in ko.build_table() if "tile_vc" in k] and not [k for k in ko.build_table(ko.BUILD / "msaa") if "tile_vc" in k]
    one = next(v for k, v in vc.items() if "tile_vc_kernel" in k)
    four = next(v for k, v in vc.items() if "tile_vc_ms_kernel" in k)
    assert one["waves_per_simd"] >= next(iter(main.values()))["waves_per_simd"]
    assert four["waves_per_simd"] >= next(iter(ms.values()))["waves_per_simd"]
