"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the surface heat's kernels
(surface_backproject.hip: score, paint, peaks), which are built into an object directory of their own
(mvlm_amd/csrc/build/backproject/) and recorded in a table of their own (tests/golden/kernel_occupancy_backproject.json,
tools/kernel_occupancy.py --write): exactly these kernels, no fewer waves per SIMD and no more spilled registers than recorded, none
spills, none uses scratch memory - and none of them in any other object directory."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
KERNELS = ("backproject_score_kernel", "backproject_paint_kernel", "backproject_peaks_kernel")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_occupancy", REPO / "tools" / "kernel_occupancy.py")
    ko = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ko)
    return ko


def test_backproject_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "backproject"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.BACKPROJECT_TABLE.read_text())
    got = ko.build_table(objdir)
    assert len(got) == len(KERNELS) and len(want) == len(KERNELS), sorted(got)
    for name in KERNELS:
        assert len([k for k in got if name in k]) == 1, (name, sorted(got))
    assert all(set(v) == {"waves_per_simd", "spilled", "scratch"} for v in want.values()), want
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"]
                               or v["scratch"] > want[k]["scratch"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in got.values()), got
    assert all(v["spilled"] == 0 and v["scratch"] == 0 for v in want.values()), want


def test_the_backproject_kernels_live_in_their_own_object_directory():
    ko = _tool()
    if not any((ko.BUILD / "backproject").glob("*.o")) or not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    others = [d for d in ko.BUILD.iterdir() if d.is_dir() and d.name not in ("backproject", "timing")]
    assert not [k for k in ko.build_table() if "backproject_" in k]
    for d in others:
        assert not [k for k in ko.build_table(d) if "backproject_" in k], d


def test_the_table_is_committed_and_the_tool_writes_it():
    """Needs no build: the table lists the three kernels, and the tool knows the directory."""
    ko = _tool()
    want = json.loads(ko.BACKPROJECT_TABLE.read_text())
    assert ko.BACKPROJECT_TABLE == REPO / "tests" / "golden" / "kernel_occupancy_backproject.json"
    assert len(want) == 3 and all(len([k for k in want if name in k]) == 1 for name in KERNELS)
