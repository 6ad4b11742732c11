"""The occupancy guard of tests/test_host_logic.py::test_kernel_occupancy_table for the two kernels of the opt-in landmark
report, which are built into an object directory of their own (mvlm_amd/csrc/build/report/) and recorded in a table of their
own (tests/golden/kernel_occupancy_report.json, tools/kernel_occupancy.py --write): exactly these two kernels, no fewer waves
per SIMD and no more spilled registers than recorded, none spills at all - and none of them in the main object directory,
whose table stays as it was."""
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


def test_report_kernel_occupancy_table():
    ko = _tool()
    objdir = ko.BUILD / "report"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    want = json.loads(ko.REPORT_TABLE.read_text())
    got = ko.build_table(objdir)
    assert len(got) == 2 and len(want) == 2, sorted(got)
    assert [k for k in got if "report_kernel" in k] and [k for k in got if "attach_final_kernel" in k], sorted(got)
    worse = {k: (want[k], v) for k, v in got.items()
             if k in want and (v["waves_per_simd"] < want[k]["waves_per_simd"] or v["spilled"] > want[k]["spilled"])}
    assert not worse, worse
    unknown = sorted(set(got) - set(want))
    assert not unknown, f"kernels missing from the table (tools/kernel_occupancy.py --write): {unknown}"
    assert all(v["spilled"] == 0 for v in got.values())


def test_the_report_kernels_stay_out_of_the_main_table():
    ko = _tool()
    if not any(ko.BUILD.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    main = ko.build_table()
    assert not [k for k in main if "report_kernel" in k or "attach_final_kernel" in k]
    assert not set(json.loads(ko.REPORT_TABLE.read_text())) & set(json.loads(ko.TABLE.read_text()))
