"""The instruction mix of the F(4,3) Winograd tile's steady-state K loop, read off the built object (tools/conv_loop_mix.py,
build/wino4/).  The loop that tests/golden/conv_loop_mix_wino4.json records must not grow: no more non-MFMA instructions per
MFMA than recorded, and exactly one barrier per 4-channel group it processes.  build/wino/ holds no F(4,3) kernel."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("conv_loop_mix", REPO / "tools" / "conv_loop_mix.py")
    lm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lm)
    return lm


@pytest.fixture(scope="module")
def rows():
    lm = _tool()
    objdir = lm.BUILD / "wino4"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    return lm, lm.build_table(objdir)


def test_the_winograd4_loop_holds_no_more_than_recorded(rows):
    lm, got = rows
    want = json.loads(lm.WINO4_TABLE.read_text())
    assert got and sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k, v in got.items():
        print(f"\nloop-mix {k}: {v}")
        assert v["mfma"] * want[k]["non_mfma"] >= v["non_mfma"] * want[k]["mfma"], (v, want[k])  # got/mfma <= want/mfma, in integers


def test_one_barrier_per_channel_group(rows):
    lm, got = rows
    for v in got.values():
        assert v["mfma"] % lm.MFMAS_PER_CHUNK_WINO4 == 0
        assert v["barriers"] == v["mfma"] // lm.MFMAS_PER_CHUNK_WINO4, v


def test_the_winograd_directory_holds_no_winograd4_kernel(rows):
    lm, got = rows
    assert not set(got) & set(lm.build_table(lm.BUILD / "wino"))
    assert all("Li34E" in k for k in got)
