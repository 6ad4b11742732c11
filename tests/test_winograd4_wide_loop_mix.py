"""The instruction mix of the steady-state K loop of the F(4,3) Winograd tile's wide workgroup shape, read off the built object
(tools/conv_loop_mix.py, build/wino4w/).  The loop that tests/golden/conv_loop_mix_wino4w.json records must not grow: no more
non-MFMA instructions per MFMA than recorded, exactly one barrier per 4-channel group - and the recorded ratio is what the shape
is for: strictly below the 32 x 16 shape's in tests/golden/conv_loop_mix_wino4.json, whose workgroup stages the same input tile
for half as many output channels."""
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
    objdir = lm.BUILD / "wino4w"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    return lm, lm.build_table(objdir)


def test_the_wide_loop_holds_no_more_than_recorded(rows):
    lm, got = rows
    want = json.loads(lm.WINO4W_TABLE.read_text())
    assert got and sorted(got) == sorted(want), (sorted(got), sorted(want))
    assert all("Li64E" in k and "Li34E" in k for k in got)
    for k, v in got.items():
        print(f"\nloop-mix {k}: {v}")
        assert v["mfma"] * want[k]["non_mfma"] >= v["non_mfma"] * want[k]["mfma"], (v, want[k])  # got/mfma <= want/mfma, in integers


def test_one_barrier_per_channel_group(rows):
    lm, got = rows
    for v in got.values():
        assert v["mfma"] % lm.MFMAS_PER_CHUNK_WINO4 == 0
        assert v["barriers"] == v["mfma"] // lm.MFMAS_PER_CHUNK_WINO4, v


def test_the_recorded_ratio_is_below_the_narrow_shape():
    lm = _tool()
    wide = json.loads(lm.WINO4W_TABLE.read_text())
    narrow = json.loads(lm.WINO4_TABLE.read_text())
    assert wide and len(narrow) == 1
    (n,) = narrow.values()
    assert (n["non_mfma"], n["mfma"]) == (422, 72)  # 211 per 36
    for v in wide.values():
        assert v["non_mfma"] * n["mfma"] < n["non_mfma"] * v["mfma"], (v, n)  # strictly fewer per MFMA, in integers
