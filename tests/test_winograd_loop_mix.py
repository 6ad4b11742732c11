"""The instruction mix of the Winograd tile's steady-state K loop, read off the built object (tools/conv_loop_mix.py).

The tile is compute-bound by construction; what it loses against the matrix peak is what its waves issue besides MFMAs inside
the K loop.  The loop that tests/golden/conv_loop_mix_wino.json records must not grow: no more non-MFMA instructions per MFMA
than recorded, at most half of what the loop held before it was rewritten (284 for the 48 MFMAs of one 4-channel group), and
exactly one barrier per 4-channel group it processes."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
BEFORE_NON_MFMA, BEFORE_MFMA = 284, 48  # the loop of one K-chunk before the rewrite


def _tool():
    spec = importlib.util.spec_from_file_location("conv_loop_mix", REPO / "tools" / "conv_loop_mix.py")
    lm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lm)
    return lm


@pytest.fixture(scope="module")
def rows():
    lm = _tool()
    objdir = lm.BUILD / "wino"
    if not any(objdir.glob("*.o")):
        pytest.skip("no object files (the library was not built from source here)")
    return lm, lm.build_table(objdir)


def test_the_winograd_loop_holds_no_more_than_recorded(rows):
    lm, got = rows
    want = json.loads(lm.WINO_TABLE.read_text())
    assert got and sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k, v in got.items():
        print(f"\nloop-mix {k}: {v}")
        assert v["mfma"] * want[k]["non_mfma"] >= v["non_mfma"] * want[k]["mfma"], (v, want[k])  # got/mfma <= want/mfma, in integers


def test_the_winograd_loop_holds_at_most_half_of_what_it_did(rows):
    _, got = rows
    for v in got.values():
        assert 2 * v["non_mfma"] * BEFORE_MFMA <= BEFORE_NON_MFMA * v["mfma"], v
        assert v["non_mfma_per_mfma"] <= 3.0


def test_one_barrier_per_channel_group(rows):
    lm, got = rows
    for v in got.values():
        assert v["mfma"] % lm.MFMAS_PER_CHUNK_WINO == 0
        assert v["barriers"] == v["mfma"] // lm.MFMAS_PER_CHUNK_WINO, v


def test_the_tool_classes_by_prefix():
    lm = _tool()
    assert lm.classify("v_mfma_f32_32x32x2_f32") == "mfma" and lm.classify("v_fma_f32") == "valu"
    assert lm.classify("ds_read2st64_b32") == "lds_read" and lm.classify("ds_write_b128") == "lds_write"
    assert lm.classify("global_load_dwordx4") == "global_load" and lm.classify("s_waitcnt") == "wait"
    assert lm.classify("s_barrier") == "barrier" and lm.classify("s_cbranch_scc1") == "scalar"
