"""The longest run of other instructions between two consecutive MFMAs of the F(4,3) Winograd tiles' steady K loop, read off the
built objects (tools/conv_loop_mix.py: max_gap; build/wino4/ and build/wino4w/), waits and the barrier counted.

A wave issues in order: behind an MFMA, only what that one MFMA covers is free.  A v_mfma_f32_32x32x2_f32 holds the matrix pipe
for 64 cycles and a vector instruction takes 4 to issue, so 16 instructions is what a gap can hold.  The chunk schedule places
the staging slice by slice in the gaps (conv_wino4.h: Wino4Plan); tests/golden/conv_gap_mix_wino4.json records the largest gap per
kernel, nothing may exceed its record, and no record may exceed 16.

The commit before the slices placed a k-step's whole staging between its 2nd and 3rd MFMA: its largest gaps, read from its
objects with the same tool, were 84 (the 32 x 16 shape) and 85 (the wide shape)."""
import importlib.util
import json
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
GAP_LIMIT = 16  # 64 cycles of one MFMA / 4 cycles of issue per vector instruction


def _tool():
    spec = importlib.util.spec_from_file_location("conv_loop_mix", REPO / "tools" / "conv_loop_mix.py")
    lm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lm)
    return lm


@pytest.fixture(scope="module")
def tables():
    lm = _tool()
    if not all(any((lm.BUILD / d).glob("*.o")) for d in lm.WINO4_GAP_DIRS):
        pytest.skip("no object files (the library was not built from source here)")
    return lm, {d: lm.gap_table(lm.BUILD / d) for d in lm.WINO4_GAP_DIRS}


def test_no_gap_exceeds_its_record(tables):
    lm, got = tables
    want = json.loads(lm.WINO4_GAP_TABLE.read_text())
    assert sorted(got) == sorted(want) == sorted(lm.WINO4_GAP_DIRS)
    for d in lm.WINO4_GAP_DIRS:
        assert got[d] and sorted(got[d]) == sorted(want[d]), (sorted(got[d]), sorted(want[d]))
        for k, gap in got[d].items():
            print(f"\ngap-mix {d} {k}: {gap} (recorded {want[d][k]})")
            assert gap <= want[d][k], (d, k, gap, want[d][k])


def test_every_record_fits_behind_one_mfma():
    lm = _tool()
    want = json.loads(lm.WINO4_GAP_TABLE.read_text())
    assert sorted(want) == sorted(lm.WINO4_GAP_DIRS)
    for d, rows in want.items():
        assert rows and all("Li34E" in k for k in rows)
        assert all(gap <= GAP_LIMIT for gap in rows.values()), (d, rows)


def test_gaps_of_a_known_body():
    lm = _tool()
    m, o = "mfma", "valu"
    assert lm.mfma_gaps([o, m, o, o, m, m, "wait", "barrier", o]) == [2, 0, 4]  # the last run continues in front of the first MFMA
    assert lm.mfma_gaps([m]) == [0]
