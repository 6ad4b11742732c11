"""The F(4,3) Winograd tile's chunk schedule moves no output byte: every case of tools/wino4_schedule_digests.py, on either
workgroup shape, hashes to what tests/golden/wino4_schedule_digests.json records.  That table was written on an MI355X from the
library of the commit before the tile's staging was spread over the MFMA gaps of a chunk, so the comparison is with the old
schedule's bytes and not with a tolerance.  The cases (one chunk to 19, both parities of the chunk count, a padded last chunk,
every border, interior seams, the padded 84-row launch, the three option sets) are described in the tool."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("wino4_schedule_digests", REPO / "tools" / "wino4_schedule_digests.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SD = _tool()
WANT = json.loads(SD.TABLE.read_text())


def test_the_table_covers_the_cases():
    assert sorted(WANT) == sorted(SD.case_id(c, w) for c in SD.CASES for w in SD.WIDE)
    assert {c[0] for c in SD.CASES} >= {4, 8, 12, 16, 20, 24, 22, 73}


@pytest.mark.parametrize("wide", SD.WIDE)
@pytest.mark.parametrize("case", SD.CASES, ids=lambda c: SD.case_id(c, "x")[:-6])
def test_output_bytes_are_the_recorded_ones(case, wide):
    import numpy as np
    from mvlm_amd import _lib

    ctx = _lib.get_context(0)
    SD.padded_launches(ctx)
    y = SD.run_case(ctx, case, wide)
    assert SD.padded_launches(ctx) == (1 if case[5] == 2 else 0)
    assert np.isfinite(y).all()
    assert SD.digest(y) == WANT[SD.case_id(case, wide)]
