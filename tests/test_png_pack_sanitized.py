"""ASan + UBSan run of the PNG encoder's host side (mvlm_amd/csrc/png_pack.cpp: layout, bound, Adler-32 combination, chunks,
CRC-32) in an executable of its own, the recipe of tests/test_jpeg_plan_sanitized.py: files assembled from the model's segments
(tests/png_model.py) equal the model's files byte for byte; the bound at 1 x 1 and 4096 x 4096 and every refusal."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

import png_cases
import png_model
from conftest import REPO


def _partials(seg: bytes):
    b = np.frombuffer(seg, np.uint8).astype(np.uint64)
    n = len(b)
    return int(b.sum() % 65521), int((b * (n - np.arange(n, dtype=np.uint64))).sum() % 65521)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_png_host_side_under_sanitizers(tmp_path):
    exe = tmp_path / "harness"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(REPO / "mvlm_amd/csrc/png_pack.cpp"), str(REPO / "tests/native/png_pack_harness.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = png_cases.small_cases() + png_cases.big_cases()[:1]
    want = []
    pack = tmp_path / "cases.pack"
    with open(pack, "wb") as f:
        for _, im, mode in cases:
            png, stream, segs = png_model.encode(im, mode)
            want.append(png)
            f.write(struct.pack("<III", im.shape[0], im.shape[1], len(segs)))
            for k, seg in enumerate(segs):
                a, b = _partials(stream[k * png_model.SEGMENT:(k + 1) * png_model.SEGMENT])
                f.write(struct.pack("<III", a, b, len(seg)))
                f.write(seg)
    out = tmp_path / "files.pack"
    r = subprocess.run([str(exe), str(pack), str(out)], capture_output=True, text=True,
                       env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "INVARIANT" not in r.stdout
    data, p = out.read_bytes(), 0
    for (name, _, _), png in zip(cases, want):
        n, = struct.unpack_from("<I", data, p)
        assert data[p + 4:p + 4 + n] == png, name
        p += 4 + n
    assert p == len(data)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("bound ")]
    assert lines[0].startswith("bound 1 1 rc=0 77 ")
    assert lines[1].startswith(f"bound 4096 4096 rc=0 {png_model.png_bound(4096, 4096)} ")
    assert len(lines) == 8 and all(" rc=1 0 png:" in ln for ln in lines[2:]), lines
    assert "crc cbf43926" in r.stdout                       # the CRC-32 check value of "123456789"
