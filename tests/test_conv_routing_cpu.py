"""What the convolution dispatcher (mvlm_amd/csrc/conv_mfma.hip) decides, pinned without a GPU.

tests/native/conv_route_harness.cpp and the dispatcher's translation unit are compiled host-only and linked without the
kernels and without the HIP runtime; stub launchers record which kernel variant a launch reaches.  The harness prints the
decisions for the shapes of the four tuned tables, a fixed list that reaches every branch of the rules, every context state
(Winograd modes, forced variants, tuning overrides), the pair routing and the per-variant queries, run-length encoded over the
batch axis, the cases that decide alike on one line.  The output must equal tests/golden/conv_routing.txt byte for byte.

The golden is a function of the committed tuned tables and of the variant list: a retune or a new variant regenerates it
(run the harness built as below and keep its output) - a change of the dispatcher's code alone must not move it."""
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import REPO

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
HOST = ["--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-value"]


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
def test_dispatcher_decisions_equal_the_golden(tmp_path):
    objs = []
    for src in ("mvlm_amd/csrc/conv_mfma.hip", "tests/native/conv_route_harness.cpp"):
        obj = tmp_path / (Path(src).stem + ".o")
        r = subprocess.run([HIPCC, *HOST, "-x", "hip", "-c", str(REPO / src), "-o", str(obj)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(str(obj))
    exe = tmp_path / "conv_route_harness"
    r = subprocess.run([HIPCC, "--offload-host-only", "-no-hip-rt", *objs, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True)
    assert r.returncode == 0, r.stderr[-3000:]
    want = (REPO / "tests/golden/conv_routing.txt").read_bytes()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (g, w) in enumerate(zip(got_lines, want_lines)) if g != w), min(len(got_lines), len(want_lines)))
        differing = sum(g != w for g, w in zip(got_lines, want_lines)) + abs(len(got_lines) - len(want_lines))
        pytest.fail(f"{differing} lines differ from the golden, the first at line {first + 1}:\n"
                    f"  golden: {want_lines[first] if first < len(want_lines) else '<end>'}\n"
                    f"  now:    {got_lines[first] if first < len(got_lines) else '<end>'}")
