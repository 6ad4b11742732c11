"""What the convolution dispatcher (mvlm_amd/csrc/conv_mfma.hip) decides, pinned without a GPU.

tests/native/conv_route_harness.cpp and the dispatcher's translation unit are compiled host-only and linked without the
kernels and without the HIP runtime; stub launchers record which kernel variant a launch reaches.  The harness prints the
decisions for the shapes of the four tuned tables, a fixed list that reaches every branch of the rules, every context state
(Winograd modes, forced variants, tuning overrides), the pair routing and the per-variant queries, run-length encoded over the
batch axis, the cases that decide alike on one line.  The output must equal tests/golden/conv_routing.txt byte for byte.

Run with the argument "wino4", the harness gives every launch the F(4,3) Winograd tile's weights (ConvArgs::w_wino4) as well and
adds what only that tile decides: the Winograd mode x F(4,3) mode axis over the shapes of both Winograd tables, the launch
features with and without those weights, code 2048 as tuning override and as forced variant, and the per-variant queries for
the codes 1024..4200.  That output must equal tests/golden/conv_routing_wino4.txt byte for byte.  It prints a refused launch
without its message, so it pins which launches are refused, which succeed and on which kernel they land, not the wording.

Run with the argument "f43", the harness prints only what the dispatcher decides once a launch has its variant code (f43_plan): which
workgroup shape of the F(4,3) tile a launch of code 2048 takes (the wide switch, the shape, conv_wino4_wide_hold.h), and which
launches of the 80- and 84-row direct tiles run on that tile over padded weights (the three modes, a forced variant, every feature
that rules it out, conv_tuned_wino4_pad.h), with variant_out and the two launch counters.  That output must equal
tests/golden/conv_routing_f43.txt byte for byte.  Its first lines list what a reader can check against the launchers this
decision was moved out of; the harness checks those statements itself and exits non-zero where one does not hold.

The goldens are a function of the committed tuned tables and of the variant list: a retune or a new variant regenerates them
(run the harness built as below and keep its output) - a change of the dispatcher's code alone must not move them."""
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import REPO

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)
HOST = ["--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-value"]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """The harness binary, built once for the three tests."""
    if HIPCC is None:
        pytest.skip("needs hipcc")
    tmp_path = tmp_path_factory.mktemp("conv_route")
    objs = []
    for src in ("mvlm_amd/csrc/conv_mfma.hip", "tests/native/conv_route_harness.cpp"):
        obj = tmp_path / (Path(src).stem + ".o")
        r = subprocess.run([HIPCC, *HOST, "-x", "hip", "-c", str(REPO / src), "-o", str(obj)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(str(obj))
    exe = tmp_path / "conv_route_harness"
    r = subprocess.run([HIPCC, "--offload-host-only", "-no-hip-rt", *objs, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _equals_golden(exe, args, golden):
    r = subprocess.run([str(exe), *args], capture_output=True)
    assert r.returncode == 0, r.stderr[-3000:]
    want = (REPO / "tests/golden" / golden).read_bytes()
    if r.stdout != want:
        got_lines, want_lines = r.stdout.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (g, w) in enumerate(zip(got_lines, want_lines)) if g != w), min(len(got_lines), len(want_lines)))
        differing = sum(g != w for g, w in zip(got_lines, want_lines)) + abs(len(got_lines) - len(want_lines))
        pytest.fail(f"{differing} lines differ from {golden}, the first at line {first + 1}:\n"
                    f"  golden: {want_lines[first] if first < len(want_lines) else '<end>'}\n"
                    f"  now:    {got_lines[first] if first < len(got_lines) else '<end>'}")


def test_dispatcher_decisions_equal_the_golden(harness):
    _equals_golden(harness, [], "conv_routing.txt")


def test_dispatcher_decisions_with_f43_weights_equal_the_golden(harness):
    _equals_golden(harness, ["wino4"], "conv_routing_wino4.txt")


def test_f43_plan_decisions_equal_the_golden(harness):
    _equals_golden(harness, ["f43"], "conv_routing_f43.txt")
