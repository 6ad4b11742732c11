"""ASan + UBSan run of the convolution weights' host side (mvlm_amd/csrc/conv_pack.cpp) in an executable of its own, the recipe of
tests/test_png_pack_sanitized.py: tests/native/conv_pack_harness.cpp packs seeded layers the way mvlm_conv2d and mvlm_cnn_load do,
and the blobs must equal a numpy restatement bit for bit - the [tap][cin_pad][cout_pad] layout with zeros in the padding, the
F(2,3) and F(4,3) forms (float64, rounded once), the padded F(4,3) copy and its bias, every offset a multiple of four floats.

The harness itself holds the hooks' padding function against the table written below from the four entry points as they stood
before they shared it (api.hip: mvlm_conv2d, mvlm_conv_bench, mvlm_conv2d_pair, mvlm_conv_pair_bench), and the timing hooks' zero
arena against every pointer they hand out; it exits non-zero where one does not hold."""
import shutil
import struct
import subprocess
from itertools import product

import numpy as np
import pytest

from conftest import REPO

SHAPES = [(3, 3, 64), (3, 5, 73), (3, 8, 84), (3, 8, 80), (1, 6, 128), (3, 32, 32)]  # ksize, cin, cout
CASES = [(k, cin, cout, bias) for k, cin, cout in SHAPES for bias in (True, False)]


def _up(x, a):
    return (x + a - 1) // a * a


# ---- the four entry points' padding, as each stated it on its own ---------------------------------------------------------------
def _conv2d_padding(ksize, cin, cout, bias, pre, post, res, up, w, h):
    tail16 = ksize == 3 and _up(cout, 16) == 80 and not pre and not post and not res and w >= 32 and h % 8 == 0
    cin_pad = _up(cin, 8) if ksize == 1 else _up(cin, 4)
    tail4 = ksize == 3 and cout == 84 and bias and not pre and not post and not res and not up and w >= 32 and h % 8 == 0
    return cin_pad, _up(cout, 16) if tail16 else 84 if tail4 else _up(cout, 32)


def _conv_bench_padding(ksize, cin, cout, flags):
    cin_pad = _up(cin, 8) if ksize == 1 else _up(cin, 4)
    plain = bool(flags & 4) and not flags & (1 | 2 | 8)
    return cin_pad, 80 if plain and _up(cout, 16) == 80 else 84 if plain and ksize == 3 and cout == 84 else _up(cout, 32)


def _pair_padding(cin, cout):
    return _up(cin, 4), _up(cout, 32)


def _padding_table():
    rows = []
    for cout, ksize, bias, pre, post, res in product(range(1, 131), (1, 3), *[(0, 1)] * 4):
        cin = cout % 13 + 1
        for up, w, h in product((0, 1), (16, 32), (4, 8)):
            rows.append((0, ksize, cin, cout, bias, pre, post, res, up, w, h, *_conv2d_padding(ksize, cin, cout, bias, pre, post, res, up, w, h)))
        flags = pre | res << 1 | bias << 2 | post << 3
        rows.append((1, ksize, cin, cout, bias, pre, post, res, 0, 64, 64, *_conv_bench_padding(ksize, cin, cout, flags)))
        if ksize == 3:  # (the pair hooks take 3x3 layers only; what else a call carries does not reach their padding)
            rows.append((2, 3, cin, cout, bias, pre, post, res, 0, 64, 64, *_pair_padding(cin, cout)))
    return rows


# ---- the packed forms in numpy ----------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _expected(ksize, cin, cout, w, bias):
    cin_pad, cout_pad = _conv2d_padding(ksize, cin, cout, bias is not None, False, False, False, False, 32, 8)
    taps = ksize * ksize
    w9 = np.zeros((taps, cin_pad, cout_pad), np.float32)
    w9[:, :cin, :cout] = w.transpose(2, 3, 1, 0).reshape(taps, cin, cout)
    want = {"dims": (cin_pad, cout_pad), "w": w9}
    if bias is not None:
        want["bias"] = np.concatenate([bias, np.zeros(cout_pad - cout, np.float32)])
    if ksize != 3:
        return want
    g0, g1, g2 = w9.astype(np.float64).reshape(3, 3, cin_pad, cout_pad)  # ky = 0, 1, 2, each [kx][cin_pad][cout_pad]
    want["f23"] = np.concatenate([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2]).astype(np.float32)
    f43 = np.concatenate([g0, 0.0 - (g0 + g1 + g2) / 3.0, (g0 - g1 + g2) / 3.0, (g0 + 2.0 * g1 + 4.0 * g2) / 15.0,
                          (-16.0 * g0 + 8.0 * g1 - 4.0 * g2) / 15.0, g2]).astype(np.float32)
    want["f43"] = f43
    P = _up(cout_pad, 32)
    want["f43_pad"] = np.zeros((18, cin_pad, P), np.float32)
    want["f43_pad"][:, :, :cout_pad] = f43
    if bias is not None:
        want["bias_pad"] = np.concatenate([want["bias"], np.zeros(P - cout_pad, np.float32)])
    return want


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_conv_pack_under_sanitizers(tmp_path):
    exe = tmp_path / "harness"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        str(REPO / "mvlm_amd/csrc/conv_pack.cpp"), str(REPO / "tests/native/conv_pack_harness.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rs = np.random.RandomState(11)
    layers = []
    with open(tmp_path / "cases.pack", "wb") as f:
        for ksize, cin, cout, has_bias in CASES:
            w = (rs.standard_normal((cout, cin, ksize, ksize)) / np.sqrt(cin * ksize * ksize)).astype(np.float32)
            bias = rs.standard_normal(cout).astype(np.float32) if has_bias else None
            layers.append((w, bias))
            f.write(struct.pack("<IIII", ksize, cin, cout, int(has_bias)) + w.tobytes() + (bias.tobytes() if has_bias else b""))
    table = _padding_table()
    (tmp_path / "padding.txt").write_text("".join(" ".join(map(str, row)) + "\n" for row in table))
    r = subprocess.run([str(exe), str(tmp_path / "cases.pack"), str(tmp_path / "blobs.pack"), str(tmp_path / "padding.txt")], capture_output=True,
                       text=True, env={"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "INVARIANT" not in r.stdout
    assert f"padding rows {len(table)}\n" in r.stdout
    # 4 values of cin_pad x 2 kernel sizes x the cout_pad the timing hook's rule gives for 1..130 channels: whole 32s, 80 and 84
    assert {row[-1] for row in table if row[0] == 1} == {32, 64, 80, 84, 96, 128, 160} and "arenas 56\n" in r.stdout
    data, p = (tmp_path / "blobs.pack").read_bytes(), 0
    for (ksize, cin, cout, has_bias), (w, bias) in zip(CASES, layers):
        name = f"k{ksize} {cin}->{cout} bias {has_bias}"
        want = _expected(ksize, cin, cout, w, bias)
        cin_pad, cout_pad, n = struct.unpack_from("<III", data, p)
        offs = dict(zip(("w", "bias", "f23", "f43", "f43_pad", "bias_pad"), struct.unpack_from("<6q", data, p + 12)))
        blob = np.frombuffer(data, np.float32, n, p + 60)
        p += 60 + 4 * n
        assert (cin_pad, cout_pad) == want.pop("dims"), name
        assert {k for k, off in offs.items() if off >= 0} == set(want), name
        assert all(off % 4 == 0 for off in offs.values() if off >= 0), (name, offs)
        covered = np.zeros(n, bool)
        for key, arr in want.items():
            got = blob[offs[key]:offs[key] + arr.size]
            assert got.size == arr.size and np.array_equal(_bits(got), _bits(arr).ravel()), (name, key)
            assert not covered[offs[key]:offs[key] + arr.size].any(), (name, key, "overlaps another array")
            covered[offs[key]:offs[key] + arr.size] = True
        assert not blob[~covered].view(np.uint32).any(), (name, "the gaps between the arrays are zeros")
    assert p == len(data)
