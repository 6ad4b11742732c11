"""The pictures the PNG encoder's tests share (tests/test_png_model_cpu.py, tests/test_png_pack_sanitized.py,
tests/test_gpu_png_encode.py): the edge and boundary shapes, the two pictures with a skewed histogram that force the length
limits, and the two 1024 x 1024 pictures rebuilt from a committed JPEG.  Each case is (name, uint8 [H,W,3], filter_mode)."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"


def _spread(counts: dict, total: int) -> np.ndarray:
    """`total` bytes in which value v occurs counts[v] times (the first value takes what is left over), every value's
    occurrences spread evenly, so that equal neighbours - runs - stay rare."""
    counts = dict(counts)
    first = next(iter(counts))
    counts[first] += total - sum(counts.values())
    assert counts[first] > 0
    keys = np.concatenate([np.full(f, v) for v, f in counts.items()])
    where = np.concatenate([(np.arange(f) + 0.5) / f for f in counts.values()])
    return keys[np.argsort(where, kind="stable")].astype(np.uint8)


def fibonacci_picture() -> np.ndarray:
    """144 x 75 under filter_mode 0 (144 rows of 1 + 225 bytes, within one segment): the literal histogram with the end-of-block
    symbol's 1 is 1, 1, 2, 3, 5, ... 10946 - the 144 is the rows' type byte 0 - so that the unlimited Huffman tree is a chain
    of depth 20; the most frequent value takes the bytes left over."""
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    fib.remove(144)  # (the type bytes)
    counts = {200 - k: f for k, f in enumerate(reversed(fib))}  # (the most frequent value first: it takes the remainder)
    return _spread(counts, 144 * 225).reshape(144, 75, 3)


def code_length_picture() -> np.ndarray:
    """128 x 85 under filter_mode 0 (one full segment): the byte values 0..139 with power-of-two counts for which the literal
    code has 3, 5, 8, 21, 13, 34, 56 codes of the lengths 2, 5, 8, 9, 11, 12, 13 (Kraft sum 1; the 128 type bytes are value 0's
    whole count).  The end-of-block symbol splits one code of length 13 into two of 14, the zeros above 139 are one symbol 18
    and the absent distance code one 0: the code lengths' own histogram is 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, which an unlimited
    code answers with 9 bits.  Values of equal length are kept apart, so that the repeat symbol 16 does not collapse them."""
    per_length = {2: 3, 5: 5, 8: 8, 9: 21, 11: 13, 12: 34, 13: 56}
    lengths = np.concatenate([np.full(n, l) for l, n in per_length.items()])
    where = np.concatenate([(np.arange(n) + 0.5) / n for n in per_length.values()])
    lengths = lengths[np.argsort(where, kind="stable")]  # the lengths of the byte values 0, 1, 2, ...
    k = int(np.flatnonzero(lengths == 8)[0])
    lengths[0], lengths[k] = lengths[k], lengths[0]  # value 0: the 128 type bytes
    counts = {v: 1 << (15 - int(l)) for v, l in enumerate(lengths)}
    counts[0] -= 128
    order = sorted(counts, key=lambda v: -counts[v])
    return _spread({v: counts[v] for v in order if counts[v]}, 128 * 255).reshape(128, 85, 3)


@functools.lru_cache(maxsize=None)
def big_pictures():
    """The two 1024 x 1024 pictures the encoder was sized on: "textured", a crop of a scanner texture under a smooth light
    inside an ellipse on white, and "grey", the ellipse filled with the light alone."""
    from PIL import Image

    tex = np.asarray(Image.open(GOLDEN / "jpeg" / "real" / "angry_01.jpg").convert("RGB"))
    S = 1024
    y, x = np.mgrid[0:S, 0:S]
    inside = ((x - 512) ** 2 / 300 ** 2 + (y - 512) ** 2 / 420 ** 2) < 1
    crop = tex[600:600 + S, 1000:1000 + S]
    light = np.clip(1 - ((x - 512) ** 2 + (y - 512) ** 2) / 700.0 ** 2, 0, 1)[..., None]
    textured = np.full((S, S, 3), 255, np.uint8)
    textured[inside] = (crop * light).astype(np.uint8)[inside]
    grey = np.full((S, S, 3), 255, np.uint8)
    grey[inside] = (np.repeat(light, 3, 2) * 230).astype(np.uint8)[inside]
    textured.setflags(write=False)
    grey.setflags(write=False)
    return textured, grey


@functools.lru_cache(maxsize=None)
def small_cases():
    rng = np.random.default_rng(20261019)

    def noise(h, w, hi=256):
        return rng.integers(0, hi, (h, w, 3), dtype=np.uint8)

    cases = [
        ("1x1", noise(1, 1), -1),
        ("1x87", noise(1, 87), -1),
        ("7x12_black_run259", np.zeros((7, 12, 3), np.uint8), -1),
        ("65x1_black_run260", np.zeros((65, 1, 3), np.uint8), -1),
        ("6x14_black_run258", np.zeros((6, 14, 3), np.uint8), -1),
        ("128x85_one_segment", noise(128, 85, 6), 0),
        ("129x85_one_row_over", noise(129, 85, 6), 0),
        ("2049x5_white", np.full((2049, 5, 3), 255, np.uint8), -1),
        ("2049x5_run_over_boundary", np.concatenate([noise(2040, 5, 6), np.zeros((9, 5, 3), np.uint8)]), 0),
        ("64x64_white", np.full((64, 64, 3), 255, np.uint8), -1),
        ("64x64_noise", noise(64, 64), -1),
        ("fibonacci", fibonacci_picture(), 0),
        ("code_lengths", code_length_picture(), 0),
        ("37x53_smooth", (np.add.outer(np.arange(37) * 3, np.arange(53) * 2)[..., None] + np.array([0, 40, 90])).astype(np.uint8), -1),
    ]
    for _, im, _ in cases:
        im.setflags(write=False)
    return tuple(cases)


def big_cases():
    textured, grey = big_pictures()
    return (("textured_1024", textured, -1), ("grey_1024", grey, -1))
