"""The PNG encoder's contract as tests/png_model.py states it, held against Pillow and zlib - never against itself or the
device code: every case decodes to its pixels with valid chunk CRCs, its IDAT inflates to the model's filtered stream (which
checks Adler-32 too), the file fits mvlm_png_bound; the adaptive filter gives Pillow's filtered stream on the two 1024 x 1024
pictures; the two skewed pictures really exceed the length limits without the limiter; and the IDAT is no larger than
zlib's own Z_RLE stream over the same filtered bytes times SIZE_BOUND (profiles/png_encode_size.txt holds the measured ratios:
the largest is 1.0039 on 2049x5_white, rounded up to 1.01, plus 0.02 for later changes of tie-breaking)."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

import png_cases
import png_model

SIZE_BOUND = 1.03
CASES = png_cases.small_cases() + png_cases.big_cases()


@pytest.fixture(scope="module")
def encoded():
    """(file, filtered stream, per-segment records) of every case, computed once."""
    out = {}
    for name, im, mode in CASES:
        info = []
        png, stream, _ = png_model.encode(im, mode, info)
        out[name] = (png, stream, info)
    return out


def z_rle(stream: bytes) -> int:
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(stream) + c.flush())


def pillow_filtered_stream(im) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(im).save(b, "PNG")
    return zlib.decompress(png_model.idat_of(b.getvalue()))


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0] for c in CASES])
def test_format_and_size(encoded, index):
    from PIL import Image

    from mvlm_amd import _lib

    name, im, mode = CASES[index]
    png, stream, info = encoded[name]
    decoded = Image.open(io.BytesIO(png))
    decoded.load()
    assert decoded.mode == "RGB" and np.array_equal(np.asarray(decoded), im)
    Image.open(io.BytesIO(png)).verify()                      # chunk CRCs
    idat = png_model.idat_of(png)
    assert idat[:2] == b"\x78\x01" and zlib.decompress(idat) == stream   # (and Adler-32)
    h, w = im.shape[:2]
    assert len(stream) == h * (1 + 3 * w) and len(info) == -(-len(stream) // png_model.SEGMENT)
    bound = C.c_size_t()
    assert _lib.load().mvlm_png_bound(h, w, C.byref(bound)) == 0 and bound.value == png_model.png_bound(h, w)
    assert len(png) <= bound.value
    ratio = len(idat) / z_rle(stream)
    print(f"{name}: IDAT {len(idat)} B, zlib Z_RLE {z_rle(stream)} B, ratio {ratio:.4f}")
    assert ratio <= SIZE_BOUND


def test_the_filter_rule_gives_pillows_stream_on_the_1024_pictures(encoded):
    for name, im, _ in png_cases.big_cases():
        assert encoded[name][1] == pillow_filtered_stream(im), name


def test_forced_filters_invert():
    from PIL import Image

    im = np.ascontiguousarray(png_cases.big_pictures()[0][380:420, 280:345])
    for mode in range(5):
        png, stream, _ = png_model.encode(im, mode)
        assert set(stream[::1 + 3 * im.shape[1]]) == {mode}
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), im)


def test_block_kinds_and_run_boundaries(encoded):
    kinds = {name: [r["kind"] for r in info] for name, (_, _, info) in encoded.items()}
    assert kinds["64x64_noise"] == [0] and kinds["1x87"] == [0]                # stored
    assert kinds["128x85_one_segment"] == [2] and len(kinds["129x85_one_row_over"]) == 2
    assert len(kinds["2049x5_white"]) == 2 and len(kinds["2049x5_run_over_boundary"]) == 2  # 32 784 bytes
    stream = encoded["2049x5_run_over_boundary"][1]              # under filter 0 the last nine rows are one run of 144 zeros
    assert stream[-144:] == bytes(144) and stream[-145] != 0     # which the boundary cuts: 128 before it, 16 behind
    _, lengths = png_model.tokenize(np.frombuffer(stream[png_model.SEGMENT:], np.uint8))
    assert lengths.tolist() == [0, 15]
    _, lengths = png_model.tokenize(np.frombuffer(stream[:png_model.SEGMENT], np.uint8))
    assert lengths[-2:].tolist() == [0, 127]
    # the black pictures are one run: a literal, then 258 + nothing, 258 + a literal, 257
    for name, total, matches, literals in (("7x12_black_run259", 259, [258], 1), ("65x1_black_run260", 260, [258], 2),
                                            ("6x14_black_run258", 258, [257], 1)):
        stream = np.frombuffer(encoded[name][1], np.uint8)
        assert len(stream) == total and not stream.any()
        _, lengths = png_model.tokenize(stream)
        assert [int(x) for x in lengths if x] == matches and int((lengths == 0).sum()) == literals


def test_the_skewed_pictures_need_the_limits(encoded):
    (rec,) = encoded["fibonacci"][2]
    assert max(png_model.unlimited_depths(rec["ll_freq"]).values()) > 15       # (20: not vacuous)
    assert max(rec["ll_lens"]) == 15 and rec["kind"] == 2
    (rec,) = encoded["code_lengths"][2]
    assert max(png_model.unlimited_depths(rec["cl_freq"]).values()) > 7        # (9)
    assert max(rec["cl_lens"]) == 7 and rec["kind"] == 2
    for name in ("fibonacci", "code_lengths"):
        (rec,) = encoded[name][2]
        for lens, limit in ((rec["ll_lens"], 15), (rec["cl_lens"], 7)):
            assert sum(2.0 ** -l for l in lens if l) == 1.0 and max(lens) <= limit   # a complete code


def test_the_bound_is_refused_out_of_range():
    for h, w in ((0, 1), (1, 0), (4097, 1), (1, 4097)):
        with pytest.raises(ValueError, match="png:"):
            png_model.png_bound(h, w)
    assert png_model.png_bound(1, 1) == 77
