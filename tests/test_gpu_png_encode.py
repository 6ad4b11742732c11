"""-m gpu: mvlm_png_encode against the model of its contract (tests/png_model.py, itself held against zlib and Pillow by
tests/test_png_model_cpu.py) - the device's files equal the model's byte for byte on every edge case, under every filter mode
and for several pictures in one call; a view drawn on the device and encoded there decodes to the host path's pixels; every
refusal names "png:" and launches nothing."""
import ctypes as C
import io

import numpy as np
import pytest

import png_cases
import png_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderer():
    from mvlm_amd.utils.render3d import HipRenderer3D

    return HipRenderer3D(n_views=1)


def _device(images):
    import torch

    rgb = np.stack(images)
    alpha = np.arange(rgb.shape[1] * rgb.shape[2], dtype=np.uint8).reshape(1, rgb.shape[1], rgb.shape[2], 1)  # (dropped)
    rgba = np.concatenate([rgb, np.broadcast_to(alpha, rgb.shape[:3] + (1,))], axis=3)
    return torch.from_numpy(np.ascontiguousarray(rgba)).cuda()


@pytest.fixture(scope="module")
def model_files():
    """The model's file of every case, computed once."""
    return {name: png_model.encode(im, mode)[0] for name, im, mode in png_cases.small_cases() + png_cases.big_cases()}


def _first_difference(a: bytes, b: bytes):
    n = min(len(a), len(b))
    x, y = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    d = np.flatnonzero(x != y)
    return f"sizes {len(a)} / {len(b)}, first differing byte {int(d[0]) if len(d) else n}"


@pytest.mark.parametrize("index", range(len(png_cases.small_cases())), ids=[c[0] for c in png_cases.small_cases()])
def test_edge_cases_equal_the_model(renderer, model_files, index):
    name, im, mode = png_cases.small_cases()[index]
    got, = renderer.encode_png(_device([im]), filter_mode=mode)
    assert len(got) <= renderer.png_bound(*im.shape[:2])
    assert got == model_files[name], _first_difference(got, model_files[name])


@pytest.mark.parametrize("index", range(2), ids=["textured_1024", "grey_1024"])
def test_the_1024_pictures_equal_the_model(renderer, model_files, index):
    name, im, mode = png_cases.big_cases()[index]
    got, = renderer.encode_png(_device([im]), filter_mode=mode)
    assert got == model_files[name], _first_difference(got, model_files[name])


def test_three_pictures_in_one_call_equal_three_calls(renderer):
    rng = np.random.default_rng(5)
    smooth = (np.add.outer(np.arange(150) * 2, np.arange(131))[..., None] + np.array([0, 85, 170])).astype(np.uint8)
    images = [smooth, rng.integers(0, 256, (150, 131, 3), dtype=np.uint8), np.full((150, 131, 3), 255, np.uint8)]
    together = renderer.encode_png(_device(images))
    assert len(together) == 3 and len({len(f) for f in together}) == 3
    for im, f in zip(images, together):
        single, = renderer.encode_png(_device([im]))
        assert f == single
        assert f == png_model.encode(im)[0]


@pytest.mark.parametrize("mode", range(5))
def test_every_forced_filter_equals_the_model(renderer, mode):
    textured, _ = png_cases.big_pictures()
    im = np.ascontiguousarray(textured[400:531, 300:497])  # 131 x 197: the ellipse's edge, three segments
    got, = renderer.encode_png(_device([im]), filter_mode=mode)
    want = png_model.encode(im, mode)[0]
    assert got == want, _first_difference(got, want)


@pytest.mark.parametrize("size", (64, 256))
def test_a_view_encoded_on_the_device_decodes_to_the_host_view(renderer, size):
    from PIL import Image
    from test_planted_cpu import planted_scene

    mesh, pts, _, _ = planted_scene(n_views=8)
    want = renderer.render_landmark_view(mesh, pts, size=size)
    view = renderer.render_landmark_view_device(mesh, pts, size=size)
    png, = renderer.encode_png(view)
    renderer.check()
    Image.open(io.BytesIO(png)).verify()
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert got.shape == (size, size, 3) and (got != 255).any()
    np.testing.assert_array_equal(got, want[0])
    assert png == png_model.encode(want[0])[0]


def test_stage_times_need_profiling_and_come_with_it(renderer):
    ctx = renderer.ctx
    im = png_cases.small_cases()[5][1]
    renderer.encode_png(_device([im]))
    with pytest.raises(Exception, match="png_stage_ms"):
        renderer.png_stage_ms()
    ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 1))
    try:
        renderer.encode_png(_device([im]))
        ms = renderer.png_stage_ms()
    finally:
        ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 0))
    assert ms.shape == (4,) and np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0


def test_refusals_name_png_and_launch_nothing(renderer):
    import torch

    ctx, lib = renderer.ctx, renderer.ctx.lib
    n = C.c_size_t()
    assert lib.mvlm_png_bound(1, 1, C.byref(n)) == 0 and n.value == 4 + 10 + 63
    assert lib.mvlm_png_bound(4096, 4096, C.byref(n)) == 0 and n.value == png_model.png_bound(4096, 4096)
    for h, w in ((0, 5), (5, 0), (4097, 5), (5, 4097), (-1, -1)):
        assert lib.mvlm_png_bound(h, w, C.byref(n)) != 0
    assert lib.mvlm_png_bound(5, 5, None) != 0

    h, w = 9, 7
    bound = renderer.png_bound(h, w)
    canary = 0xA5
    pixels = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")
    host = np.full((2, bound), canary, np.uint8)
    sizes = (C.c_size_t * 2)(7, 7)
    ctx.bind_current_stream(torch, pixels.device)

    def call(rgba=pixels.data_ptr(), n_images=2, height=h, width=w, mode=-1, out=host.ctypes.data, stride=bound, sz=sizes):
        return lib.mvlm_png_encode(ctx.handle, C.c_void_p(rgba), n_images, height, width, mode, C.c_void_p(out), C.c_size_t(stride), sz)

    refused = (dict(rgba=None), dict(out=None), dict(sz=None), dict(n_images=0), dict(n_images=-3), dict(n_images=129),
               dict(height=0), dict(width=0), dict(height=4097), dict(width=4097), dict(mode=-2), dict(mode=5),
               dict(stride=bound - 1), dict(stride=0), dict(n_images=9, height=2048, width=2048, stride=1 << 40))
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.mvlm_last_error(ctx.handle).decode().startswith("png:"), (kw, lib.mvlm_last_error(ctx.handle))
    torch.cuda.synchronize()
    assert (host == canary).all() and list(sizes) == [7, 7]      # nothing was written
    assert call() == 0
    assert all(0 < s <= bound for s in sizes) and (host[:, :8] == np.frombuffer(b"\x89PNG\r\n\x1a\n", np.uint8)).all()
    with pytest.raises(ValueError, match="png:"):
        renderer.encode_png(pixels, filter_mode=7)
    with pytest.raises(ValueError, match="png:"):
        renderer.encode_png(pixels.cpu())
    with pytest.raises(ValueError, match="png:"):
        renderer.encode_png(pixels[..., :3])
