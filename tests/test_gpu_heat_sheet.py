"""-m gpu: mvlm_heat_plane_peaks against a numpy maximum over finite values - bit for bit - and HipRenderer3D.render_heat_sheet
against tests/heat_model.py - zero differing bytes, no tolerance: layouts, both backgrounds, blobs in the centre and the corners,
ties, dead planes, a deselected landmark, refusals."""
import ctypes as C

import numpy as np
import pytest

import heat_model as hm
import sheet_model as sm

pytestmark = pytest.mark.gpu

PLANE = 256 * 256


@pytest.fixture(scope="module")
def r3():
    from mvlm_amd.utils.render3d import HipRenderer3D

    return HipRenderer3D(n_views=8, verbose=False)


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    differing = int((got != want).sum())
    print(f"{what}: {differing} differing bytes of {want.size}")
    assert differing == 0, what


# ---- mvlm_heat_plane_peaks -------------------------------------------------------------------------------------------------------
def _peak_planes():
    """12 planes [12, 65536]: noise in [-1, 0.5) with the maximum 0.75 planted where the reduction could lose it, and the planes
    without an ordinary maximum."""
    rs = np.random.RandomState(21)
    planes = rs.uniform(-1.0, 0.5, (12, PLANE)).astype(np.float32)
    word = 4 * 12345
    share = 1024 * 5 + 256 * 2          # a thread reads 16 bytes, a wave 256 floats in a row, the workgroup 1024 per round
    spots = [0, PLANE - 1, word + 1, word + 2, word + 3, share, share + 255]   # element 0 is also position 0 of its 16-byte word
    for p, k in enumerate(spots):
        planes[p, k] = 0.75
    planes[7, 255] = planes[7, 256] = 0.75                  # on a wave boundary: the last float of wave 0, the first of wave 1
    planes[8] = np.nan
    planes[9] = np.nan                                      # the only finite value is negative
    planes[9, ::3] = np.inf
    planes[9, 1::5] = -np.inf
    planes[9, 40000] = -3.25
    planes[10, 100], planes[10, 60000], planes[10, 33333] = np.inf, -np.inf, np.nan   # beside the finite maximum 0.75 at 200
    planes[10, 200] = 0.75
    planes[11] = -0.0
    return planes


def test_plane_peaks_equal_numpys_maximum_over_finite_values_bit_for_bit(r3):
    import torch

    ctx, lib = r3.ctx, r3.ctx.lib
    dev = torch.device("cuda", ctx.device)
    planes = _peak_planes()
    want = hm.peaks(planes.reshape(12, 256, 256))
    assert list(want[:8]) == [0.75] * 8 and want[8] == -np.inf and want[9] == -3.25 and want[10] == 0.75
    assert want[11] == 0 and np.signbit(want[11])
    heat = torch.from_numpy(planes).to(dev)
    peaks = torch.full((12,), 7.0, dtype=torch.float32, device=dev)
    ctx.bind_current_stream(torch, dev)
    ctx.check(lib.mvlm_heat_plane_peaks(ctx.handle, C.c_void_p(heat.data_ptr()), 12, C.c_void_p(peaks.data_ptr())))
    got = peaks.cpu().numpy()
    print("peaks:", got.tolist())
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # refusals: the error names the heat sheet and nothing is written
    peaks.fill_(7.0)
    for heat_p, n_planes, peaks_p in ((None, 12, peaks.data_ptr()), (heat.data_ptr(), 12, None), (heat.data_ptr(), 0, peaks.data_ptr()),
                                      (heat.data_ptr(), -1, peaks.data_ptr()), (heat.data_ptr(), 32769, peaks.data_ptr()),
                                      (heat.data_ptr() + 4, 11, peaks.data_ptr())):
        assert lib.mvlm_heat_plane_peaks(ctx.handle, C.c_void_p(heat_p), n_planes, C.c_void_p(peaks_p)) != 0
        assert lib.mvlm_last_error(ctx.handle).decode().startswith("heat sheet:")
    torch.cuda.synchronize()
    assert bool((peaks == 7.0).all())


# ---- mvlm_render_heat_sheet ------------------------------------------------------------------------------------------------------
N, NL = 3, 6
COLOURS = np.array([[255, 0, 0], [0, 230, 40], [30, 60, 255], [250, 220, 0], [255, 0, 255], [0, 200, 200]], np.uint8)


def _blob(cy, cx, sigma, amplitude):
    y, x = np.mgrid[0:256, 0:256].astype(np.float64)
    return (amplitude * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma))).astype(np.float32)


@pytest.fixture(scope="module")
def scene(r3):
    """(images numpy, heat numpy, images on the device, heat on the device): 3 views, 6 landmarks, read-only."""
    import torch

    rs = np.random.RandomState(31)
    images = rs.randint(0, 256, (N, 256, 256, 4)).astype(np.float32) / np.float32(255.0)
    heat = np.zeros((N, NL, 256, 256), np.float32)
    for v in range(N):
        heat[v, 0] = _blob(128, 128, 9.0, 0.9 - 0.2 * v) + rs.uniform(-0.01, 0.01, (256, 256)).astype(np.float32)   # the centre
        heat[v, 1] = _blob(0, 0, 7.0, 0.6) + _blob(255, 255, 7.0, 0.5 + 0.05 * v)                                   # the corners
        heat[v, 2] = _blob(80, 150 + 10 * v, 8.0, 0.4)
        # twice landmark 2 - the same share t of its own peak on every pixel of that blob, bit for bit - and a weaker blob of its own
        heat[v, 3] = np.float32(2.0) * heat[v, 2] + _blob(200, 60, 6.0, 0.5)
        heat[v, 4] = np.nan
        heat[v, 5] = -rs.uniform(0.0, 1.0, (256, 256)).astype(np.float32)
        heat[v, 5, 9, 9] = 0.0
    heat[2, 0, 128, 130], heat[2, 0, 126, 128], heat[2, 0, 120, 120] = np.nan, np.inf, -np.inf   # holes in a live plane
    assert float(hm.peaks(heat[0, 3])) == 2.0 * float(hm.peaks(heat[0, 2]))
    images.setflags(write=False)
    heat.setflags(write=False)
    dev = torch.device("cuda", r3.ctx.device)
    return images, heat, torch.from_numpy(images.copy()).to(dev), torch.from_numpy(heat.copy()).to(dev)


CASES = [(scale, gap, cols, background) for scale in (1, 2) for gap in (0, 2) for cols in (None, 1) for background in ("rgb", "depth")]


@pytest.mark.parametrize("scale,gap,cols,background", CASES)
def test_heat_sheet_equals_the_model(r3, scene, scale, gap, cols, background):
    images, heat, images_dev, heat_dev = scene
    k = CASES.index((scale, gap, cols, background))
    deselected = (2, 0, 1, 3)[k % 4]                       # one landmark is left out: a tie partner, the centre, the corners, ...
    kw = dict(landmarks=[l for l in range(NL) if l != deselected], colors=COLOURS, background=background, cols=cols, scale=scale,
              gap=gap, floor=(0.25, 0.1)[k % 2], opacity=(0.75, 1.0)[k // 8])
    got = r3.render_heat_sheet(images_dev, heat_dev, **kw)
    want = hm.render(images, heat, **kw)
    _same(got, want, f"scale={scale} gap={gap} cols={cols} {background} without landmark {deselected}")
    c, r, w, h = sm.layout(N, cols, scale, gap)
    assert got.shape == (h, w, 3)
    plain = sm.render(images, background=background, cols=cols, scale=scale, gap=gap)
    assert (want != plain).any()                           # the heat shows ...
    if cols is None:                                       # ... and the fourth cell of two columns is empty: grey
        side = 256 * scale
        assert (got[gap + side + gap:gap + 2 * side + gap, gap + side + gap:gap + 2 * side + gap] == 128).all()


def test_ties_dead_planes_corners_and_the_deselected_landmark(r3, scene):
    images, heat, images_dev, heat_dev = scene
    kw = dict(colors=COLOURS, gap=0, cols=1, floor=0.25, opacity=1.0)
    full = r3.render_heat_sheet(images_dev, heat_dev, **kw)
    _same(full, hm.render(images, heat, **kw), "all landmarks")
    assert tuple(full[80, 150]) == tuple(COLOURS[2])       # t = 1 for landmarks 2 and 3 alike: the lower index shows
    assert tuple(full[0, 0]) == tuple(COLOURS[1])          # the corner pixels carry the corner blobs' peaks
    without2 = r3.render_heat_sheet(images_dev, heat_dev, landmarks=[0, 1, 3, 4, 5], **kw)
    assert tuple(without2[80, 150]) == tuple(COLOURS[3])
    only_dead = r3.render_heat_sheet(images_dev, heat_dev, landmarks=[4, 5], **kw)
    _same(only_dead, sm.render(images, gap=0, cols=1), "the NaN plane and the non-positive plane draw nothing")
    # numpy arrays are uploaded, lists of colours and the default colour are taken
    got = r3.render_heat_sheet(images, heat, landmarks=(0,), gap=0, cols=1)
    _same(got, hm.render(images, heat, landmarks=[0], gap=0, cols=1), "numpy inputs, default colour")
    assert tuple(got[128, 128]) == tuple(hm.render(images, heat[:, :1], gap=0, cols=1)[128, 128])


def test_with_every_landmark_deselected_the_output_is_the_view_sheet(r3, scene):
    images, heat, images_dev, heat_dev = scene
    for kw in (dict(), dict(scale=2, gap=3, background="depth"), dict(cols=3, gap=0)):
        got = r3.render_heat_sheet(images_dev, heat_dev, landmarks=[], **kw)
        _same(got, r3.render_view_sheet(images_dev, **kw), f"no landmark selected, {kw}")
    device = r3.render_heat_sheet_device(images_dev, heat_dev, landmarks=[])
    assert str(device.dtype) == "torch.uint8" and tuple(device.shape) == (518, 518, 4) and bool((device[..., 3] == 255).all())


def test_stage_times_need_profiling_and_come_with_it(r3, scene):
    _, _, images_dev, heat_dev = scene
    ctx = r3.ctx
    r3.render_heat_sheet(images_dev, heat_dev)
    with pytest.raises(Exception, match="heat_sheet_stage_ms"):
        r3.heat_sheet_stage_ms()
    ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 1))
    try:
        r3.render_heat_sheet(images_dev, heat_dev)
        ms = r3.heat_sheet_stage_ms()
    finally:
        ctx.check(ctx.lib.mvlm_render_set_profiling(ctx.handle, 0))
    print("background, peak, compose [ms]:", ms.tolist())
    assert ms.shape == (3,) and np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses_bad_arguments(r3, scene):
    import torch

    images, heat, images_dev, heat_dev = scene
    bad_calls = [
        lambda: r3.render_heat_sheet(images_dev[0], heat_dev),
        lambda: r3.render_heat_sheet(images_dev.double(), heat_dev),
        lambda: r3.render_heat_sheet(images_dev.cpu(), heat_dev),
        lambda: r3.render_heat_sheet(images_dev, heat_dev[:2]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev[:, :, :128]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev.double()),
        lambda: r3.render_heat_sheet(images_dev, heat_dev.cpu()),
        lambda: r3.render_heat_sheet(images_dev, heat_dev[:, :0]),
        lambda: r3.render_heat_sheet(images_dev, np.zeros((N, 256, 256), np.float32)),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, landmarks=[6]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, landmarks=[-1]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, landmarks=[1, 1]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, landmarks=[0.5]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, colors=COLOURS[:5]),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, colors="red"),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, background="heat"),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, floor=1.0),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, floor=-0.01),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, floor=float("nan")),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, opacity=0.0),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, opacity=1.01),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, opacity=float("inf")),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, cols=0),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, scale=0),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, scale=5),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, gap=17),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, gap=-1),
        lambda: r3.render_heat_sheet(images_dev, heat_dev, cols=1, scale=4, gap=16),      # 3 x 1024 + 4 x 16 fits; ...
    ]
    for k, call in enumerate(bad_calls[:-1]):
        with pytest.raises(ValueError, match="^heat sheet:"):
            call()
        assert k >= 0
    assert bad_calls[-1]().shape == (3 * 1024 + 64, 1024 + 32, 3)
    with pytest.raises(ValueError, match="^heat sheet: .*largest scale that fits is 3"):     # ... four in a column at scale 4 do not
        r3.render_heat_sheet(torch.zeros((4, 256, 256, 4), device=images_dev.device), torch.zeros((4, 1, 256, 256), device=images_dev.device),
                             cols=1, scale=4)
    _same(r3.render_heat_sheet(images_dev, heat_dev), hm.render(images, heat), "after the refusals")


def test_every_refusal_of_the_library_sets_the_error_and_launches_nothing(r3, scene):
    import torch

    from mvlm_amd import _lib

    images, heat, images_dev, heat_dev = scene
    ctx, lib = r3.ctx, r3.ctx.lib
    dev = torch.device("cuda", ctx.device)
    _, _, w, h = sm.layout(N)
    out = torch.full((h, w, 4), 7, dtype=torch.uint8, device=dev)
    sel = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    ctx.bind_current_stream(torch, dev)

    def call(images_p=images_dev.data_ptr(), heat_p=heat_dev.data_ptr(), n_views=N, n_lm=NL, background=0, cols=0, scale=1, gap=2,
             floor=0.25, opacity=0.75, out_p=out.data_ptr()):
        return lib.mvlm_render_heat_sheet(ctx.handle, C.c_void_p(images_p), C.c_void_p(heat_p), n_views, n_lm,
                                          _lib.as_ptr(sel, C.c_uint8), _lib.as_ptr(COLOURS, C.c_uint8), background, cols, scale, gap,
                                          C.c_double(floor), C.c_double(opacity), C.c_void_p(out_p))

    refusals = [dict(images_p=None), dict(heat_p=None), dict(out_p=None), dict(heat_p=heat_dev.data_ptr() + 4), dict(n_views=0),
                dict(n_views=-1), dict(n_lm=0), dict(n_lm=-1), dict(n_lm=65537), dict(n_views=8, n_lm=4097), dict(n_views=1, n_lm=32769),
                dict(background=2), dict(background=-1), dict(cols=-1), dict(scale=0), dict(scale=5), dict(gap=-1), dict(gap=17),
                dict(floor=-0.01), dict(floor=1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(opacity=0.0),
                dict(opacity=1.01), dict(opacity=float("nan")), dict(opacity=-0.5), dict(n_views=96, scale=2)]
    for kw in refusals:
        assert call(**kw) != 0, kw
        msg = lib.mvlm_last_error(ctx.handle).decode()
        assert msg.startswith("heat sheet:"), (kw, msg)
        if kw == dict(n_views=96, scale=2):
            assert "largest scale that fits is 1" in msg
    torch.cuda.synchronize()
    assert bool((out == 7).all())                       # nothing was launched
    assert call() == 0                                  # ... and the context draws correctly afterwards
    got = out.cpu().numpy()
    r3.check()
    assert (got[..., 3] == 255).all()
    _same(got[..., :3], hm.render(images, heat, landmarks=[0, 1, 3, 4, 5], colors=COLOURS), "after the library's refusals")
