"""-m gpu: HipRenderer3D.render_view_sheet against tests/sheet_model.py - zero differing bytes, no tolerance: layouts, both
backgrounds, one and several staging rounds of landmarks, marker placement, rings, residuals, refusals."""
import ctypes as C

import numpy as np
import pytest

import sheet_model as sm

pytestmark = pytest.mark.gpu

POSES = np.array([[0, 0, 0, 0, 0, 0], [30, 15, 0, 0, 0, 0], [-25, -70, 12, 0, 0, 0], [10, 45, -20, 0, 0, 0], [-38, 5, 3, 0, 0, 0]], np.float64)


@pytest.fixture(scope="module")
def r3():
    from mvlm_amd.utils.render3d import HipRenderer3D

    return HipRenderer3D(n_views=8, verbose=False)


@pytest.fixture(scope="module")
def stack():
    """Five views of random k / 255 values in all four planes (read-only)."""
    rs = np.random.RandomState(11)
    images = rs.randint(0, 256, (5, 256, 256, 4)).astype(np.float32) / np.float32(255.0)
    images.setflags(write=False)
    return images


def _rot(n):
    from mvlm_amd.utils.render3d import view_rotations

    return np.ascontiguousarray(view_rotations(POSES[:n]), dtype=np.float64).reshape(n, 3, 3)


def _scene(n, nl, seed):
    """maxima [NL,N,3] in and around the cell, landmarks whose projections lie in and around it, colours, survivor flags."""
    rs = np.random.RandomState(seed)
    maxima = np.empty((nl, n, 3), np.float32)
    maxima[:, :, :2] = rs.uniform(-8, 264, (nl, n, 2))
    maxima[:, :, 2] = rs.uniform(0, 1, (nl, n))
    landmarks = rs.uniform(-160, 160, (nl, 3))
    colors = rs.randint(0, 256, (nl, 3)).astype(np.uint8)
    used = (rs.uniform(size=(nl, n)) > 0.35).astype(np.uint8)
    return maxima, landmarks, colors, used


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    differing = int((got != want).sum())
    print(f"{what}: {differing} differing bytes of {want.size}")
    assert differing == 0, what


# n_views, cols, scale, gap, background, n_landmarks: every value of the issue's list in at least one row; cols 1 and N; 257 > one
# staging round of 256; gap 3 so that no tile aligns with the sheet
BASE = [(1, None, 1, 0, "rgb", 1), (1, 1, 2, 3, "depth", 84), (2, None, 1, 3, "rgb", 257), (2, 1, 2, 0, "depth", 1),
        (3, None, 2, 3, "rgb", 84), (3, 3, 1, 0, "depth", 257), (3, 1, 1, 3, "rgb", 84), (5, None, 1, 3, "depth", 84),
        (5, 5, 1, 0, "rgb", 257), (5, 1, 2, 3, "rgb", 1), (5, None, 2, 0, "depth", 257), (2, 2, 2, 3, "rgb", 257)]


@pytest.mark.parametrize("n,cols,scale,gap,background,nl", BASE)
def test_sheet_equals_the_model(r3, stack, n, cols, scale, gap, background, nl):
    maxima, landmarks, colors, used = _scene(n, nl, seed=100 + n + nl)
    kw = dict(maxima=maxima, rot=_rot(n), landmarks=landmarks, colors=colors, used=used, background=background, cols=cols,
              scale=scale, gap=gap)
    got = r3.render_view_sheet(stack[:n], **kw)
    _same(got, sm.render(stack[:n], **kw), f"N={n} cols={cols} scale={scale} gap={gap} {background} NL={nl}")
    c, r, w, h = sm.layout(n, cols, scale, gap)
    assert got.shape == (h, w, 3)
    if c * r > n:  # the last row is partly empty: grey
        side = 256 * scale
        y0, x0 = gap + (n // c) * (side + gap), gap + (n % c) * (side + gap)
        assert (got[y0:y0 + side, x0:x0 + side] == 128).all()


def _placement_maxima(n):
    """(a, b) such that the marker (X = b, Y = a + 1) stands on pixel centres, pixel corners, every border and corner of the cell,
    outside it, and nowhere (NaN / inf)."""
    spots = [(100.5, 60.5), (30.0, 200.0), (77.25, 13.75),                                    # centre, corner, in between
             (0.0, 100.5), (256.0, 100.5), (100.5, 0.0), (100.5, 256.0),                      # on the four borders
             (0.0, 0.0), (256.0, 0.0), (0.0, 256.0), (256.0, 256.0),                          # on the four corners
             (0.5, 0.5), (255.5, 255.5), (0.5, 255.5), (255.5, 0.5),                          # the corner pixels' centres
             (-1.5, 128.5), (257.5, 128.5), (128.5, -2.0), (128.5, 258.0),                    # outside, the rim reaching in
             (-40.0, 50.0), (300.0, 300.0), (1e6, 20.0), (50.0, -3e7),                        # far outside
             (150.5, 150.5), (150.5, 150.5), (152.5, 150.5)]                                  # twice the same spot, and an overlap
    xy = np.array(spots, np.float64)
    nl = len(spots) + 4
    maxima = np.zeros((nl, n, 3), np.float32)
    maxima[:len(spots), :, 0] = (xy[:, 1] - 1.0)[:, None]   # a = Y - 1
    maxima[:len(spots), :, 1] = xy[:, 0][:, None]           # b = X
    maxima[:, :, 2] = 0.5
    maxima[len(spots):, :, :2] = 64.5
    maxima[len(spots), :, 0] = np.nan
    maxima[len(spots) + 1, :, 1] = np.inf
    maxima[len(spots) + 2, :, 2] = np.nan
    maxima[len(spots) + 3, :, 2] = -np.inf
    return maxima, len(spots)


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("radius", [0.5, 2.0, 16.0])
def test_marker_placement_rings_and_radii(r3, stack, scale, radius):
    n = 2
    maxima, n_spots = _placement_maxima(n)
    nl = maxima.shape[0]
    colors = np.stack([np.arange(nl) * 9 % 256, 255 - np.arange(nl) * 5 % 256, np.arange(nl) * 31 % 256], axis=1).astype(np.uint8)
    used = np.ones((nl, n), np.uint8)
    used[::2, 0] = 0       # rings and discs mixed: view 0 alternates, view 1 rings the second of the two on one spot
    used[n_spots - 2, 1] = 0
    kw = dict(maxima=maxima, colors=colors, used=used, scale=scale, gap=3, marker_radius=radius)
    got = r3.render_view_sheet(stack[:n], **kw)
    _same(got, sm.render(stack[:n], **kw), f"placement scale={scale} R={radius}")
    if radius <= 2.0:  # nothing of a non-finite prediction: the spot (64.5, 65.5) shows the background
        side = 256 * scale
        cell0 = got[3:3 + side, 3:3 + side]
        want_bg = (stack[0, 65, 64, :3] * 255 + 0.5).astype(np.uint8)
        assert tuple(cell0[int(65.5 * scale), int(64.5 * scale)]) == tuple(want_bg)


def test_of_two_markers_on_one_spot_the_later_wins(r3, stack):
    maxima = np.zeros((3, 1, 3), np.float32)
    maxima[:, 0, :2] = [(99.5, 40.5), (99.5, 40.5), (99.5, 43.5)]       # X = 40.5 twice, then 43.5; Y = 100.5
    colors = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    used = np.array([[1], [0], [1]], np.uint8)                         # the second one is a ring
    got = r3.render_view_sheet(stack[:1], maxima, colors=colors, used=used, gap=0)
    _same(got, sm.render(stack[:1], maxima, colors=colors, used=used, gap=0), "two on one spot")
    assert tuple(got[100, 40]) == (10, 20, 30)      # the ring's hole shows the first marker's disc
    assert tuple(got[100, 38]) == (40, 50, 60)      # the ring itself lies over it
    assert tuple(got[100, 42]) == (70, 80, 90)      # and the third marker over both
    both = r3.render_view_sheet(stack[:1], maxima[:2], colors=colors[:2], gap=0)
    assert tuple(both[100, 40]) == (40, 50, 60) and not (both == (10, 20, 30)).all(axis=2).any()


def test_default_colour_is_blue_and_all_are_used(r3, stack):
    maxima = np.array([[[99.5, 40.5, 1.0]]], np.float32)
    got = r3.render_view_sheet(stack[:1], maxima, gap=0)
    _same(got, sm.render(stack[:1], maxima, gap=0), "defaults")
    assert tuple(got[100, 40]) == (0, 0, 255) and int((got == (0, 0, 255)).all(axis=2).sum()) >= 13


@pytest.mark.parametrize("scale", [1, 2])
def test_residuals(r3, stack, scale):
    """Identity and two rotated poses; segments of every direction, some ending far outside the cell; a zero-length one; non-finite
    landmarks; a landmark so far away that its projection overflows."""
    n, nl = 3, 40
    rs = np.random.RandomState(7)
    maxima = np.empty((nl, n, 3), np.float32)
    maxima[:, :, :2] = rs.uniform(5, 250, (nl, n, 2))
    maxima[:, :, 2] = 1.0
    landmarks = rs.uniform(-150, 150, (nl, 3))
    landmarks[0] = [400.0, 0.0, 0.0]            # leaves every cell towards a neighbour
    landmarks[1] = [0.0, -900.0, 50.0]
    landmarks[2] = [np.nan, 0.0, 0.0]
    landmarks[3] = [0.0, np.inf, 0.0]
    landmarks[4] = [1e306, 1e306, 1e306]        # finite, its projection is not
    landmarks[5] = [1e12, -1e12, 0.0]           # finite and far
    # zero length under the identity: the landmark that projects onto its own marker (X = 40.5, Y = 20.5)
    maxima[6, 0, :2] = (19.5, 40.5)
    landmarks[6] = [40.5 * 300 / 256 - 150, (256 - 20.5) * 300 / 256 - 150, 0.0]
    maxima[7, :, 0] = np.nan                    # no marker: no residual either
    kw = dict(maxima=maxima, rot=_rot(n), landmarks=landmarks, scale=scale, gap=3)
    got = r3.render_view_sheet(stack[:n], **kw)
    _same(got, sm.render(stack[:n], **kw), f"residuals scale={scale}")
    assert (got == sm.RED).all(axis=2).sum() > 1000


def test_a_residual_never_shows_in_the_neighbouring_cell_or_the_gap(r3, stack):
    n = 2
    maxima = np.full((1, n, 3), np.nan, np.float32)
    maxima[0, 0] = (127.0, 200.5, 1.0)                       # X = 200.5, Y = 128; view 1 has no prediction
    landmarks = np.array([[600.0, 0.0, 0.0]])                # projects to Y' = 128, far to the right: through view 1's cell
    rot = np.tile(np.eye(3), (n, 1, 1))
    got = r3.render_view_sheet(stack[:n], maxima, rot, landmarks, cols=2, gap=3)
    _same(got, sm.render(stack[:n], maxima, rot, landmarks, cols=2, gap=3), "neighbour")
    plain = r3.render_view_sheet(stack[:n], cols=2, gap=3)
    np.testing.assert_array_equal(got[:, 3 + 256:], plain[:, 3 + 256:])     # the gap right of view 0 and all of view 1
    assert (got[3 + 127:3 + 129, 3 + 203:3 + 256] == sm.RED).all()          # ... while view 0 carries it to its border


def test_images_only_and_partial_inputs(r3, stack):
    for background in ("rgb", "depth"):
        got = r3.render_view_sheet(stack[:3], background=background)
        _same(got, sm.render(stack[:3], background=background), f"images only {background}")
    maxima, landmarks, _, _ = _scene(3, 5, seed=3)
    # rotations without landmarks, landmarks without rotations: markers, no residuals
    want = sm.render(stack[:3], maxima)
    _same(r3.render_view_sheet(stack[:3], maxima, rot=_rot(3)), want, "rot only")
    _same(r3.render_view_sheet(stack[:3], maxima, landmarks=landmarks), want, "landmarks only")
    # "auto": the planes the predictor read
    _same(r3.render_view_sheet(stack[:3], background="auto", chan_sel=[3]), sm.render(stack[:3], background="depth"), "auto depth")
    _same(r3.render_view_sheet(stack[:3], background="auto", chan_sel=[0, 1, 2, 3]), sm.render(stack[:3]), "auto rgb")
    _same(r3.render_view_sheet(stack[:3], background="auto"), sm.render(stack[:3]), "auto unknown")


def test_numpy_inputs_equal_tensor_inputs(r3, stack):
    import torch

    n, nl = 3, 84
    maxima, landmarks, colors, used = _scene(n, nl, seed=9)
    dev = torch.device("cuda", r3.ctx.device)
    a = r3.render_view_sheet(stack[:n], maxima, _rot(n), landmarks, colors, used, scale=2)
    out = r3.render_view_sheet_device(torch.from_numpy(stack[:n].copy()).to(dev), torch.from_numpy(maxima).to(dev),
                                      torch.from_numpy(_rot(n).copy()).to(dev), torch.from_numpy(landmarks).to(dev),
                                      torch.from_numpy(colors).to(dev), torch.from_numpy(used).to(dev), scale=2)
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == a.shape[:2] + (4,)
    b = out.cpu().numpy()
    r3.check()
    assert (b[..., 3] == 255).all()
    np.testing.assert_array_equal(b[..., :3], a)
    files = r3.encode_png(out)                      # the layout encode_png takes
    assert len(files) == 1 and files[0][:8] == b"\x89PNG\r\n\x1a\n"


def test_python_refusals(r3, stack):
    import torch

    maxima, landmarks, colors, used = _scene(2, 4, seed=1)
    ok = stack[:2]
    bad_calls = [
        lambda: r3.render_view_sheet(np.zeros((2, 128, 128, 4), np.float32)),
        lambda: r3.render_view_sheet(np.zeros((256, 256, 4), np.float32)),
        lambda: r3.render_view_sheet(np.zeros((0, 256, 256, 4), np.float32)),
        lambda: r3.render_view_sheet(torch.zeros((2, 256, 256, 4), dtype=torch.float64, device="cuda")),
        lambda: r3.render_view_sheet(torch.zeros((2, 256, 256, 4), dtype=torch.float32)),                      # a host tensor
        lambda: r3.render_view_sheet(ok, maxima[:, :1]),
        lambda: r3.render_view_sheet(ok, maxima[..., :2]),
        lambda: r3.render_view_sheet(ok, torch.from_numpy(maxima).double().cuda()),
        lambda: r3.render_view_sheet(ok, maxima, rot=np.zeros((3, 3, 3))),
        lambda: r3.render_view_sheet(ok, maxima, rot=np.full((2, 3, 3), np.nan), landmarks=landmarks),
        lambda: r3.render_view_sheet(ok, maxima, landmarks=landmarks[:3]),
        lambda: r3.render_view_sheet(ok, maxima, colors=colors[:3]),
        lambda: r3.render_view_sheet(ok, maxima, used=used[:, :1]),
        lambda: r3.render_view_sheet(ok, maxima, background="heat"),
        lambda: r3.render_view_sheet(ok, maxima, marker_radius=0.25),
        lambda: r3.render_view_sheet(ok, maxima, marker_radius=16.5),
        lambda: r3.render_view_sheet(ok, maxima, marker_radius=float("nan")),
        lambda: r3.render_view_sheet(ok, cols=0),
        lambda: r3.render_view_sheet(ok, scale=0),
        lambda: r3.render_view_sheet(ok, scale=5),
        lambda: r3.render_view_sheet(ok, gap=17),
        lambda: r3.render_view_sheet(ok, gap=-1),
        lambda: r3.render_view_sheet(ok, cols=1, scale=4, gap=16),     # 2 x 1024 + 3 x 16 fits; ...
    ]
    for k, call in enumerate(bad_calls[:-1]):
        with pytest.raises(ValueError):
            call()
        assert k >= 0
    assert bad_calls[-1]().shape == (2 * 1024 + 48, 1024 + 32, 3)
    with pytest.raises(ValueError, match="largest scale that fits is 3"):   # ... five in a row at scale 4 do not
        r3.render_view_sheet(stack, cols=5, scale=4)
    _same(r3.render_view_sheet(ok, maxima), sm.render(ok, maxima), "after the refusals")


def test_every_refusal_of_the_library_sets_the_error_and_launches_nothing(r3, stack):
    import torch

    from mvlm_amd import _lib

    ctx, lib = r3.ctx, r3.ctx.lib
    dev = torch.device("cuda", ctx.device)
    n, nl = 2, 3
    images = torch.from_numpy(stack[:n].copy()).to(dev)
    maxima_np, landmarks, _, _ = _scene(n, nl, seed=2)
    maxima = torch.from_numpy(maxima_np).to(dev)
    _, _, w, h = sm.layout(n)
    out = torch.full((h, w, 4), 7, dtype=torch.uint8, device=dev)
    rot = np.ascontiguousarray(_rot(n).reshape(n, 9))
    bad_rot = rot.copy()
    bad_rot[1, 4] = np.inf
    ctx.bind_current_stream(torch, dev)

    def call(images_p=images.data_ptr(), n_views=n, n_lm=nl, rot_h=rot, background=0, cols=0, scale=1, gap=2, radius=2.0,
             out_p=out.data_ptr()):
        return lib.mvlm_render_view_sheet(ctx.handle, C.c_void_p(images_p), n_views, C.c_void_p(maxima.data_ptr()), n_lm,
                                          _lib.as_ptr(rot_h, C.c_double), _lib.as_ptr(landmarks, C.c_double), None, None, background,
                                          cols, scale, gap, C.c_double(radius), C.c_void_p(out_p))

    refusals = [dict(images_p=None), dict(out_p=None), dict(n_views=0), dict(n_views=-1), dict(n_lm=-1), dict(n_lm=65537),
                dict(rot_h=bad_rot), dict(background=2), dict(background=-1), dict(cols=-1), dict(scale=0), dict(scale=5),
                dict(gap=-1), dict(gap=17), dict(radius=0.49), dict(radius=16.01), dict(radius=float("nan")),
                dict(radius=float("inf")), dict(n_views=96, scale=2)]
    for kw in refusals:
        assert call(**kw) != 0, kw
        msg = lib.mvlm_last_error(ctx.handle).decode()
        assert msg.startswith("view sheet:"), (kw, msg)
        if kw == dict(n_views=96, scale=2):
            assert "largest scale that fits is 1" in msg
    torch.cuda.synchronize()
    assert bool((out == 7).all())                       # nothing was launched
    assert call() == 0                                  # ... and the context renders correctly afterwards
    got = out.cpu().numpy()
    r3.check()
    _same(got[..., :3], sm.render(stack[:n], maxima_np, rot, landmarks), "after the library's refusals")
