"""The view sheet without a GPU: mvlm_view_sheet_layout against tests/sheet_model.py, the model against closed forms and against
the reference estimator's own rays (tests/golden/marker_rays.npz), and the checks the pipeline makes before any GPU work."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import sheet_model as sm

GOLDEN = Path(__file__).parent / "golden"


def _c_layout(n, cols, scale, gap):
    from mvlm_amd import _lib

    out = [C.c_int(-1) for _ in range(4)]
    why = C.create_string_buffer(512)
    rc = _lib.load().mvlm_view_sheet_layout(n, cols, scale, gap, *[C.byref(o) for o in out], why, len(why))
    return rc, tuple(o.value for o in out), why.value.decode()


# ---- mvlm_view_sheet_layout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8, 96, 128])
def test_layout_equals_the_model(n):
    from mvlm_amd.utils.render3d import HipRenderer3D

    fits = 0
    for cols in (None, 1, 2, 5, n):
        for scale in (1, 2, 3, 4):
            for gap in (0, 2, 16):
                try:
                    want = sm.layout(n, cols, scale, gap)
                except ValueError:
                    want = None
                rc, got, why = _c_layout(n, 0 if cols is None else cols, scale, gap)
                if want is None:
                    assert rc != 0 and "4096" in why, (n, cols, scale, gap, got)
                    with pytest.raises(ValueError, match="4096"):
                        HipRenderer3D.view_sheet_layout(n, cols, scale, gap)
                else:
                    assert rc == 0 and got == want and why == "", (n, cols, scale, gap, got, want, why)
                    assert HipRenderer3D.view_sheet_layout(n, cols, scale, gap) == want
                    c, r, w, h = got
                    assert r == -(-n // c) and w == c * 256 * scale + (c + 1) * gap and h == r * 256 * scale + (r + 1) * gap
                    fits += 1
    assert fits > 0


def test_default_columns_are_the_ceiling_of_the_square_root():
    for n, cols in ((1, 1), (2, 2), (3, 2), (4, 2), (5, 3), (8, 3), (9, 3), (10, 4), (96, 10), (128, 12)):
        assert _c_layout(n, 0, 1, 2)[1][0] == cols == sm.layout(n)[0]


def test_layout_refusals():
    from mvlm_amd.utils.render3d import HipRenderer3D

    rc, _, why = _c_layout(96, 0, 2, 2)
    assert rc != 0 and "largest scale that fits is 1" in why, why
    with pytest.raises(ValueError, match="largest scale that fits is 1"):
        HipRenderer3D.view_sheet_layout(96, None, 2, 2)
    rc, _, why = _c_layout(128, 0, 4, 16)
    assert rc != 0 and "largest scale that fits is 1" in why, why
    rc, _, why = _c_layout(4, 1, 4, 2)           # one column of four rows: 4 x 1024 + gaps does not fit, scale 3 does
    assert rc != 0 and "largest scale that fits is 3" in why, why
    rc, _, why = _c_layout(20, 20, 1, 0)         # 20 columns never fit
    assert rc != 0 and "no scale fits" in why, why
    for n, cols, scale, gap, word in ((8, -1, 1, 2, "cols"), (8, 0, 0, 2, "scale"), (8, 0, 5, 2, "scale"), (8, 0, 1, -1, "gap"),
                                      (8, 0, 1, 17, "gap"), (0, 0, 1, 2, "n_views"), (-3, 0, 1, 2, "n_views")):
        rc, got, why = _c_layout(n, cols, scale, gap)
        assert rc != 0 and word in why and got == (-1, -1, -1, -1), (n, cols, scale, gap, why)
    # the public wrapper: cols is None (the default) or at least 1
    for kw in (dict(cols=0), dict(cols=-1), dict(scale=0), dict(scale=5), dict(gap=-1), dict(gap=17), dict(scale=1.5), dict(cols=True)):
        with pytest.raises(ValueError):
            HipRenderer3D.view_sheet_layout(8, **kw)
    with pytest.raises(ValueError):
        HipRenderer3D.view_sheet_layout(0)
    for kw in (dict(cols=0), dict(cols=-1), dict(scale=0), dict(scale=5), dict(gap=-1), dict(gap=17)):
        with pytest.raises(ValueError):
            sm.layout(8, **kw)
    with pytest.raises(ValueError):
        sm.layout(0)


# ---- the model against closed forms --------------------------------------------------------------------------------------------
def _disc(cx2, cy2, lo2, hi2, side, scale=1):
    """Pixels (i, j) of the cell with lo2 < 4 d^2 <= hi2, d from the centre (i + 0.5, j + 0.5) to (cx2 / 2, cy2 / 2): integers."""
    out = set()
    for j in range(side):
        for i in range(side):
            d = (2 * i + 1 - cx2) ** 2 + (2 * j + 1 - cy2) ** 2
            if lo2 < d <= hi2:
                out.add((i, j))
    return out


def test_a_marker_of_radius_2_on_a_pixel_centre_covers_13_pixels():
    got = sm.pixels(sm.marker_mask(10.5, 20.5, 2.0, 1))
    assert len(got) == 13
    assert got == {(10 + dx, 20 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy <= 4}


@pytest.mark.parametrize("x", [0.5, 128.5, 255.5])
@pytest.mark.parametrize("y", [0.5, 128.5, 255.5])
def test_a_marker_is_clipped_at_the_borders_and_corners_of_its_cell(x, y):
    got = sm.pixels(sm.marker_mask(x, y, 2.0, 1))
    i0, j0 = int(x - 0.5), int(y - 0.5)
    want = {(i0 + dx, j0 + dy) for dx in range(-2, 3) for dy in range(-2, 3)
            if dx * dx + dy * dy <= 4 and 0 <= i0 + dx < 256 and 0 <= j0 + dy < 256}
    assert got == want
    assert len(got) == {0: 13, 1: 9, 2: 6}[(x != 128.5) + (y != 128.5)]


def test_markers_outside_the_cell():
    assert sm.pixels(sm.marker_mask(-3.0, 100.0, 2.0, 1)) == set()
    assert sm.pixels(sm.marker_mask(100.0, 259.0, 2.0, 2)) == set()
    assert sm.pixels(sm.marker_mask(-1.5, 100.5, 2.0, 1)) == {(0, 100)}  # the disc's rim reaches the centre of column 0 (<=)


def test_the_ring_at_scale_1_and_2():
    # scale 1: 1 < d <= 2 around a pixel centre: the 13 pixels less the centre and its four neighbours
    got = sm.pixels(sm.marker_mask(10.5, 20.5, 2.0, 1, used=False))
    assert got == {(10 + dx, 20 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if 1 < dx * dx + dy * dy <= 4} and len(got) == 8
    # scale 2: R scale = 4, ring width max(1, 2) = 2: 2 < d <= 4 around (21, 41) sheet pixels
    got = sm.pixels(sm.marker_mask(10.5, 20.5, 2.0, 2, used=False))
    assert got == _disc(42, 82, 16, 64, 512) and got
    assert sm.pixels(sm.marker_mask(10.5, 20.5, 2.0, 2)) == _disc(42, 82, -1, 64, 512)
    # a ring wider than the disc is the disc: R = 0.5 at scale 1
    assert sm.pixels(sm.marker_mask(10.5, 20.5, 0.5, 1, used=False)) == sm.pixels(sm.marker_mask(10.5, 20.5, 0.5, 1)) == {(10, 20)}
    # inner radius exactly 0 (R = 1 at scale 1): the centre pixel alone is cut out
    assert sm.pixels(sm.marker_mask(10.5, 20.5, 1.0, 1, used=False)) == {(9, 20), (11, 20), (10, 19), (10, 21)}


def test_markers_on_pixel_corners():
    # on a corner the four pixels around it are nearest, at d^2 = 0.5; R = 2 reaches d^2 <= 4: 2 i' + 1 odd offsets
    got = sm.pixels(sm.marker_mask(10.0, 20.0, 2.0, 1))
    assert got == _disc(20, 40, -1, 16, 256) and len(got) == 12


def test_segments():
    # horizontal through pixel centres: the pixels it passes, none beside (their centres are 1 away) or beyond the ends
    assert sm.pixels(sm.segment_mask(10.5, 20.5, 30.5, 20.5, 1)) == {(i, 20) for i in range(10, 31)}
    # horizontal ON a pixel boundary: the centres of both rows are exactly 0.5 away (<=); the ends' centres are 0.5 inside
    assert sm.pixels(sm.segment_mask(10.0, 20.0, 30.0, 20.0, 1)) == {(i, j) for i in range(10, 30) for j in (19, 20)}
    # vertical, given end first
    assert sm.pixels(sm.segment_mask(7.5, 40.5, 7.5, 12.5, 1)) == {(7, j) for j in range(12, 41)}
    # 45 degrees through centres: the diagonal only (its neighbours are 0.707 away)
    assert sm.pixels(sm.segment_mask(10.5, 10.5, 20.5, 20.5, 1)) == {(i, i) for i in range(10, 21)}
    # scale 2, half width 1: (21, 41) -> (61, 41) sheet pixels covers rows 40 and 41, and the end caps reach one column out
    assert sm.pixels(sm.segment_mask(10.5, 20.5, 30.5, 20.5, 2)) == {(i, j) for i in range(20, 62) for j in (40, 41)}
    # clipped to the cell
    assert sm.pixels(sm.segment_mask(250.5, 3.5, 300.5, 3.5, 1)) == {(i, 3) for i in range(250, 256)}
    assert sm.pixels(sm.segment_mask(-40.0, 3.5, -2.0, 3.5, 1)) == set()


def test_a_zero_length_segment_is_a_dot():
    assert sm.pixels(sm.segment_mask(10.5, 20.5, 10.5, 20.5, 1)) == {(10, 20)}
    assert sm.pixels(sm.segment_mask(10.5, 20.5, 10.5, 20.5, 2)) == _disc(42, 82, -1, 4, 512)
    assert sm.pixels(sm.segment_mask(10.0, 20.0, 10.0, 20.0, 1)) == set()  # on a corner every centre is 0.707 away


def test_render_composes_background_residuals_and_markers_in_that_order():
    rs = np.random.RandomState(0)
    images = (rs.randint(0, 256, (3, 256, 256, 4)).astype(np.float32) / np.float32(255.0))
    maxima = np.zeros((2, 3, 3), np.float32)
    maxima[0, :, :2] = (19.5, 10.5)     # a = 19.5 -> Y = 20.5; b = 10.5 -> X = 10.5
    maxima[1, :, :2] = (19.5, 12.5)     # overlaps landmark 0's marker
    maxima[1, 2, 2] = np.nan            # no marker, no residual in view 2
    rot = np.tile(np.eye(3).ravel(), (3, 1))
    # identity: X' = (x + 150) * 256 / 300, Y' = 256 - (y + 150) * 256 / 300; choose the landmark that projects to (40.5, 20.5)
    lm = np.array([[40.5 * 300 / 256 - 150, (256 - 20.5) * 300 / 256 - 150, 7.0], [np.nan, 0.0, 0.0]])
    assert sm.project(rot[0], lm[0]) == pytest.approx((40.5, 20.5), abs=1e-12)
    colors = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    sheet = sm.render(images, maxima, rot, lm, colors=colors, cols=2, scale=1, gap=3)
    assert sheet.shape == (2 * 256 + 9, 2 * 256 + 9, 3) and sm.layout(3, 2, 1, 3) == (2, 2, 521, 521)
    want = (images[..., :3] * 255 + 0.5).astype(np.uint8)
    for v, (y0, x0) in enumerate(((3, 3), (3, 262), (262, 3))):
        cell = sheet[y0:y0 + 256, x0:x0 + 256]
        marked = np.zeros((256, 256), bool)
        d0 = {(10 + dx, 20 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy <= 4}
        d1 = {(12 + dx, 20 + dy) for dx in range(-2, 3) for dy in range(-2, 3) if dx * dx + dy * dy <= 4} if v != 2 else set()
        seg = {(i, 20) for i in range(10, 41)}
        for i, j in seg:
            marked[j, i] = True
            if (i, j) not in d0 | d1:
                assert tuple(cell[j, i]) == sm.RED
        for i, j in d0 - d1:
            assert tuple(cell[j, i]) == (1, 2, 3)
        for i, j in d1:                                     # the later landmark wins the overlap
            assert tuple(cell[j, i]) == (4, 5, 6)
        for i, j in d0 | d1:
            marked[j, i] = True
        np.testing.assert_array_equal(cell[~marked], want[v][~marked])
    grey = np.ones((521, 521), bool)
    for y0, x0 in ((3, 3), (3, 262), (262, 3)):
        grey[y0:y0 + 256, x0:x0 + 256] = False
    assert (sheet[grey] == 128).all()                       # gaps and the empty fourth cell
    depth = sm.render(images, background="depth", scale=2, gap=0)
    assert depth.shape == (1024, 1024, 3)
    np.testing.assert_array_equal(depth[:512, 512:, 1], np.repeat(np.repeat((images[1, :, :, 3] * 255 + 0.5).astype(np.uint8), 2, 0), 2, 1))
    assert sm.auto_background([0, 1, 2, 3]) == "rgb" and sm.auto_background([3]) == "depth" and sm.auto_background([2]) == "rgb"


def test_the_marker_stands_where_the_reference_estimators_ray_pierces_the_image():
    """estimator3d.py:73-78 read backwards: every point of the ray the REFERENCE estimator spans for (a, b) in a view projects, by
    the residual's formulas, onto the marker's position - to 1e-9 view pixels."""
    from oracle.estimator import view_rotation

    g = np.load(GOLDEN / "marker_rays.npz")
    lms, s, e, poses = g["corner_lms"], g["corner_s"], g["corner_e"], g["poses"]
    worst = 0.0
    for v in range(lms.shape[1]):
        m = view_rotation(*poses[v, :3]).ravel()
        for l in range(lms.shape[0]):
            x, y = sm.marker_position(lms[l, v, 0], lms[l, v, 1])
            for t in (0.0, 0.37, 1.0):
                xp, yp = sm.project(m, s[l, v] + t * (e[l, v] - s[l, v]))
                worst = max(worst, abs(xp - x), abs(yp - y))
    assert worst <= 1e-9, worst
    # the reference drawer's int() truncation is NOT that point: it lands up to a pixel off
    a, b = float(lms[0, 0, 0]), float(lms[0, 0, 1])
    assert sm.marker_position(a, b) == (b, a + 1.0)


# ---- the pipeline's checks that need no GPU ------------------------------------------------------------------------------------
def test_pipeline_constructor_checks():
    from mvlm_amd import pipeline

    with pytest.raises(ValueError, match="largest scale that fits is 1"):
        pipeline.create_pipeline("dtu3d", n_views=96, weights="synthetic:5", visualize_sheet=True, sheet_scale=2)
    for bad in (0, 5, 1.5, "2", True):
        with pytest.raises(ValueError, match="sheet_scale"):
            pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", visualize_sheet=True, sheet_scale=bad)


def _stub_pipeline(**attrs):
    from mvlm_amd.pipeline import DTU3DPipeline
    from mvlm_amd.utils.render3d import HipRenderer3D

    pipe = object.__new__(DTU3DPipeline)
    pipe.__dict__.update(dict(visualize_img=False, visualize_rays_img=False, visualize_sheet=True, shard_views=False,
                              renderer_3d=object.__new__(HipRenderer3D), predictor_2d=object(), estimator_3d=object()), **attrs)
    return pipe


def test_a_sharded_run_is_refused_before_any_gpu_work(monkeypatch, tmp_path):
    from mvlm_amd import parallel

    pipe = _stub_pipeline(shard_views=True)
    pipe._check_visualize()                                   # not distributed: one process holds every view
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    with pytest.raises(ValueError, match="shard_views"):
        pipe._check_visualize()
    with pytest.raises(ValueError, match="shard_views"):      # the first thing a prediction does
        pipe.predict_one_file(tmp_path / "missing.obj")
    with pytest.raises(ValueError, match="shard_views"):
        next(pipe.predict_files([tmp_path / "missing.obj"]))
    with pytest.raises(ValueError, match="shard_views"):
        pipe.predict_mesh_device.__wrapped__(pipe, None, np.zeros((8, 6)))
    _stub_pipeline(shard_views=True, visualize_sheet=False)._check_visualize()


def test_another_renderer_in_the_slot_is_refused():
    pipe = _stub_pipeline(renderer_3d=object())
    with pytest.raises(ValueError, match="visualize_sheet needs a HipRenderer3D"):
        pipe._check_visualize()


def test_the_path_helper_and_the_command_line():
    from mvlm_amd.__main__ import build_parser
    from mvlm_amd.utils.viewer import view_sheet_path

    assert view_sheet_path("/data/scans/face_01.obj", "dtu3d") == Path("visualization") / "face_01_dtu3d_views.png"
    assert view_sheet_path("face.obj") == Path("visualization") / "face_views.png"
    args = build_parser().parse_args(["-p", "x.obj", "--visualize-sheet", "--sheet-scale", "2"])
    assert args.visualize_sheet and args.sheet_scale == 2
    args = build_parser().parse_args(["-p", "x.obj"])
    assert not args.visualize_sheet and args.sheet_scale == 1
