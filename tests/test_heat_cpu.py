"""The heat sheet without a GPU: tests/heat_model.py against closed forms, and the checks the wrapper and the pipeline make before
any GPU work."""
import ctypes as C
import types
from pathlib import Path

import numpy as np
import pytest

import heat_model as hm
import sheet_model as sm


def _black(n=1):
    return np.zeros((n, 256, 256, 4), np.float32)


# ---- the model against closed forms ------------------------------------------------------------------------------------------
def test_peaks_are_the_largest_finite_value_or_minus_infinity():
    heat = np.zeros((6, 256, 256), np.float32)
    heat[0, 17, 200] = 3.5
    heat[1] = np.nan
    heat[2] = -2.0
    heat[2, 0, 0] = -1.5
    heat[3, 5, 5], heat[3, 6, 6], heat[3, 7, 7] = np.inf, 2.0, -np.inf
    heat[4] = -0.0
    heat[5] = np.inf
    got = hm.peaks(heat)
    assert got.dtype == np.float32 and got.shape == (6,)
    assert got[0] == 3.5 and got[1] == -np.inf and got[2] == -1.5 and got[3] == 2.0 and got[5] == -np.inf
    assert got[4] == 0.0 and np.signbit(got[4])
    assert hm.peaks(heat.reshape(2, 3, 256, 256)).shape == (2, 3)


def test_a_single_one_on_black_gives_exactly_the_opacity_of_the_colour_there_and_nothing_elsewhere():
    heat = np.zeros((1, 1, 256, 256), np.float32)
    heat[0, 0, 40, 99] = 1.0                                     # [row, col]
    colours = np.array([[200, 100, 40]], np.uint8)
    for floor in (0.25, 0.0, 0.5):
        sheet = hm.render(_black(), heat, colors=colours, gap=2, floor=floor, opacity=0.75)
        assert sheet.shape == (260, 260, 3)
        cell = sheet[2:258, 2:258]
        assert tuple(cell[40, 99]) == (150, 75, 30)              # row 40, column 99 of the image: 0.75 of the colour, exactly
        rest = np.ones((256, 256), bool)
        rest[40, 99] = False
        assert (cell[rest] == 0).all()                           # t = 0 <= floor, also at floor 0
    sheet = hm.render(_black(), heat, gap=0, opacity=1.0)        # the default colour: red; t = 1 at full opacity is the colour
    assert tuple(sheet[40, 99]) == hm.RED and int(sheet.astype(np.int64).sum()) == 255
    sheet = hm.render(_black(), heat, colors=colours, gap=1, scale=2)
    assert sheet.shape == (514, 514, 3)
    assert (sheet[81:83, 199:201] == (150, 75, 30)).all() and int((sheet[1:513, 1:513] != 0).any(axis=2).sum()) == 4


def test_a_share_equal_to_the_floor_draws_nothing_and_above_it_the_opacity_grows_linearly():
    heat = np.zeros((1, 1, 256, 256), np.float32)
    heat[0, 0, 0, 0] = 1.0
    heat[0, 0, 0, 1] = 0.25                                      # t == floor
    heat[0, 0, 0, 2] = 0.5                                       # a = 0.75 * 0.25 / 0.75 = 0.25
    heat[0, 0, 0, 3] = -0.5                                      # a negative share never draws
    images = _black()
    images[0, 0, :4, :3] = 100.0 / 255.0
    sheet = hm.render(images, heat, colors=[[200, 200, 0]], gap=0, floor=0.25, opacity=0.75)
    assert tuple(sheet[0, 0]) == (175, 175, 25)                  # 100 + 0.75 * (200 - 100), 100 + 0.75 * (0 - 100)
    assert tuple(sheet[0, 1]) == (100, 100, 100)
    assert tuple(sheet[0, 2]) == (125, 125, 75)                  # 100 + 0.25 * 100, 100 - 0.25 * 100
    assert tuple(sheet[0, 3]) == (100, 100, 100)
    np.testing.assert_array_equal(sheet[1:], sm.render(images, gap=0)[1:])


def test_the_lowest_index_wins_a_tie_and_the_larger_share_wins_otherwise():
    heat = np.zeros((1, 3, 256, 256), np.float32)
    heat[0, 0, 10, 10], heat[0, 0, 10, 11] = 2.0, 1.0            # shares 1, 0.5
    heat[0, 1, 10, 10], heat[0, 1, 10, 11], heat[0, 1, 10, 12] = 4.0, 2.0, 3.0   # shares 1, 0.5, 0.75: ties with landmark 0 twice
    heat[0, 2, 10, 12], heat[0, 2, 10, 13] = 8.0, 7.9            # share 1 beats landmark 1's 0.75
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    sheet = hm.render(_black(), heat, colors=colours, gap=0, floor=0.0, opacity=1.0)
    assert tuple(sheet[10, 10]) == (255, 0, 0) and tuple(sheet[10, 11]) == (128, 0, 0)       # landmark 0 keeps both ties
    assert tuple(sheet[10, 12]) == (0, 0, 255)
    win, t = hm.winners(heat[0], np.ones(3, bool), 0.0)
    assert win[10, 10] == 0 and win[10, 11] == 0 and win[10, 12] == 2 and win[10, 13] == 2 and win[0, 0] == -1
    assert t[10, 11] == 0.5 and t[10, 12] == 1.0
    # the order the landmarks are named in does not matter: ascending index
    np.testing.assert_array_equal(hm.render(_black(), heat, landmarks=[2, 1, 0], colors=colours, gap=0, floor=0.0, opacity=1.0), sheet)
    # without landmark 0 the tie is gone: landmark 1 shows
    sheet = hm.render(_black(), heat, landmarks=[1, 2], colors=colours, gap=0, floor=0.0, opacity=1.0)
    assert tuple(sheet[10, 10]) == (0, 255, 0) and tuple(sheet[10, 11]) == (0, 128, 0)


def test_unselected_nan_nonpositive_and_infinite_planes():
    rs = np.random.RandomState(5)
    images = rs.randint(0, 256, (2, 256, 256, 4)).astype(np.float32) / np.float32(255.0)
    plain = sm.render(images, gap=2)
    heat = np.zeros((2, 4, 256, 256), np.float32)
    heat[:, 0] = np.nan                                          # no finite value: peak -inf
    heat[:, 1] = -rs.uniform(0, 1, (2, 256, 256)).astype(np.float32)   # all <= 0
    heat[:, 1, 3, 3] = 0.0
    heat[:, 2, 100:120, 100:120] = 1.0                           # a real blob, deselected below
    heat[:, 3, 50, 50], heat[:, 3, 50, 51], heat[:, 3, 50, 52] = np.inf, 2.0, 1.0
    np.testing.assert_array_equal(hm.render(images, heat, landmarks=[0, 1]), plain)
    np.testing.assert_array_equal(hm.render(images, heat, landmarks=[]), plain)
    sheet = hm.render(images, heat, landmarks=[0, 1, 3], colors=np.full((4, 3), 255, np.uint8), floor=0.25, opacity=1.0)
    changed = (sheet != plain).any(axis=2)
    # +inf is skipped by the peak (2.0) and draws nothing itself; 2.0 is the peak (white), 1.0 is half of it: a = 1 / 3
    assert (sheet[2 + 50, 2 + 50] == plain[2 + 50, 2 + 50]).all() and (sheet[2 + 50, 2 + 51] == 255).all()
    bg = plain[2 + 50, 2 + 52].astype(np.float64)
    a = 1.0 * (0.5 - 0.25) / (1.0 - 0.25)
    assert tuple(sheet[2 + 50, 2 + 52]) == tuple(int(b + a * (255.0 - b) + 0.5) for b in bg)
    changed[2 + 50, 2 + 51:2 + 53] = changed[2 + 50, 260 + 51:260 + 53] = False
    assert not changed.any()                                     # and nothing else, in either view
    assert (hm.render(images, heat) != plain).any(axis=2).sum() >= 2 * 400 - 2   # all landmarks: the blob shows too


def test_the_layout_and_the_background_are_the_view_sheets():
    rs = np.random.RandomState(6)
    images = rs.randint(0, 256, (3, 256, 256, 4)).astype(np.float32) / np.float32(255.0)
    heat = np.full((3, 1, 256, 256), -1.0, np.float32)
    for kw in (dict(), dict(cols=1, gap=0), dict(scale=2, background="depth"), dict(cols=2, gap=5, scale=3)):
        np.testing.assert_array_equal(hm.render(images, heat, **kw), sm.render(images, **kw))


# ---- the wrapper's checks that need no GPU ---------------------------------------------------------------------------------------
def _stub_renderer():
    from mvlm_amd.utils.render3d import HipRenderer3D

    r = object.__new__(HipRenderer3D)
    r.ctx = types.SimpleNamespace(device=0)                      # no context: reaching the library would fail with AttributeError
    return r


def test_the_wrapper_refuses_bad_arguments_before_any_gpu_work():
    r = _stub_renderer()
    images, heat = np.zeros((2, 256, 256, 4), np.float32), np.zeros((2, 3, 256, 256), np.float32)
    for kw in (dict(floor=1.0), dict(floor=-0.1), dict(floor=float("nan")), dict(floor="x"), dict(opacity=0.0), dict(opacity=1.5),
               dict(opacity=float("inf")), dict(background="red"), dict(landmarks=[0, 0]), dict(landmarks=[0.5]), dict(landmarks=3),
               dict(landmarks=[True]), dict(scale=0), dict(scale=5), dict(scale=1.5), dict(gap=17), dict(gap=-1), dict(cols=0),
               dict(cols=True)):
        with pytest.raises(ValueError, match="^heat sheet:"):
            r.render_heat_sheet_device(images, heat, **kw)
        with pytest.raises(ValueError, match="^heat sheet:"):
            r.render_heat_sheet(images, heat, **kw)
    for bad_images in (np.zeros((2, 256, 256, 3), np.float32), np.zeros((0, 256, 256, 4), np.float32), np.zeros((256, 256, 4), np.float32),
                       [["a"]]):
        with pytest.raises(ValueError, match="^heat sheet: images"):
            r.render_heat_sheet_device(bad_images, heat)
    with pytest.raises(ValueError, match="^heat sheet: .*4096"):
        r.render_heat_sheet_device(np.zeros((17, 256, 256, 4), np.float32), heat, cols=17)
    with pytest.raises(ValueError, match="^heat sheet: .*largest scale that fits is 3"):
        r.render_heat_sheet_device(np.zeros((4, 256, 256, 4), np.float32), heat, cols=1, scale=4)


def test_the_c_abi_is_declared_and_bound():
    from mvlm_amd import _lib

    header = (Path(__file__).resolve().parents[1] / "include" / "mvlm_hip.h").read_text()
    for name in ("mvlm_heat_plane_peaks", "mvlm_render_heat_sheet", "mvlm_heat_sheet_stage_ms"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
        assert getattr(_lib.load(), name).restype is C.c_int
    assert _lib.SIGNATURES["mvlm_heat_sheet_stage_ms"] == (C.c_int, [C.c_void_p, _lib.c_float_p])
    assert len(_lib.SIGNATURES["mvlm_render_heat_sheet"][1]) == 14 and len(_lib.SIGNATURES["mvlm_heat_plane_peaks"][1]) == 4


# ---- the pipeline's checks that need no GPU ------------------------------------------------------------------------------------
def test_pipeline_constructor_checks():
    from mvlm_amd import pipeline

    with pytest.raises(ValueError, match="^heat sheet: .*largest scale that fits is 1"):
        pipeline.create_pipeline("dtu3d", n_views=96, weights="synthetic:5", visualize_heat=True, sheet_scale=2)
    for bad in (0, 5, 1.5, "2", True):
        with pytest.raises(ValueError, match="sheet_scale"):
            pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", visualize_heat=True, sheet_scale=bad)
    for bad in ([0, 0], [-1], [1.5], "3", 3, [True]):
        with pytest.raises(ValueError, match="heat_landmarks"):
            pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", visualize_heat=True, heat_landmarks=bad)
    for bad in (1.0, -0.5, float("nan"), "0.3", True):
        with pytest.raises(ValueError, match="heat_floor"):
            pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", visualize_heat=True, heat_floor=bad)


class _Heatmaps:
    def __init__(self, nl=73):
        self.nl = nl

    def get_lm_count(self):
        return self.nl

    def heatmaps_device(self, images):  # pragma: no cover - never reached here
        raise AssertionError("GPU work")


def _stub_pipeline(**attrs):
    from mvlm_amd.pipeline import DTU3DPipeline
    from mvlm_amd.utils.render3d import HipRenderer3D

    pipe = object.__new__(DTU3DPipeline)
    pipe.__dict__.update(dict(visualize_img=False, visualize_rays_img=False, visualize_sheet=False, visualize_heat=True,
                              heat_landmarks=None, shard_views=False, renderer_3d=object.__new__(HipRenderer3D),
                              predictor_2d=_Heatmaps(), estimator_3d=object()), **attrs)
    return pipe


def test_a_predictor_without_heatmaps_is_refused(tmp_path):
    from mvlm_amd.prediction import PrecomputedPredictor

    _stub_pipeline()._check_visualize()
    pipe = _stub_pipeline(predictor_2d=PrecomputedPredictor(5, fn=lambda images: None))
    with pytest.raises(ValueError, match="visualize_heat needs a predictor with heatmaps_device"):
        pipe._check_visualize()
    with pytest.raises(ValueError, match="heatmaps_device"):      # the first thing a prediction does
        pipe.predict_one_file(tmp_path / "missing.obj")
    with pytest.raises(ValueError, match="heatmaps_device"):
        next(pipe.predict_files([tmp_path / "missing.obj"]))
    with pytest.raises(ValueError, match="heatmaps_device"):
        pipe.predict_mesh_device.__wrapped__(pipe, None, np.zeros((8, 6)))
    _stub_pipeline(predictor_2d=object(), visualize_heat=False)._check_visualize()


def test_another_renderer_a_sharded_run_and_landmarks_out_of_range_are_refused(monkeypatch, tmp_path):
    from mvlm_amd import parallel

    with pytest.raises(ValueError, match="visualize_heat needs a HipRenderer3D"):
        _stub_pipeline(renderer_3d=object())._check_visualize()
    _stub_pipeline(heat_landmarks=[0, 72])._check_visualize()
    pipe = _stub_pipeline(heat_landmarks=[0, 73])
    with pytest.raises(ValueError, match=r"heat_landmarks must lie in 0\.\.72"):
        pipe._check_visualize()
    with pytest.raises(ValueError, match="heat_landmarks"):
        pipe.predict_one_file(tmp_path / "missing.obj")
    pipe = _stub_pipeline(shard_views=True)
    pipe._check_visualize()                                      # not distributed: one process holds every view
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    with pytest.raises(ValueError, match="visualize_heat is not supported with shard_views"):
        pipe._check_visualize()
    with pytest.raises(ValueError, match="shard_views"):
        pipe.predict_mesh_device.__wrapped__(pipe, None, np.zeros((8, 6)))


def test_the_path_helper_the_palette_and_the_command_line():
    from mvlm_amd.__main__ import build_parser
    from mvlm_amd.utils.viewer import HEAT_PALETTE, heat_colours, heat_sheet_path

    assert heat_sheet_path("/data/scans/face_01.obj", "dtu3d") == Path("visualization") / "face_01_dtu3d_heat.png"
    assert heat_sheet_path("face.obj") == Path("visualization") / "face_heat.png"
    colours = heat_colours(84)
    assert colours.dtype == np.uint8 and colours.shape == (84, 3) and len(set(HEAT_PALETTE)) == len(HEAT_PALETTE) >= 6
    assert all(tuple(colours[l]) == HEAT_PALETTE[l % len(HEAT_PALETTE)] for l in range(84))
    assert all(tuple(colours[l]) != tuple(colours[l + 1]) for l in range(83))       # neighbours differ
    args = build_parser().parse_args(["-p", "x.obj", "--visualize-heat", "--heat-landmarks", "3,17,40", "--heat-floor", "0.4",
                                      "--sheet-scale", "2"])
    assert args.visualize_heat and args.heat_landmarks == [3, 17, 40] and args.heat_floor == 0.4 and args.sheet_scale == 2
    args = build_parser().parse_args(["-p", "x.obj"])
    assert not args.visualize_heat and args.heat_landmarks is None and args.heat_floor == 0.25
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-p", "x.obj", "--heat-landmarks", "3,x"])
