"""The surface heat without a GPU: tests/backproject_model.py against hand-computed cases - three vertices, two views, a constant
depth plane, two landmarks, one case per rule of the contract ("Surface heat") -, the C ABI's new entries, the
command line's flags, and the rules the pipeline checks before any GPU work.

The hand computation.  View 0 is the identity, view 1 a half turn about y (x -> -x, z -> -z).  A vertex (x, y, z) lies at window
x = (x + 150) * 256 / 300 pixels: x = 0 -> 128.0, x = 30 -> 153.6, x = -30 -> 102.4, x = 200 -> 298.7 (outside); y = 0 -> j = 128,
image row 255 - 128 = 127.  Its z-buffer value is (500 - z) / 1500: z = 50 -> 0.3 -> trunc(255 * 0.3) = 76 depth steps, z = -50 ->
0.3667 -> 93.  A depth plane of the constant byte B says the surface lies at (256 - B) & 255 steps."""
import ctypes as C
import types
from pathlib import Path

import numpy as np
import pytest

import backproject_model as bm

ROT = np.array([np.eye(3), np.diag([-1.0, 1.0, -1.0])])
VERTS = np.array([[0, 0, 50], [30, 0, 50], [200, 0, 50]], np.float32)
PIX = {(0, 0): (127, 128), (0, 1): (127, 153), (1, 0): (127, 128), (1, 1): (127, 102)}   # (view, vertex) -> (row, col)


def _images(steps0=76, steps1=93):
    """Two views whose depth planes say: the surface lies at steps0 / steps1 depth steps everywhere."""
    images = np.zeros((2, 256, 256, 4), np.float32)
    images[0, :, :, 3] = np.float32(256 - steps0) / np.float32(255.0)
    images[1, :, :, 3] = np.float32(256 - steps1) / np.float32(255.0)
    return images


def _heat(values, peak=2.0):
    """[2,2,256,256]: every plane has its peak ``peak`` at [0, 0] (a pixel no vertex lies at); values[(view, landmark, vertex)] is
    put at that vertex's pixel in that view."""
    heat = np.zeros((2, 2, 256, 256), np.float32)
    heat[:, :, 0, 0] = peak
    for (n, l, v), h in values.items():
        heat[(n, l) + PIX[(n, v)]] = h
    return heat


def _mesh(colors=None):
    from mvlm_amd.utils.mesh_io import Mesh

    return Mesh(VERTS, np.array([[0, 1, 2]], np.int32), colors=colors)


# ---- the model against the hand computation -----------------------------------------------------------------------------------
def test_where_the_vertices_lie_and_who_is_outside():
    for n in (0, 1):
        vis, row, col = bm.visibility(ROT[n], VERTS, _images()[n, :, :, 3], depth_tol=0)
        assert vis.tolist() == [True, True, False]                         # the third vertex is outside the window in both views
        assert (int(row[0]), int(col[0])) == PIX[(n, 0)] and (int(row[1]), int(col[1])) == PIX[(n, 1)]
    X, Y, z, finite = bm.transform(ROT[0], VERTS)
    assert X.tolist() == [32768, 39322, 76459] and Y.tolist() == [32768] * 3 and finite.all()   # 153.6 * 256 = 39321.6 -> 39322
    assert np.trunc(255.0 * z.astype(np.float64)).tolist() == [76, 76, 76]
    assert bm.transform(ROT[0], VERTS, sub_bits=4)[0].tolist() == [32768, 39328, 76464]          # snapped to 1/16 pixel: 2457.6 -> 2458
    # a vertex that is not finite, one behind the far plane and one in front of the near plane are outside
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -1001], [0, 0, 501], [0, 0, 500]], np.float32)
    vis, _, _ = bm.visibility(ROT[0], odd, np.full((256, 256), 1 / 255, np.float32), depth_tol=255)
    assert vis.tolist() == [False, False, False, False, True]


def test_the_mean_over_the_views_that_see_the_vertex():
    heat = _heat({(0, 0, 0): 1.0, (1, 0, 0): 2.0, (0, 1, 1): 0.5})
    got = bm.surface_heat(_mesh(), ROT, _images(), heat, floor=0.25, opacity=0.75)
    assert got["n_visible"].tolist() == [2, 2, 0] and got["n_visible"].dtype == np.int32
    assert got["scores"].dtype == np.float32 and got["scores"].shape == (3, 2)
    assert got["scores"].tolist() == [[0.75, 0.0], [0.0, 0.125], [0.0, 0.0]]     # (0.5 + 1.0) / 2; (0.25 + 0) / 2
    # vertex 0: landmark 0 at 0.75 -> opacity 0.75 * 0.5 / 0.75 = 0.5 of red over grey 200: 200 + 27.5 + 0.5 -> 228, 200 - 100 + 0.5 -> 100
    assert got["colors"].tolist() == [[228, 100, 100, 255], [200, 200, 200, 255], [200, 200, 200, 255]]   # 0.125 <= floor: the base
    assert got["peak_vertex"].tolist() == [0, 1] and got["peak_score"].tolist() == [0.75, 0.125]
    assert got["peak_vertex"].dtype == np.int32 and got["peak_score"].dtype == np.float32


def test_a_vertex_outside_the_window_has_no_view_no_score_and_its_base_colour():
    heat = _heat({})
    heat[:] = 2.0                                                          # every pixel at its plane's peak
    colours = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    got = bm.surface_heat(_mesh(colours), ROT, _images(), heat, floor=0.0, opacity=1.0, colors=[[1, 2, 3], [4, 5, 6]])
    assert got["n_visible"].tolist() == [2, 2, 0] and got["scores"].tolist() == [[1.0, 1.0]] * 2 + [[0.0, 0.0]]
    assert got["colors"].tolist() == [[1, 2, 3, 255], [1, 2, 3, 255], [70, 80, 90, 255]]     # its own colour is the base


def test_one_step_beyond_the_tolerance_hides_the_vertex():
    heat = _heat({(0, 0, 0): 2.0, (1, 0, 0): 1.0})
    for steps0, tol, seen in ((74, 2, True), (73, 2, False), (76, 0, True), (75, 0, False), (0, 76, True), (0, 75, False), (0, 255, True)):
        score, n_vis = bm.scores(VERTS, ROT, _images(steps0=steps0), heat, depth_tol=tol)
        assert n_vis.tolist() == ([2, 2, 0] if seen else [1, 1, 0]), (steps0, tol)
        assert score[0, 0] == (0.75 if seen else 0.5), (steps0, tol)       # seen: (1 + 0.5) / 2; hidden in view 0: 0.5 / 1
    # the background's byte 1 is 255 steps: nothing in the clip range is behind it
    assert bm.scores(VERTS, ROT, _images(steps0=255, steps1=255), heat, depth_tol=0)[1].tolist() == [2, 2, 0]


@pytest.mark.parametrize("bad", (np.nan, -1.0, np.inf, -np.inf))
def test_a_value_that_is_not_finite_or_negative_adds_nothing_and_still_counts_in_the_mean(bad):
    heat = _heat({(0, 0, 0): bad, (1, 0, 0): 2.0})
    score, n_vis = bm.scores(VERTS, ROT, _images(), heat)
    assert n_vis.tolist() == [2, 2, 0] and score[0, 0] == 0.5 and np.isfinite(score).all()   # (0 + 1) / 2
    assert bm.plane_peaks(heat)[0, 0] == 2.0                               # (the peak skips what is not finite)


@pytest.mark.parametrize("fill", (0.0, -3.0, np.nan, np.inf))
def test_a_plane_whose_peak_does_not_count_adds_nothing(fill):
    heat = _heat({(1, 0, 0): 1.0})
    heat[0, 0] = fill                                                      # peak 0, -3, -inf (no finite value) twice
    score, n_vis = bm.scores(VERTS, ROT, _images(), heat)
    assert n_vis.tolist() == [2, 2, 0] and score[0, 0] == 0.25             # (0 + 0.5) / 2
    assert not bm.plane_peaks(heat)[0, 0] > 0


def test_a_tie_between_landmarks_goes_to_the_lowest_selected_index():
    heat = _heat({(0, 0, 0): 1.0, (0, 1, 0): 1.0, (1, 0, 0): 2.0, (1, 1, 0): 2.0})
    score, _ = bm.scores(VERTS, ROT, _images(), heat)
    assert score[0].tolist() == [0.75, 0.75]
    rgb = np.array([[255, 0, 0], [0, 0, 255]], np.uint8)
    base = np.full((3, 3), 200, np.uint8)
    assert bm.paint(score, base, None, rgb, 0.25, 0.75)[0].tolist() == [228, 100, 100, 255]
    assert bm.paint(score, base, [1, 0], rgb, 0.25, 0.75)[0].tolist() == [228, 100, 100, 255]   # the order of naming does not matter
    assert bm.paint(score, base, [1], rgb, 0.25, 0.75)[0].tolist() == [100, 100, 228, 255]
    assert bm.paint(score, base, [], rgb, 0.25, 0.75)[0].tolist() == [200, 200, 200, 255]
    assert bm.paint(score, base, None, None, 0.75, 0.75)[0].tolist() == [200, 200, 200, 255]    # a score equal to the floor draws nothing
    assert bm.paint(score, base, None, None, 0.0, 1.0)[0].tolist() == [241, 50, 50, 255]        # red by default: 200 + 0.75 * 55 + 0.5


def test_a_tie_between_vertices_goes_to_the_lowest_id():
    heat = _heat({(0, 1, 0): 1.0, (0, 1, 1): 1.0, (1, 1, 0): 0.5, (1, 1, 1): 0.5})
    got = bm.surface_heat(_mesh(), ROT, _images(), heat)
    assert got["scores"][:, 1].tolist() == [0.375, 0.375, 0.0]
    assert got["peak_vertex"].tolist() == [-1, 0] and got["peak_score"].tolist() == [0.0, 0.375]   # landmark 0: no score above 0
    flipped = bm.surface_peaks(got["scores"][::-1])
    assert flipped[0].tolist() == [-1, 1]                                  # the same scores in the other order: still the lower id


def test_nothing_visible_anywhere():
    heat = _heat({})
    heat[:] = 2.0
    got = bm.surface_heat(_mesh(), ROT, _images(steps0=10, steps1=10), heat, floor=0.0, opacity=1.0)
    assert got["n_visible"].tolist() == [0, 0, 0] and not got["scores"].any()
    assert got["peak_vertex"].tolist() == [-1, -1] and got["peak_score"].tolist() == [0.0, 0.0]
    assert (got["colors"] == [200, 200, 200, 255]).all()


def test_the_base_is_the_colour_then_the_texel_then_grey():
    from mvlm_amd.utils.mesh_io import Mesh
    from mvlm_amd.utils.synthetic import face_like_mesh

    m = face_like_mesh(grid=5, tex_size=16, vertex_colors=True)           # its colours are its texels, computed by its own code
    inner = (m.uvs < 1).all(axis=1)                                        # (u = 1 wraps to texel 0 here; its own code clamps it)
    np.testing.assert_array_equal(bm.base_colours(m)[inner], m.colors[inner])   # textured: the texel
    assert inner.sum() == 16
    plain = Mesh(m.verts, m.tris, colors=m.colors)
    np.testing.assert_array_equal(bm.base_colours(plain), m.colors)        # colours and no texture: the colours
    assert (bm.base_colours(Mesh(m.verts, m.tris)) == 200).all()
    tex = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3)            # rows top first; v = 0 is the bottom row
    uv = np.array([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9], [1.25, -0.25]], np.float32)   # the last wraps to (0.25, 0.75)
    got = bm.base_colours(Mesh(np.zeros((4, 3), np.float32), np.array([[0, 1, 2]], np.int32), uv, tex))
    assert got.tolist() == [tex[1, 0].tolist(), tex[1, 1].tolist(), tex[0, 0].tolist(), tex[0, 0].tolist()]


# ---- the C ABI, the wrapper and the command line -----------------------------------------------------------------------------------
def test_the_c_abi_is_declared_and_bound():
    from mvlm_amd import _lib

    header = (Path(__file__).resolve().parents[1] / "include" / "mvlm_hip.h").read_text()
    for name, n_args in (("mvlm_surface_heat", 17), ("mvlm_surface_heat_stage_ms", 2), ("mvlm_render_landmark_view_colored", 13),
                         ("mvlm_scratch_bytes", 3), ("mvlm_surface_heat_release", 1)):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name][0] is C.c_int and len(_lib.SIGNATURES[name][1]) == n_args
        assert getattr(_lib.load(), name).restype is C.c_int
    # the landmark view's arguments plus the colours
    assert _lib.SIGNATURES["mvlm_render_landmark_view_colored"][1][:12] == _lib.SIGNATURES["mvlm_render_landmark_view"][1]


def _stub_renderer():
    from mvlm_amd.utils.render3d import HipRenderer3D

    r = object.__new__(HipRenderer3D)
    r.ctx = types.SimpleNamespace(device=0)                                # no context: reaching the library would fail with AttributeError
    return r


def test_the_wrapper_refuses_bad_arguments_before_any_gpu_work():
    from mvlm_amd.utils.mesh_io import Mesh

    r = _stub_renderer()
    images, heat = np.zeros((2, 256, 256, 4), np.float32), np.zeros((2, 3, 256, 256), np.float32)
    for kw in (dict(floor=1.0), dict(floor=-0.1), dict(floor=float("nan")), dict(floor="x"), dict(opacity=0.0), dict(opacity=1.5),
               dict(depth_tol=-1), dict(depth_tol=256), dict(depth_tol=1.5), dict(depth_tol=True), dict(landmarks=[0, 0]),
               dict(landmarks=[0.5]), dict(landmarks=3), dict(landmarks=[True])):
        with pytest.raises(ValueError, match="^surface heat:"):
            r.surface_heat(_mesh(), images, heat, ROT, **kw)
    with pytest.raises(ValueError, match="^surface heat: .*point cloud"):
        r.surface_heat(Mesh(VERTS, np.zeros((0, 3), np.int32)), images, heat, ROT)
    with pytest.raises(ValueError, match="^surface heat: mesh"):
        r.surface_heat("scan.obj", images, heat, ROT)


def test_the_path_helper_and_the_command_line():
    from mvlm_amd.__main__ import build_parser
    from mvlm_amd.utils.viewer import surface_path

    assert surface_path("/data/scans/face_01.obj", "dtu3d") == Path("visualization") / "face_01_dtu3d_surface.png"
    args = build_parser().parse_args(["-p", "x.obj", "--visualize-surface", "--surface-depth-tol", "4", "--surface-mesh",
                                      "--heat-landmarks", "3,17", "--heat-floor", "0.4"])
    assert args.visualize_surface and args.surface_depth_tol == 4 and args.surface_mesh and args.heat_landmarks == [3, 17]
    args = build_parser().parse_args(["-p", "x.obj"])
    assert not args.visualize_surface and args.surface_depth_tol == 2 and not args.surface_mesh
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-p", "x.obj", "--surface-depth-tol", "two"])


# ---- the pipeline's rules that need no GPU ---------------------------------------------------------------------------------------
def test_pipeline_constructor_checks():
    from mvlm_amd import pipeline

    make = lambda **kw: pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, visualize_surface=True, **kw)
    for bad in (-1, 256, 1.5, "2", True):
        with pytest.raises(ValueError, match="surface_depth_tol"):
            make(surface_depth_tol=bad)
    for bad in ([0, 0], [-1], "3", [True]):
        with pytest.raises(ValueError, match="heat_landmarks"):
            make(heat_landmarks=bad)
    for bad in (1.0, -0.5, float("nan"), True):
        with pytest.raises(ValueError, match="heat_floor"):
            make(heat_floor=bad)
    for bad in (32, 1000, 4096):
        with pytest.raises(ValueError, match="visualize_size"):
            make(visualize_size=bad)
    # (a constructor that passes goes on to open the GPU: the options' checks alone, on an object that carries the options)
    from mvlm_amd.pipeline import pictures

    opts = types.SimpleNamespace(visualize_img=False, visualize_rays_img=False, visualize_sheet=False, visualize_heat=False,
                                 visualize_surface=True, sheet_scale=1, heat_floor=0, heat_landmarks=None, visualize_size=256,
                                 surface_depth_tol=np.int64(3))
    pictures.check_options(opts, 8, (4, 1), 256)
    assert opts.surface_depth_tol == 3 and type(opts.surface_depth_tol) is int and opts.heat_landmarks == [4, 1]
    assert opts.heat_floor == 0.0 and type(opts.heat_floor) is float
    pictures.check_options(opts, 96, None, 256)                            # no sheet: 96 views need no layout that fits
    stub = _stub_pipeline(_surface_mesh=None)
    with pytest.raises(ValueError, match="write_surface_mesh: no surface heat"):
        stub.write_surface_mesh("x.obj")


class _Heatmaps:
    def __init__(self, nl=73):
        self.nl, self.calls = nl, 0

    def get_lm_count(self):
        return self.nl

    def heatmaps_device(self, images):
        self.calls += 1
        return _FakeTensor(np.zeros((len(images.a), self.nl, 256, 256), np.float32)) if isinstance(images, _FakeTensor) else None


def _stub_pipeline(**attrs):
    from mvlm_amd.pipeline import DTU3DPipeline
    from mvlm_amd.utils.render3d import HipRenderer3D

    pipe = object.__new__(DTU3DPipeline)
    pipe.__dict__.update(dict(visualize_img=False, visualize_rays_img=False, visualize_sheet=False, visualize_heat=False,
                              visualize_surface=True, heat_landmarks=None, shard_views=False, renderer_3d=object.__new__(HipRenderer3D),
                              predictor_2d=_Heatmaps(), estimator_3d=object()), **attrs)
    return pipe


def test_the_picture_rules(monkeypatch, tmp_path):
    from mvlm_amd import parallel
    from mvlm_amd.pipeline import pictures
    from mvlm_amd.prediction import PrecomputedPredictor
    from mvlm_amd.utils.mesh_io import Mesh

    assert "visualize_surface" in pictures.FLAGS and pictures.wanted(_stub_pipeline()) and pictures.keeps_images(_stub_pipeline())
    _stub_pipeline()._check_visualize()
    pipe = _stub_pipeline(predictor_2d=PrecomputedPredictor(5, fn=lambda images: None))
    with pytest.raises(ValueError, match="visualize_surface needs a predictor with heatmaps_device"):
        pipe._check_visualize()
    with pytest.raises(ValueError, match="heatmaps_device"):               # the first thing a prediction does
        pipe.predict_mesh_device.__wrapped__(pipe, None, np.zeros((8, 6)))
    with pytest.raises(ValueError, match=r"visualize_surface needs a HipRenderer3D in the renderer slot \(it draws the mesh"):
        _stub_pipeline(renderer_3d=object())._check_visualize()
    _stub_pipeline(heat_landmarks=[0, 72])._check_visualize()
    with pytest.raises(ValueError, match=r"heat_landmarks must lie in 0\.\.72"):
        _stub_pipeline(heat_landmarks=[0, 73])._check_visualize()
    pipe = _stub_pipeline(shard_views=True)
    pipe._check_visualize()                                                # not distributed: one process holds every view
    monkeypatch.setattr(parallel, "is_distributed", lambda: True)
    with pytest.raises(ValueError, match="visualize_surface is not supported with shard_views in a distributed run: a rank holds only "
                                         "its slice of the views"):
        pipe._check_visualize()
    # the heat sheet's refusal in the same words
    with pytest.raises(ValueError, match="visualize_heat is not supported with shard_views in a distributed run: a rank holds only "
                                         "its slice of the views"):
        _stub_pipeline(shard_views=True, visualize_surface=False, visualize_heat=True)._check_visualize()
    # a point cloud: refused like the other pictures of a mesh
    cloud = Mesh(VERTS, np.zeros((0, 3), np.int32), path=Path("cloud.ply"))
    with pytest.raises(ValueError, match="cloud.ply is a point cloud: visualize_surface is not supported"):
        _stub_pipeline(landmark_report=False)._check_cloud(cloud)
    _stub_pipeline(landmark_report=False, visualize_surface=False, render_image_stack=False)._check_cloud(cloud)


class _FakeTensor:
    """What the picture code asks of a device tensor, on the host."""

    def __init__(self, a):
        self.a = np.asarray(a)
        self.shape = self.a.shape

    def data_ptr(self):
        return 0

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _fake_renderer(log):
    from mvlm_amd.utils.render3d import HipRenderer3D

    class Fake(HipRenderer3D):
        def __init__(self):
            pass

        def render_heat_sheet(self, images, heat, **kw):
            log.append(("heat_sheet", heat))
            return np.zeros((8, 8, 3), np.uint8)

        def surface_heat(self, mesh, images, heat, rot, **kw):
            log.append(("surface_heat", heat, kw))
            nl = heat.shape[1]
            peak = np.full(nl, -1, np.int32)
            peak[0], peak[1] = 2, 0
            return {"colors": _FakeTensor(np.zeros((mesh.n_verts, 4), np.uint8)), "peak_vertex": _FakeTensor(peak),
                    "peak_score": _FakeTensor(np.linspace(1, 0, nl).astype(np.float32))}

        def render_landmark_view(self, mesh, landmarks, **kw):
            log.append(("landmark_view", landmarks, kw))
            return np.zeros((1, 8, 8, 3), np.uint8)

    return Fake()


@pytest.mark.parametrize("flags", ((True, True), (False, True), (True, False)))
def test_both_heat_pictures_share_one_pass_of_heatmaps(flags, monkeypatch, tmp_path):
    from mvlm_amd.pipeline import pictures
    from mvlm_amd.pipeline.general_pipeline import StageTimer

    monkeypatch.chdir(tmp_path)
    log = []
    heat_on, surface_on = flags
    pipe = _stub_pipeline(visualize_heat=heat_on, visualize_surface=surface_on, renderer_3d=_fake_renderer(log), predictor_2d=_Heatmaps(4),
                          heat_floor=0.25, heat_landmarks=[1, 3], surface_depth_tol=5, sheet_scale=1, visualize_size=256,
                          visualize_name="dtu3d", view_png_encoder="host", timings={}, verbose=False)
    pipe._timer = StageTimer(pipe.timings, pipe._say)
    landmarks = np.array([[0, 0, 53.0], [np.nan, 0, 0], [1, 1, 1], [2, 2, 2]])
    p = pictures.Pass(_mesh(), _FakeTensor(np.zeros((2, 256, 256, 4), np.float32)), None, ROT, None, None, landmarks)
    pictures.draw(pipe, p)
    assert pipe.predictor_2d.calls == 1                                    # one second pass, whatever it feeds
    kinds = [entry[0] for entry in log]
    assert kinds == ["heat_sheet"] * heat_on + ["surface_heat", "landmark_view"] * surface_on
    if heat_on and surface_on:
        assert log[0][1] is log[1][1]                                      # the same heatmaps
    if not surface_on:
        return
    kw = log[-2][2]
    assert kw["landmarks"] == [1, 3] and kw["floor"] == 0.25 and kw["depth_tol"] == 5 and kw["colors"].shape == (4, 3)
    view = log[-1]
    assert view[1].shape == (3, 3) and view[2]["size"] == 256 and view[2]["vertex_colors"].shape == (3, 4)   # the finite landmarks
    assert pipe.last_surface_path == Path("visualization") / "mesh_dtu3d_surface.png" and (tmp_path / pipe.last_surface_path).is_file()
    got = pipe.last_surface_heat
    assert sorted(got) == ["distance", "peak_score", "peak_vertex"] and all(len(got[k]) == 4 for k in got)
    # landmark 0 peaks at vertex 2 (200, 0, 50): |(0, 0, 53) - (200, 0, 50)|; landmark 1 is not finite; 2 and 3 have no peak
    assert got["distance"][0] == np.sqrt(200.0 ** 2 + 3.0 ** 2) and np.isnan(got["distance"][1:]).all()
    out = pipe.write_surface_mesh(tmp_path / "scan_surface.obj")
    assert out.is_file() and len([line for line in out.read_text().splitlines() if line.startswith("v ")]) == 3
