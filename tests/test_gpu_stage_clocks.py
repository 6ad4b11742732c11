"""-m gpu: the eight per-feature stage clocks (csrc/common.h: StageClock) through their readers mvlm_*_stage_ms - each refuses with
its own message unless the feature's last call ran under render profiling, and gives its stage times when it did; the landmark and
the ray view share one clock and refuse after each other's call; a refused PNG or heat sheet call forgets the times before it; a
context that has profiled a surface heat is destroyed and the process goes on.  The clocks are host code: the inputs are as small
as the features' own tests use, every kernel merely has to run."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = {
    "points": "points_stage_ms: no point cloud was rendered with render profiling on",
    "normals": "normals_stage_ms: no normals were estimated with render profiling on",
    "cloud_mesh": "cloud_mesh_stage_ms: no cloud was triangulated with render profiling on",
    "landmark_view": "landmark_view_stage_ms: no landmark view was drawn with render profiling on",
    "ray_view": "ray_view_stage_ms: no ray view was drawn with render profiling on",
    "png": "png_stage_ms: no picture was encoded with render profiling on",
    "heat_sheet": "heat_sheet_stage_ms: no heat sheet was drawn with render profiling on",
    "surface_heat": "surface_heat_stage_ms: no surface heat was computed with render profiling on",
}
STAGES = {"points": 2, "normals": 3, "cloud_mesh": 3, "landmark_view": 7, "ray_view": 8, "png": 4, "heat_sheet": 3, "surface_heat": 3}
FRONT = np.zeros((1, 6), np.float32)
N, NL = 8, 5


@pytest.fixture(scope="module")
def r3():
    from mvlm_amd.utils.render3d import HipRenderer3D

    return HipRenderer3D(n_views=8, verbose=False)


def _blob(cy, cx, sigma, amplitude):
    y, x = np.mgrid[0:256, 0:256].astype(np.float64)
    return (amplitude * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2.0 * sigma * sigma))).astype(np.float32)


def _heat(seed):
    """[8,5,256,256]: a Gaussian bump of its own place, width and height on every plane"""
    rs = np.random.RandomState(seed)
    return np.stack([np.stack([_blob(rs.uniform(60, 196), rs.uniform(60, 196), rs.uniform(8, 40), rs.uniform(0.5, 9.0)) for _ in range(NL)])
                     for _ in range(N)])


def _small_mesh():
    """A face of 20 x 20 vertices: the surface heat's scene takes its face from the same call."""
    from mvlm_amd.utils.mesh_io import Mesh
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=20, tex_size=16)
    return Mesh(face.verts, face.tris)


class Feature:
    """One feature: ``run()`` makes one call of it, ``read()`` returns its reader's times (or raises the library's error)."""

    def __init__(self, name, run, read):
        self.name, self.run, self.read = name, run, read


@pytest.fixture(scope="module")
def features(r3):
    """The eight features on one renderer, each with inputs of its own that stay alive and unchanged for the module."""
    import torch

    from mvlm_amd.utils.mesh_io import Mesh
    from mvlm_amd.utils.render3d import upload_mesh, view_rotations
    from mvlm_amd.utils.synthetic import face_like_mesh

    ctx, lib = r3.ctx, r3.ctx.lib
    dev = torch.device("cuda", ctx.device)

    def through_lib(entry, n):
        def read():
            ms = np.zeros(n, np.float32)
            ctx.check(getattr(lib, entry)(ctx.handle, ms.ctypes.data_as(C.POINTER(C.c_float))))
            return ms
        return read

    # a cloud of 32 x 32 = 1024 points, its device copy and - for the triangulation - the device's neighbour table
    cloud = Mesh(np.ascontiguousarray(face_like_mesh(grid=32, tex_size=16, seed=1).verts, np.float32), np.zeros((0, 3), np.int32))
    cloud_handle = upload_mesh(ctx, cloud)
    table = torch.empty((cloud.n_verts, 16), dtype=torch.int32, device=dev)
    ctx.bind_current_stream(torch, dev)
    ctx.check(lib.mvlm_mesh_estimate_normals(ctx.handle, cloud_handle, C.c_void_p(table.data_ptr())))
    cap = 4 * cloud.n_verts
    tris = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def render_cloud():
        r3.render_device(cloud, FRONT)
        r3.check()

    def triangulate():
        ctx.bind_current_stream(torch, dev)
        ctx.check(lib.mvlm_mesh_triangulate_points(ctx.handle, cloud_handle, C.c_void_p(table.data_ptr()), C.c_void_p(tris.data_ptr()),
                                                   C.c_longlong(cap), C.c_void_p(count.data_ptr())))
        assert 1000 < int(count.item()) <= cap

    # a small mesh, one landmark and one ray at size 256
    mesh = _small_mesh()
    landmark = np.asarray(mesh.verts, np.float64)[[210]]
    start, end = landmark + [0.0, 0.0, 200.0], landmark - [0.0, 0.0, 50.0]

    # one 256 x 256 RGBA picture
    picture = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (256, 256, 4)).astype(np.uint8)).to(dev)

    # the heat sheet's scene: random views, a bump per plane; the surface heat's: the GPU's own render of the mesh, a bump per plane
    rs = np.random.RandomState(31)
    sheet_images = torch.from_numpy(rs.randint(0, 256, (N, 256, 256, 4)).astype(np.float32) / np.float32(255.0)).to(dev)
    sheet_heat = torch.from_numpy(_heat(32)).to(dev)
    poses = r3.generate_3d_transformations()
    assert poses.shape == (N, 6)
    surface_images = r3.render_device(mesh, poses).clone()
    r3.check()
    surface_heat = torch.from_numpy(_heat(7)).to(dev)
    rot = np.asarray(view_rotations(poses), np.float64).reshape(N, 3, 3)

    fs = [Feature("points", render_cloud, through_lib("mvlm_points_stage_ms", 2)),
          Feature("normals", lambda: r3.estimate_point_normals(cloud), r3.normals_stage_ms),
          Feature("cloud_mesh", triangulate, r3.cloud_mesh_stage_ms),
          Feature("landmark_view", lambda: r3.render_landmark_view(mesh, landmark, size=256), through_lib("mvlm_landmark_view_stage_ms", 7)),
          Feature("ray_view", lambda: r3.render_ray_view(mesh, landmark, start, end, size=256), through_lib("mvlm_ray_view_stage_ms", 8)),
          Feature("png", lambda: r3.encode_png(picture), r3.png_stage_ms),
          Feature("heat_sheet", lambda: r3.render_heat_sheet(sheet_images, sheet_heat), r3.heat_sheet_stage_ms),
          Feature("surface_heat", lambda: r3.surface_heat(mesh, surface_images, surface_heat, rot), r3.surface_heat_stage_ms)]
    out = {f.name: f for f in fs}
    out["scene"] = dict(mesh=mesh, picture=picture, sheet=(sheet_images, sheet_heat), surface=(surface_images, surface_heat, rot))
    return out


class profiling:
    """mvlm_render_set_profiling on for the block, off behind it whatever happens"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.check(self.ctx.lib.mvlm_render_set_profiling(self.ctx.handle, 1))

    def __exit__(self, *exc):
        self.ctx.check(self.ctx.lib.mvlm_render_set_profiling(self.ctx.handle, 0))
        return False


def _refuses(feature):
    from mvlm_amd import _lib

    with pytest.raises(_lib.MvlmHipError) as e:
        feature.read()
    assert str(e.value) == NONE[feature.name]


def _times(feature):
    ms = feature.read()
    print(f"{feature.name} [ms]:", ms.tolist())
    assert ms.shape == (STAGES[feature.name],) and ms.dtype == np.float32
    assert np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0
    return ms


@pytest.mark.parametrize("name", list(STAGES))
def test_a_reader_refuses_without_profiling_and_gives_its_times_with_it(r3, features, name):
    f = features[name]
    f.run()
    _refuses(f)
    with profiling(r3.ctx):
        f.run()
        _times(f)
    f.run()
    _refuses(f)


def test_the_two_views_share_one_clock(r3, features):
    landmark_view, ray_view = features["landmark_view"], features["ray_view"]
    with profiling(r3.ctx):
        ray_view.run()
        _refuses(landmark_view)
        _times(ray_view)
        landmark_view.run()
        _times(landmark_view)
        _refuses(ray_view)


def test_a_refused_call_forgets_the_times_before_it(r3, features):
    import torch

    ctx, lib = r3.ctx, r3.ctx.lib
    scene = features["scene"]
    images, heat = scene["sheet"]
    _, _, width, height = r3.view_sheet_layout(N)
    out = torch.empty((height, width, 4), dtype=torch.uint8, device=images.device)
    with profiling(ctx):
        features["png"].run()
        _times(features["png"])
        with pytest.raises(ValueError, match="^png: filter_mode must be -1..4 \\(7 given\\)"):
            r3.encode_png(scene["picture"], filter_mode=7)
        _refuses(features["png"])

        features["heat_sheet"].run()
        _times(features["heat_sheet"])
        ctx.bind_current_stream(torch, images.device)
        rc = lib.mvlm_render_heat_sheet(ctx.handle, C.c_void_p(images.data_ptr()), C.c_void_p(heat.data_ptr()), N, NL, None, None,
                                        2, 0, 1, 2, C.c_double(0.25), C.c_double(0.75), C.c_void_p(out.data_ptr()))
        assert rc != 0 and lib.mvlm_last_error(ctx.handle).decode().startswith("heat sheet: background must be 0 (rgb) or 1 (depth)")
        _refuses(features["heat_sheet"])


def test_a_context_that_profiled_a_surface_heat_is_destroyed(r3, features):
    """The teardown frees the surface heat's events with every other clock's; the first context works on."""
    from mvlm_amd import _lib
    from mvlm_amd.utils.render3d import HipRenderer3D

    images, heat, rot = features["scene"]["surface"]
    other = HipRenderer3D(n_views=8, verbose=False)
    other.ctx = _lib.Context(r3.ctx.device)
    assert other.ctx.handle.value != r3.ctx.handle.value
    mesh = _small_mesh()                                   # (a Mesh of its own: its device copy belongs to the second context)
    try:
        with profiling(other.ctx):
            other.surface_heat(mesh, images, heat, rot)
            ms = other.surface_heat_stage_ms()
        assert ms.shape == (3,) and np.isfinite(ms).all() and (ms >= 0).all() and ms.sum() > 0
        other.check()
        mesh._device.clear()                               # the device copy goes back to its context before that goes
    finally:
        other.ctx.close()
    with profiling(r3.ctx):
        features["surface_heat"].run()
        _times(features["surface_heat"])
    r3.check()
