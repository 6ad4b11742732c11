"""-m gpu: the surface heat's kernels (mvlm_surface_heat) against tests/backproject_model.py, exactly; the landmark view drawn with a
colour per vertex against the landmark view of a mesh that carries those colours; the refusals.

The scene: a face of 20 x 20 vertices beside two flat parallel sheets of 20 x 20 vertices 40 units apart, and one triangle that no
view holds - 1203 vertices, so the workgroups of 256 end inside each part and the last one is not full.  The back sheet lies 6 to 7 depth steps (5.9 units each) behind the front one: hidden from
the front at any tolerance below 6, seen from behind.  Three poses: front, 60 degrees of yaw - where the sheets, far out in z, swing
partly out of the window - and 180.  The views are the GPU's own render; the heatmaps are synthetic."""
import numpy as np
import pytest

import backproject_model as bm

pytestmark = pytest.mark.gpu

POSES = np.array([[0, 0, 0], [0, 60, 0], [0, 180, 0]], np.float64)
SELECTED = [0, 2, 4]
LM_RGB = np.array([[255, 0, 0], [0, 200, 0], [0, 90, 255], [255, 200, 0], [255, 0, 255]], np.uint8)


def scene_arrays():
    """(verts float32 [1203,3], tris int32): the face, the front sheet, the back sheet, a triangle outside every view."""
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=20, tex_size=16)
    fv = face.verts.astype(np.float64) * 0.6 + np.array([-75.0, 0.0, 0.0])       # x in -135..-15
    lin = np.linspace(-57.0, 57.0, 20)
    x, y = np.meshgrid(lin + 75.0, lin)                                          # x in 18..132
    front = np.stack([x.ravel(), y.ravel(), np.full(400, 100.0)], axis=1)
    back = front - np.array([0.0, 0.0, 40.0])
    above = np.array([[-10.0, 300.0, 0.0], [10.0, 300.0, 0.0], [0.0, 320.0, 0.0]])   # a triangle no view of these poses holds
    verts = np.concatenate([fv, front, back, above]).astype(np.float32)
    tris = np.concatenate([face.tris, face.tris + 400, face.tris + 800, [[1200, 1201, 1202]]]).astype(np.int32)
    return verts, tris


def scene_mesh(kind: str):
    """The scene as a plain mesh, a mesh with a colour per vertex, or a textured one."""
    from mvlm_amd.utils.mesh_io import Mesh

    verts, tris = scene_arrays()
    rs = np.random.RandomState(3)
    if kind == "colors":
        return Mesh(verts, tris, colors=rs.randint(0, 256, (len(verts), 3)).astype(np.uint8))
    if kind == "texture":
        uvs = rs.uniform(-0.5, 1.5, (len(verts), 2)).astype(np.float32)          # (some wrap round)
        return Mesh(verts, tris, uvs, rs.randint(0, 256, (24, 40, 3)).astype(np.uint8))
    return Mesh(verts, tris)


def synthetic_heat(seed: int = 7) -> np.ndarray:
    """[3,5,256,256]: a Gaussian bump per plane with its own height, plane (1, 2) all zero, plane (2, 3) all negative, and NaN,
    +inf, -inf and negative values planted on 3 % of the pixels of every plane."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    heat = np.empty((3, 5, 256, 256), np.float32)
    for n in range(3):
        for l in range(5):
            cy, cx, s = rs.uniform(60, 196), rs.uniform(60, 196), rs.uniform(25, 60)
            heat[n, l] = rs.uniform(0.5, 9.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    heat[1, 2] = 0.0
    heat[2, 3] = -heat[2, 3] - 1.0
    planted = rs.uniform(size=heat.shape) < 0.03
    heat[planted] = rs.choice(np.array([np.nan, np.inf, -np.inf, -0.5], np.float32), size=int(planted.sum()))
    return heat


@pytest.fixture(scope="module")
def renderers():
    from mvlm_amd.utils.render3d import HipRenderer3D

    return {bits: HipRenderer3D(n_views=3, verbose=False, subpixel_bits=bits) for bits in (8, 4)}


@pytest.fixture(scope="module")
def heat():
    import torch

    host = synthetic_heat()
    return host, torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def views(renderers):
    """Per sub-pixel setting: the plain scene, its views on the device and on the host, the rotations."""
    from mvlm_amd.utils.render3d import view_rotations

    out = {}
    for bits, r in renderers.items():
        mesh = scene_mesh("plain")
        images = r.render_device(mesh, POSES).clone()
        r.check()
        out[bits] = (mesh, images, images.cpu().numpy(), np.asarray(view_rotations(POSES), np.float64).reshape(3, 3, 3))
    return out


def _compare(got: dict, want: dict, what):
    for key in ("n_visible", "scores", "colors", "peak_vertex", "peak_score"):
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, (what, key)
        differing = int((g != want[key]).sum()) if key != "scores" else int((g.view(np.uint32) != want[key].view(np.uint32)).sum())
        print(f"{what}: {key}: {differing} of {g.size} differ")
        np.testing.assert_array_equal(g, want[key], err_msg=f"{what}: {key}")


def test_the_scene_can_tell_right_from_wrong(views, heat):
    """Asserted on the model's output, so that the comparisons below cannot pass vacuously."""
    mesh, _, images, rot = views[8]
    front, _, _ = bm.visibility(rot[0], mesh.verts, images[0, :, :, 3], depth_tol=2)
    assert front.sum() >= 300 and (~front).sum() >= 300                  # a quarter of the vertices each way; the back sheet alone is a third
    assert not front[800:1200].any() and front[400:800].all()                # the back sheet is hidden from the front, the front one seen
    behind, _, _ = bm.visibility(rot[2], mesh.verts, images[2, :, :, 3], depth_tol=2)
    assert behind[800:1200].all() and not behind[400:800].any()              # and the other way round from behind
    for n, outside in ((0, False), (1, True), (2, False)):               # only the yawed view loses vertices to the window
        X, Y, z, _ = bm.transform(rot[n], mesh.verts)
        assert bool(((X < 0) | (X >= 65536))[:1200].any()) == outside and ((Y >= 65536) == (np.arange(1203) >= 1200)).all(), n
    wide, _, _ = bm.visibility(rot[0], mesh.verts, images[0, :, :, 3], depth_tol=255)
    assert wide[:1200].all() and not wide[1200:].any()
    want = bm.surface_heat(mesh, rot, images, heat[0], selected=SELECTED, colors=LM_RGB)
    assert (want["peak_vertex"] >= 0).sum() >= 3 and set(want["n_visible"].tolist()) == {0, 1, 2, 3}
    assert not want["n_visible"][1200:].any() and not want["scores"][1200:].any()
    assert (want["colors"][:, :3] != 200).any(axis=1).sum() >= 100 and (want["colors"][:, :3] == 200).all(axis=1).sum() >= 100


@pytest.mark.parametrize("depth_tol", (0, 2, 255))
@pytest.mark.parametrize("bits", (8, 4))
def test_the_kernels_equal_the_model(renderers, views, heat, bits, depth_tol):
    mesh, images_dev, images, rot = views[bits]
    r = renderers[bits]
    got = r.surface_heat(mesh, images_dev, heat[1], rot, landmarks=SELECTED, colors=LM_RGB, depth_tol=depth_tol, return_scores=True)
    r.check()
    want = bm.surface_heat(mesh, rot, images, heat[0], selected=SELECTED, colors=LM_RGB, depth_tol=depth_tol, sub_bits=bits)
    _compare(got, want, f"bits {bits}, depth_tol {depth_tol}")
    if bits == 8 and depth_tol == 2:
        # the rotations where the rasteriser keeps them, numpy inputs, no score table asked for, no selection and the default red
        r.render_device(mesh, POSES)
        again = r.surface_heat(mesh, images, heat[0], r.rotations_device(), landmarks=SELECTED, colors=LM_RGB)
        assert "scores" not in again
        for key in ("n_visible", "colors", "peak_vertex", "peak_score"):
            np.testing.assert_array_equal(again[key].cpu().numpy(), want[key], err_msg=key)
        everyone = r.surface_heat(mesh, images_dev, heat[1], rot, floor=0.1, opacity=1.0, return_scores=True)
        _compare(everyone, bm.surface_heat(mesh, rot, images, heat[0], floor=0.1, opacity=1.0), "all landmarks, red")


@pytest.mark.parametrize("kind", ("colors", "texture", "plain"))
def test_each_kind_of_mesh_takes_its_base(renderers, heat, kind):
    from mvlm_amd.utils.render3d import view_rotations

    r = renderers[8]
    mesh = scene_mesh(kind)
    images_dev = r.render_device(mesh, POSES).clone()
    rot = np.asarray(view_rotations(POSES), np.float64).reshape(3, 3, 3)
    got = r.surface_heat(mesh, images_dev, heat[1], rot, landmarks=SELECTED, colors=LM_RGB, floor=0.5, return_scores=True)
    r.check()
    want = bm.surface_heat(mesh, rot, images_dev.cpu().numpy(), heat[0], selected=SELECTED, colors=LM_RGB, floor=0.5)
    _compare(got, want, kind)
    base = bm.base_colours(mesh)
    untouched = (want["scores"][:, SELECTED] <= 0.5).all(axis=1)
    assert untouched.sum() >= 100 and (~untouched).sum() >= 100
    np.testing.assert_array_equal(got["colors"].cpu().numpy()[untouched, :3], base[untouched])
    assert (kind == "plain") == bool((base == 200).all())


@pytest.mark.parametrize("size", (64, 256))
def test_the_coloured_landmark_view_is_the_view_of_a_mesh_with_those_colours(renderers, views, heat, size):
    from mvlm_amd.utils.mesh_io import Mesh

    r = renderers[8]
    landmarks = np.array([[-75.0, 0.0, 40.0], [75.0, 10.0, 101.0], [0.0, -40.0, 0.0]])
    poses = [[0, 0, 0], [10, 60, 0]]
    for kind in ("texture", "plain"):                                    # a texture of the mesh's own is not drawn
        mesh = scene_mesh(kind)
        mesh_views = r.render_device(mesh, POSES).clone()
        colours = r.surface_heat(mesh, mesh_views, heat[1], views[8][3], colors=LM_RGB, floor=0.1)["colors"]
        host = colours.cpu().numpy()
        assert len(np.unique(host[:, :3], axis=0)) > 50
        want, want_px = r.render_landmark_view(Mesh(mesh.verts, mesh.tris, colors=host[:, :3].copy()), landmarks, poses=poses, size=size,
                                               return_pixels=True)
        got, got_px = r.render_landmark_view(mesh, landmarks, poses=poses, size=size, return_pixels=True, vertex_colors=colours)
        print(f"size {size}, {kind}: {int((got != want).sum())} differing bytes of {want.size}")
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_px, want_px)
        np.testing.assert_array_equal(r.render_landmark_view(mesh, landmarks, poses=poses, size=size, vertex_colors=host[:, :3]), want)   # numpy [V,3]
        today = r.render_landmark_view(mesh, landmarks, poses=poses, size=size)
        np.testing.assert_array_equal(r.render_landmark_view(mesh, landmarks, poses=poses, size=size, vertex_colors=None), today)
        assert (today != want).any()
    with pytest.raises(ValueError, match="vertex_colors"):
        r.render_landmark_view(mesh, landmarks, size=size, vertex_colors=np.zeros((5, 4), np.uint8))


def test_refusals_leave_the_context_rendering(renderers, views, heat):
    import torch

    from mvlm_amd.utils.mesh_io import Mesh

    r = renderers[8]
    mesh, images_dev, images, rot = views[8]
    before = r.surface_heat(mesh, images_dev, heat[1], rot, return_scores=True)
    cloud = Mesh(mesh.verts, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="^surface heat: .*point cloud"):
        r.surface_heat(cloud, images_dev, heat[1], rot)
    flat = torch.zeros(heat[1].numel() + 1, dtype=torch.float32, device="cuda")
    misaligned = flat[1:].view(heat[1].shape)
    assert misaligned.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="^surface heat: .*16-byte aligned"):
        r.surface_heat(mesh, images_dev, misaligned, rot)
    for kw in (dict(floor=1.0), dict(floor=-0.01), dict(opacity=0.0), dict(opacity=1.01), dict(depth_tol=-1), dict(depth_tol=256)):
        with pytest.raises(ValueError, match="^surface heat:"):
            r.surface_heat(mesh, images_dev, heat[1], rot, **kw)
    # the library's own checks, behind the wrapper's
    import ctypes as C

    from mvlm_amd import _lib
    from mvlm_amd.utils.render3d import upload_mesh

    ctx = r.ctx
    rot_dev = torch.from_numpy(rot.reshape(3, 9).copy()).cuda()
    outs = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (1203, 5, 5)]
    def call(mesh_handle, heat_ptr, floor=0.25, opacity=0.75, tol=2, rot_ptr=None):
        return ctx.lib.mvlm_surface_heat(ctx.handle, mesh_handle, C.c_void_p(rot_dev.data_ptr() if rot_ptr is None else rot_ptr),
                                         C.c_void_p(images_dev.data_ptr()), C.c_void_p(heat_ptr), 3, 5, None, None, C.c_double(floor),
                                         C.c_double(opacity), tol, C.c_void_p(outs[0].data_ptr()), None, None, C.c_void_p(outs[1].data_ptr()),
                                         C.c_void_p(outs[2].data_ptr()))
    handle, cloud_handle = upload_mesh(ctx, mesh), upload_mesh(ctx, cloud)
    for args, word in (((cloud_handle, heat[1].data_ptr()), "point cloud"), ((handle, misaligned.data_ptr()), "16-byte aligned"),
                       ((handle, heat[1].data_ptr(), 1.0), "floor"), ((handle, heat[1].data_ptr(), 0.25, 0.0), "opacity"),
                       ((handle, heat[1].data_ptr(), 0.25, 0.75, 256), "depth_tol"), ((handle, 0), "null pointer"),
                       ((handle, heat[1].data_ptr(), 0.25, 0.75, 2, rot_dev.data_ptr() + 4), "8-byte aligned")):
        assert call(*args) == 1
        message = ctx.lib.mvlm_last_error(ctx.handle).decode()
        assert message.startswith("surface heat:") and word in message, message
    assert not any(int(o.any()) for o in outs)                           # nothing was launched
    assert call(handle, heat[1].data_ptr()) == 0
    after = r.surface_heat(mesh, images_dev, heat[1], rot, return_scores=True)
    r.check()
    for key in before:
        np.testing.assert_array_equal(after[key].cpu().numpy(), before[key].cpu().numpy(), err_msg=key)
    np.testing.assert_array_equal(outs[0].cpu().numpy().view(np.uint8).reshape(1203, 4), before["colors"].cpu().numpy())
    np.testing.assert_array_equal(r.render_device(mesh, POSES).cpu().numpy(), images)


def test_the_stage_times_need_profiling(renderers, views, heat):
    r = renderers[8]
    mesh, images_dev, _, rot = views[8]
    r.ctx.check(r.ctx.lib.mvlm_render_set_profiling(r.ctx.handle, 1))
    try:
        r.surface_heat(mesh, images_dev, heat[1], rot)
        ms = r.surface_heat_stage_ms()
        assert ms.shape == (3,) and (ms > 0).all() and ms.sum() < 1000
    finally:
        r.ctx.check(r.ctx.lib.mvlm_render_set_profiling(r.ctx.handle, 0))
    r.surface_heat(mesh, images_dev, heat[1], rot)
    with pytest.raises(Exception, match="no surface heat was computed with render profiling on"):
        r.surface_heat_stage_ms()
    assert 0 < r.scratch_bytes("backproject") < r.scratch_bytes()
    r.release_surface_heat()
    assert r.scratch_bytes("backproject") == 0
