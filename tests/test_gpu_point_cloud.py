"""-m gpu: point clouds - scans with points and no faces - on the device: the splat renderer (raster_points.hip) against the
numpy statement of its contract (tests/points_model.py) bit for bit, the nearest-point snap (surface_points.hip) against
numpy brute force, the refusals, and a cloud through every layer down to the command line."""
import ctypes as C

import numpy as np
import pytest

import points_model as pm

pytestmark = pytest.mark.gpu

NO_TRIS = np.zeros((0, 3), np.int32)
FRONT = np.zeros((1, 6), np.float32)
K = 300.0 / 256.0  # model units per pixel


def _cloud(verts, colors=None, radius=None):
    from mvlm_amd.utils import Mesh

    return Mesh(np.ascontiguousarray(verts, np.float32).reshape(-1, 3), NO_TRIS, colors=colors, point_radius=radius)


def _hip(mesh, poses, bits=8, ctx=None, **kw):
    from mvlm_amd.utils import HipRenderer3D

    r = HipRenderer3D(n_views=len(poses), verbose=False, subpixel_bits=bits, **kw)
    if ctx is not None:
        r.ctx = ctx
    out = r.render_device(mesh, np.asarray(poses)).cpu().numpy()
    r.check()
    return out


def _poses(seed, n):
    rs = np.random.RandomState(seed)
    p = np.zeros((n, 6), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = rs.randint(-40, 40, n), rs.randint(-80, 80, n), rs.randint(-20, 20, n)
    return p


def _colours(n, seed=0):
    return np.random.RandomState(seed).randint(0, 255, size=(n, 3)).astype(np.uint8)  # (never white: a splat shows)


def _equal(mesh, poses, bits=8):
    want = pm.render(mesh.verts, poses, mesh.point_radius, mesh.colors, bits)
    np.testing.assert_array_equal(_hip(mesh, poses, bits), want)
    return want


# ---- 1. render_device equals the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [4, 8])
def test_one_point_at_every_radius_and_position(bits):
    """0.75 px: the floor; 1 px on a pixel centre: the rim runs through four pixel centres and <= decides; 8 px: the largest box."""
    centre = [100.5 * K - 150.0, 60.5 * K - 150.0, 5.0]     # the centre of pixel (100, 60)
    corner = [100.0 * K - 150.0, 60.0 * K - 150.0, 5.0]     # where four pixels meet
    generic = [17.31, -42.77, 12.3]
    X, Y, _ = pm.transform(np.array([centre, corner], np.float32), pm.rotations(FRONT)[0], bits)
    assert (X[0], Y[0]) == (256 * 100 + 128, 256 * 60 + 128) and (X[1], Y[1]) == (256 * 100, 256 * 60)
    covered = {}
    for r_px in (0.75, 1.0, 2.5, 8.0):
        for name, p in (("centre", centre), ("corner", corner), ("generic", generic)):
            mesh = _cloud([p], _colours(1), radius=pm.px_to_model(r_px))
            want = _equal(mesh, FRONT, bits)
            covered[r_px, name] = int((want[0, :, :, 0] != 1.0).sum())
    assert covered[0.75, "centre"] == 1 and covered[0.75, "corner"] == 4
    assert covered[1.0, "centre"] == 5 and covered[1.0, "corner"] == 4      # the four centres at exactly 256 steps are in
    assert covered[8.0, "centre"] == 197                                     # lattice points with dx^2 + dy^2 <= 64
    assert all(n >= 1 for n in covered.values())


@pytest.mark.parametrize("bits", [4, 8])
def test_equal_depths_go_to_the_higher_id(bits):
    """Neighbours of one depth split the screen along their bisector; put where four pixels meet, one pixel apart, the
    bisector runs through a column (a row) of pixel centres, where both splats have the same depth bit for bit."""
    px = np.array([[100.0, 60.0], [101.0, 60.0], [100.0, 61.0]])
    pts = np.column_stack([px * K - 150.0, np.full(3, 7.0)]).astype(np.float32)
    col = np.array([[200, 0, 0], [0, 200, 0], [0, 0, 200]], np.uint8)
    seen = []
    for n in (2, 3):
        for order in (slice(None), slice(None, None, -1)):
            mesh = _cloud(pts[:n][order], col[:n][order], radius=pm.px_to_model(3.0))
            seen.append(_equal(mesh, FRONT, bits))
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[2], seen[3])   # the file order decides the ties
    # exactly coincident points: the whole disc is a tie, the later point takes all of it
    mesh = _cloud(np.repeat(pts[:1], 3, axis=0), col, radius=pm.px_to_model(3.0))
    got = _equal(mesh, FRONT, bits)
    hit = got[0, :, :, 3] != got[0, 0, 0, 3]
    assert hit.any() and (np.rint(got[0][hit][:, :3] * 255) == col[2]).all()


@pytest.mark.parametrize("bits", [4, 8])
def test_window_edges_clip_planes_and_a_nan_point(bits):
    e = 150.0
    pts = [[-e, 0, 0], [e, 0, 0], [0, -e, 0], [0, e, 0], [-e, -e, 0], [e, -e, 0], [-e, e, 0], [e, e, 0],       # straddling
           [-e - 1.0, 40, 0], [e + 1.5, 40, 0], [40, -e - 2.0, 0], [40, e + 0.5, 0],                              # partly in
           [-e - 20, 0, 0], [e + 20, 0, 0], [0, -e - 20, 0], [0, e + 20, 0], [1e6, 0, 0], [0, -3e38, 0],         # wholly outside
           [-100, 100, 499.99], [-80, 100, 500.01], [-60, 100, 501.5], [-40, 100, 504.0],                        # near plane
           [-100, 70, -999.9], [-80, 70, -1000.01], [-60, 70, -998.0], [-40, 70, -1004.0],                      # far plane
           [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [30, 30, 3]]
    mesh = _cloud(pts, _colours(len(pts), 2), radius=pm.px_to_model(2.5))
    want = _equal(mesh, FRONT, bits)
    shown = {tuple(c) for c in np.rint(want[0][want[0, :, :, 0] != 1.0][:, :3] * 255).astype(int)}
    col = [tuple(int(v) for v in c) for c in mesh.colors]
    assert all(col[k] in shown for k in list(range(12)) + [18, 22, 24, 29])
    assert not any(col[k] in shown for k in [12, 13, 14, 15, 16, 17, 21, 25, 26, 27, 28])
    assert col[20] in shown and col[19] in shown    # behind the near plane at the centre, the rising rim comes back inside
    _equal(mesh, _poses(4, 3), bits)


@pytest.mark.parametrize("bits", [4, 8])
def test_a_face_like_cloud_with_and_without_colours(bits):
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=40, tex_size=64, seed=1, vertex_colors=True)
    poses = _poses(7, 8)
    with_c = _equal(_cloud(face.verts, face.colors), poses, bits)
    without = _equal(_cloud(face.verts), poses, bits)
    np.testing.assert_array_equal(with_c[..., 3], without[..., 3])
    assert (with_c[..., :3] != without[..., :3]).any(-1).mean() > 0.1
    assert (without[..., :3] == 1.0).all()


@pytest.mark.parametrize("n_views", [1, 3])
def test_one_point_past_a_workgroup(n_views):
    rs = np.random.RandomState(11)
    verts = rs.uniform(-120, 120, size=(257, 3)).astype(np.float32)
    verts[256] = [3.0, -4.0, 125.0]                          # the 257th point: in front of all others in the front view
    mesh = _cloud(verts, _colours(257, 3))
    poses = _poses(5, n_views)
    poses[0, :3] = 0.0
    want = _equal(mesh, poses)
    last = tuple(int(v) for v in mesh.colors[256])
    assert any(tuple(c) == last for c in np.rint(want[0][want[0, :, :, 0] != 1.0][:, :3] * 255).astype(int))


# ---- 2. clouds and triangle meshes take turns on one context ---------------------------------------------------------------
def test_clouds_and_meshes_alternate_on_one_context():
    from mvlm_amd import _lib
    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=40, tex_size=64, seed=1, vertex_colors=True)
    poses = _poses(9, 3)
    make = [lambda: _cloud(face.verts, face.colors), lambda: Mesh(face.verts, face.tris, face.uvs, face.texture),
            lambda: _cloud(face.verts[::3] * 0.7), lambda: Mesh(face.verts * 0.8, face.tris, colors=face.colors)]
    shared = _lib.Context(0)
    try:
        for k, mk in enumerate(make):
            got = _hip(mk(), poses, ctx=shared)
            fresh = _lib.Context(0)
            try:
                np.testing.assert_array_equal(got, _hip(mk(), poses, ctx=fresh), err_msg=f"render {k}")
            finally:
                fresh.close()
            if k in (0, 2):
                m = mk()
                np.testing.assert_array_equal(got, pm.render(m.verts, poses, None, m.colors))
    finally:
        shared.close()


# ---- 3. the snap -----------------------------------------------------------------------------------------------------------
def _snap(mesh, queries):
    from mvlm_amd.utils import HipEstimator3D

    return HipEstimator3D(verbose=False).project_landmarks_to_surface(mesh, queries)


@pytest.mark.parametrize("n_points,n_queries", [(1, 3), (1025, 9), (3000, 478)])
def test_snap_is_numpy_brute_force(n_points, n_queries):
    rs = np.random.RandomState(n_points)
    verts = rs.uniform(-100, 100, size=(n_points, 3)).astype(np.float32)
    queries = rs.uniform(-120, 120, size=(n_queries, 3))
    queries[0] = verts[-1].astype(np.float64)                # on a point: distance 0
    got = _snap(_cloud(verts), queries)
    np.testing.assert_array_equal(got, pm.nearest(verts, queries))
    rows = {r.tobytes() for r in verts.astype(np.float64)}
    assert all(g.tobytes() in rows for g in got)             # every answer is a row of the cloud


def test_snap_ties_nan_points_and_nan_queries():
    rs = np.random.RandomState(2)
    verts = rs.uniform(-50, 50, size=(1500, 3)).astype(np.float32)
    verts[1200] = verts[7]                                   # duplicates: the lowest id wins (same coordinates either way) ...
    verts[300] = [10.0, 0.0, 0.0]
    verts[1100] = [-10.0, 0.0, 0.0]                          # ... and two points at one distance from (0, 0, 0): id 300 wins
    verts[5] = [np.nan, 0.0, 0.0]
    verts[6] = [0.0, np.inf, 0.0]
    keep = np.linalg.norm(verts, axis=1) >= 10.0
    keep[[5, 6]] = True
    verts[~keep] *= 30.0 / np.maximum(np.linalg.norm(verts[~keep], axis=1, keepdims=True), 1e-3)   # nothing nearer the origin
    queries = rs.uniform(-60, 60, size=(20, 3))
    queries[0] = 0.0
    queries[1] = verts[7].astype(np.float64) + 1e-3
    queries[2] = [np.nan, 1.0, 2.0]
    queries[3] = [1.0, np.inf, 2.0]
    got = _snap(_cloud(verts), queries)
    want = pm.nearest(verts, queries)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0], [10.0, 0.0, 0.0])
    np.testing.assert_array_equal(got[2], queries[2])
    np.testing.assert_array_equal(got[3], queries[3])
    assert np.isfinite(np.delete(got, [2, 3], axis=0)).all()


# ---- 4. argument errors ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    import torch

    from mvlm_amd import _lib
    from mvlm_amd.utils import HipEstimator3D, HipRenderer3D, Mesh
    from mvlm_amd.utils.render3d import upload_mesh
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=12, tex_size=16, seed=1, vertex_colors=True)
    cloud = _cloud(face.verts, face.colors)
    want = pm.render(cloud.verts, FRONT, None, cloud.colors)
    r = HipRenderer3D(n_views=1, verbose=False)
    e3 = HipEstimator3D(verbose=False)
    lib, h = r.ctx.lib, r.ctx.handle
    lm = face.verts[:4].astype(np.float64)
    dev = torch.device("cuda", r.ctx.device)

    def refused(call, match):
        with pytest.raises(ValueError, match=match):
            call()
        msg = lib.mvlm_last_error(h).decode()
        assert msg and "point cloud" in msg, msg
        np.testing.assert_array_equal(_hip(cloud, FRONT), want)             # ... and the context renders on

    refused(lambda: _hip(cloud, FRONT, shading="geometry"), "geometry shading of a point cloud")
    refused(lambda: _hip(cloud, FRONT, multisamples=4), "multisampled rendering of a point cloud")
    refused(lambda: r.render_landmark_view(cloud, lm, size=64), "landmark view: a point cloud")
    refused(lambda: r.render_ray_view(cloud, lm, lm, lm + 1.0, size=64), "ray view: a point cloud")
    refused(lambda: e3.clip_rays_to_mesh(cloud, lm[None], lm[None] + 1.0), "ray clipping against a point cloud")
    refused(lambda: e3.attach_landmarks_to_surface(cloud, lm), "surface attachment of a point cloud")

    # the radius: out of range, not a number, on a mesh with triangles
    handle = upload_mesh(r.ctx, cloud)
    auto = C.c_double()
    assert lib.mvlm_mesh_point_radius(handle, C.byref(auto)) == 0 and auto.value == pm.auto_radius(cloud.verts)
    for bad in (0.75 * K - 0.01, 8.0 * K + 0.01, 0.0, -1.0, float("nan"), float("inf")):
        assert lib.mvlm_mesh_set_point_radius(h, handle, C.c_double(bad)) != 0
        assert "0.75 to 8 pixels" in lib.mvlm_last_error(h).decode()
    now = C.c_double()
    assert lib.mvlm_mesh_point_radius(handle, C.byref(now)) == 0 and now.value == auto.value     # a refused radius changes nothing
    np.testing.assert_array_equal(_hip(cloud, FRONT), want)
    for good in (0.75 * K, 8.0 * K):
        assert lib.mvlm_mesh_set_point_radius(h, handle, C.c_double(good)) == 0
    assert lib.mvlm_mesh_set_point_radius(h, handle, C.c_double(auto.value)) == 0
    tri_mesh = Mesh(face.verts, face.tris)
    tri_handle = upload_mesh(r.ctx, tri_mesh)
    assert lib.mvlm_mesh_set_point_radius(h, tri_handle, C.c_double(3.0)) != 0
    assert "has triangles" in lib.mvlm_last_error(h).decode()
    assert lib.mvlm_mesh_point_radius(tri_handle, C.byref(now)) != 0
    with pytest.raises(ValueError, match="0.75 to 8 pixels"):
        _hip(_cloud(face.verts, radius=20.0), FRONT)

    # a cloud takes no texture: the JPEG and the decoded-texture upload entries refuse n_tris == 0
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(face.texture).save(buf, format="JPEG")
    raw = np.frombuffer(buf.getvalue(), np.uint8)
    verts = np.ascontiguousarray(face.verts)
    out = C.c_void_p()
    assert lib.mvlm_mesh_upload_jpeg(h, _lib.as_ptr(verts, C.c_float), _lib.as_ptr(face.uvs, C.c_float), face.n_verts, None, 0,
                                     _lib.as_ptr(raw, C.c_uint8), raw.size, C.byref(out)) == 1
    assert "point cloud" in lib.mvlm_last_error(h).decode() and not out.value
    tex = C.c_void_p()
    assert lib.mvlm_texture_from_jpeg(h, _lib.as_ptr(raw, C.c_uint8), raw.size, C.byref(tex)) == 0
    consumed = C.c_int(-1)
    assert lib.mvlm_mesh_upload_texture(h, _lib.as_ptr(verts, C.c_float), _lib.as_ptr(face.uvs, C.c_float), face.n_verts, None, 0,
                                        tex, C.byref(consumed), C.byref(out)) == 1
    assert "point cloud" in lib.mvlm_last_error(h).decode() and consumed.value == 0 and not out.value
    lib.mvlm_texture_free(h, tex)
    # ... while mvlm_mesh_upload ignores uvs and a texture given with a cloud
    textured_cloud = Mesh(face.verts, NO_TRIS, face.uvs, face.texture, colors=face.colors)
    np.testing.assert_array_equal(_hip(textured_cloud, FRONT), want)
    del dev


def test_the_pipeline_says_what_a_cloud_cannot_do(tmp_path):
    from mvlm_amd import config, pipeline
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=41, tex_size=64, seed=2, vertex_colors=True)
    obj = tmp_path / "cloud.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in face.verts.astype(np.float64)) + "\n")
    for kw, match in (({"landmark_report": True}, "landmark_report"), ({"visualize_img": True}, "visualize_img"),
                      ({"visualize_rays_img": True}, "visualize_rays_img"), ({"render_multisamples": 4}, "render_multisamples")):
        pipe = pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, **kw)
        with pytest.raises(ValueError, match=match):
            pipe.predict_one_file(obj)
        with pytest.raises(ValueError, match=match):
            pipe.predict_mesh_device(_cloud(face.verts), pipe.renderer_3d.generate_3d_transformations())
        with pytest.raises(ValueError, match=match):
            list(pipe.predict_files([obj]))
    pipe = pipeline_from_config(config.default_config("DTU3D", "geometry", n_views=8), weights="synthetic:5", verbose=False)
    with pytest.raises(ValueError, match="geometry"):
        pipe.predict_one_file(obj)


# ---- 5. every layer --------------------------------------------------------------------------------------------------------
def test_a_coloured_cloud_goes_through_every_layer(tmp_path):
    from mvlm_amd import pipeline
    from mvlm_amd.__main__ import main
    from mvlm_amd.utils import load_mesh
    from mvlm_amd.utils.mesh_io import load_obj
    from mvlm_amd.utils.synthetic import write_face_like_obj

    full = load_obj(write_face_like_obj(tmp_path / "full.obj", grid=41, tex_size=64, seed=2, vertex_colors=True))
    work = tmp_path / "scan"
    work.mkdir()
    obj = work / "f.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f} {r:.6f} {g:.6f} {b:.6f}" for (x, y, z), (r, g, b)
                             in zip(full.verts.astype(np.float64), full.colors.astype(np.float64) / 255.0)) + "\n")
    ref = load_obj(obj)
    assert ref.n_tris == 0 and ref.n_verts == full.n_verts and len(np.unique(ref.colors, axis=0)) > 100
    pipe = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False)
    np.random.seed(3)
    images, poses, mesh = pipe.renderer_3d.multiview_render(obj)          # the slot protocol
    want = pm.render(ref.verts, poses, None, ref.colors)
    np.testing.assert_array_equal(images, want)
    assert (images[..., :3] != 1.0).any(-1).mean() > 0.1                  # not white
    np.random.seed(3)
    fused, _ = pipe.predict_mesh_device(mesh, poses)                      # the fused path
    np.random.seed(3)
    lms, _ = pipe.predictor_2d.predict_landmarks_from_images(images)
    starts, ends = pipe.estimator_3d.estimate_landmark_lines(images, lms, poses)
    raw, _ = pipe.estimator_3d.estimate_landmarks_from_lines(lms, starts, ends)
    np.testing.assert_array_equal(fused, pipe.estimator_3d.project_landmarks_to_surface(mesh, raw))
    np.testing.assert_array_equal(fused, pm.nearest(ref.verts, raw))
    np.random.seed(3)
    one = pipe.predict_one_file(obj)
    assert one.shape == (73, 3) and np.isfinite(one).all()
    grouped = pipe.predict_meshes_device([load_obj(obj), load_obj(obj)])  # clouds go one by one
    assert len(grouped) == 2 and all(np.isfinite(lm).all() for lm, _ in grouped)
    out = tmp_path / "out"
    args = ["-p", str(work), "-o", str(out), "-n", "8", "--weights", "synthetic:1", "--pipelines", "dtu3d", "--seed", "2"]
    assert main(args) == 0
    lm = np.loadtxt(out / "f_dtu3d.txt", delimiter=",")
    assert lm.shape == (73, 3) and np.isfinite(lm).all()
    out3 = tmp_path / "out3"
    assert main(args[:2] + ["-o", str(out3)] + args[4:] + ["--point-radius", "3.0"]) == 0
    assert np.loadtxt(out3 / "f_dtu3d.txt", delimiter=",").shape == (73, 3)
    # a radius of the user's: other images, the model's at that radius
    wide = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False, point_radius=3.0)
    np.random.seed(3)
    images3, poses3, mesh3 = wide.renderer_3d.multiview_render(obj)
    np.testing.assert_array_equal(poses3, poses)
    assert mesh3.point_radius == 3.0 and not np.array_equal(images3, images)
    np.testing.assert_array_equal(images3, pm.render(ref.verts, poses, 3.0, ref.colors))
    # the same cloud as a binary .ply through load_mesh -> render_device, and with a radius changed after the upload
    with open(tmp_path / "f.ply", "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {ref.n_verts}\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode())
        rec = np.zeros(ref.n_verts, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
        rec["p"], rec["c"] = ref.verts, ref.colors
        f.write(rec.tobytes())
    ply = load_mesh(tmp_path / "f.ply")
    assert ply.n_tris == 0
    np.testing.assert_array_equal(ply.colors, ref.colors)
    np.testing.assert_array_equal(pipe.renderer_3d.render_device(ply, poses).cpu().numpy(), images)
    ply.point_radius = 3.0
    np.testing.assert_array_equal(pipe.renderer_3d.render_device(ply, poses).cpu().numpy(), images3)
    ply.point_radius = None
    np.testing.assert_array_equal(pipe.renderer_3d.render_device(ply, poses).cpu().numpy(), images)
    pipe.renderer_3d.check()
    lm_ply, _ = pipe.predict_mesh_device(ply, poses)
    assert np.isfinite(lm_ply).all()


def test_a_pre_aligned_cloud_gets_its_radius_from_the_aligned_points(tmp_path):
    from mvlm_amd.utils import HipRenderer3D
    from mvlm_amd.utils.prealign import apply_prealign
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=30, tex_size=16, seed=3)
    block = {"align_center_of_mass": True, "rot_x": 0, "rot_y": 0, "rot_z": 0, "scale": 2.0}
    small = (face.verts.astype(np.float64) / 2.0 + [30.0, -10.0, 5.0]).astype(np.float32)
    obj = tmp_path / "small.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in small.astype(np.float64)) + "\n")
    r = HipRenderer3D(n_views=1, verbose=False)
    r.pre_align = block
    mesh = r.load_mesh(obj)
    assert mesh.n_tris == 0 and mesh.to_original is not None
    from mvlm_amd.utils.mesh_io import load_obj

    want_verts = apply_prealign(load_obj(obj), block)[0].verts
    np.testing.assert_array_equal(mesh.verts, want_verts)
    got = r.render_device(mesh, FRONT).cpu().numpy()
    r.check()
    np.testing.assert_array_equal(got, pm.render(want_verts, FRONT))            # (the automatic radius of the ALIGNED points)
    assert pm.auto_radius(want_verts) > pm.auto_radius(small)


# ---- 6. the planted detector -----------------------------------------------------------------------------------------------
def test_what_dropping_the_faces_does_to_the_landmarks():
    """The planted-peak detector end to end on the coloured triangle mesh (the yardstick: test_what_colours_do_to_the_landmarks)
    and on the same vertices and colours without faces.  Both take the inlier branch for every landmark; the cloud's median
    distance to the planted truth is at most the yardstick's plus twice the cloud's radius - one radius for how far a splat can
    move an image feature, one for snapping to a point instead of the surface."""
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils import Mesh
    from test_planted_cpu import planted_scene

    mesh, pts, sd, poses = planted_scene(n_views=48)
    tex = mesh.texture
    th, tw = tex.shape[:2]
    tx = np.clip((mesh.uvs[:, 0] * tw).astype(np.int64), 0, tw - 1)
    ty = np.clip((mesh.uvs[:, 1] * th).astype(np.int64), 0, th - 1)
    colors = np.ascontiguousarray(tex[th - 1 - ty, tx])
    pipe = pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=48), weights=sd, verbose=False)
    lm, err = {}, {}
    for name, m in (("mesh", Mesh(mesh.verts, mesh.tris, colors=colors)), ("cloud", _cloud(mesh.verts, colors))):
        np.random.seed(1)
        lm[name], err[name] = pipe.predict_mesh_device(m, poses)
    radius = pm.auto_radius(mesh.verts)
    med = {name: float(np.median(np.linalg.norm(lm[name] - pts, axis=1))) for name in lm}
    print(f"median distance to the planted truth: coloured mesh {med['mesh']:.3f}, cloud {med['cloud']:.3f} model units "
          f"(cloud radius {radius:.3f} = {pm.radius_steps(radius) / 256.0:.3f} px); RANSAC error {err['mesh']:.3f} / {err['cloud']:.3f}")
    assert err["mesh"] < 10.0 and err["cloud"] < 10.0                       # the inlier branch for every landmark
    assert med["cloud"] <= med["mesh"] + 2.0 * radius
