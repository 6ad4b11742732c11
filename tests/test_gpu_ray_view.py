"""-m gpu: mvlm_render_ray_view (raster_rays.hip) through the C ABI - against the CPU model of the contract
(tests/native/ray_view.c) bit for bit, against mvlm_render_landmark_view where the contract says the two are equal (no rays; a ray
seen end-on), its argument checks, and that it leaves mvlm_render and mvlm_render_landmark_view alone.

What "equal to the model" compares: the image, the per-landmark and the per-ray pixel counts.  Every case asserts that the thing it
is about shows in the model's winner plane.  The tile kernel's LDS ray list holds RAYS_CAP = 256 rays at a time (raster_rays.hip);
`many_identical` puts 600 on one tile."""
import ctypes as C

import numpy as np
import pytest

import ray_model
import vcolor_contract
import view_model
from gl_contract import load

pytestmark = pytest.mark.gpu

_, SCENES = load()
_, COLOURED = vcolor_contract.load()
RAY_LIST_CAPACITY = 256     # RAYS_CAP of raster_rays.hip
UNIT = (0.0, 0.0, 128.0)    # at S = 256: k = 1, a pixel is a model unit, window = model + 128
FRONT = [[0.0, 0.0, 0.0]]
THREE = [[0.0, 0.0, 0.0], [10.0, -60.0, 5.0], [-25.0, 40.0, -10.0]]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("ray_model_gpu")
    view_model.load(d)
    ray_model.load(d)
    return ray_model.render


def _renderer(bits=8, shading="texture"):
    from mvlm_amd.utils import HipRenderer3D

    return HipRenderer3D(n_views=1, verbose=False, subpixel_bits=bits, shading=shading)


def _set_mode(r):
    lib, h = r.ctx.lib, r.ctx.handle
    r.ctx.check(lib.mvlm_set_render_shading(h, 1 if r.shading == "geometry" else 0))
    r.ctx.check(lib.mvlm_set_render_subpixel_bits(h, r.subpixel_bits))
    r.ctx._render_mode = None


def _call(r, mesh, poses, size, frame, landmarks=None, radius=0.0, rgb=None, starts=None, ends=None, ray_radius=0.5, ray_rgb=None,
          out=None, n_rays=None, null_rays=False):
    """mvlm_render_ray_view itself -> (rc, image u8 [n,S,S,4], lm counts i32 [n,NL], ray counts i32 [n,NR]) (device tensors)"""
    import torch

    from mvlm_amd import _lib
    from mvlm_amd.utils.render3d import upload_mesh

    rot = view_model.rotations(poses)
    n = rot.shape[0]
    fr = view_model.frames_for(n, frame)
    lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3) if landmarks is not None else np.zeros((0, 3))
    nl = lm.shape[0]
    col = np.ascontiguousarray(rgb, np.uint8).reshape(nl, 3) if rgb is not None else None
    a = np.ascontiguousarray(starts, np.float64).reshape(-1, 3) if starts is not None else np.zeros((0, 3))
    b = np.ascontiguousarray(ends, np.float64).reshape(-1, 3) if ends is not None else np.zeros((0, 3))
    nr = a.shape[0]
    rcol = np.ascontiguousarray(ray_rgb, np.uint8).reshape(nr, 3) if ray_rgb is not None else None
    dev = torch.device("cuda", r.ctx.device)
    a_dev, b_dev = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    if out is None:
        out = torch.empty((n, size, size, 4), dtype=torch.uint8, device=dev)
    counts = torch.full((n, max(nl, 1)), -7, dtype=torch.int32, device=dev)
    rcounts = torch.full((n, max(nr, 1)), -7, dtype=torch.int32, device=dev)
    handle = upload_mesh(r.ctx, mesh)
    r.ctx.bind_current_stream(torch, dev)
    _set_mode(r)
    rc = r.ctx.lib.mvlm_render_ray_view(
        r.ctx.handle, handle, _lib.as_ptr(rot, C.c_double), n, size, _lib.as_ptr(fr, C.c_float),
        _lib.as_ptr(lm, C.c_double) if nl else None, nl, C.c_float(radius), None if col is None else _lib.as_ptr(col, C.c_uint8),
        C.c_void_p(a_dev.data_ptr()) if nr and not null_rays else None, C.c_void_p(b_dev.data_ptr()) if nr and not null_rays else None,
        nr if n_rays is None else n_rays, C.c_float(ray_radius), None if rcol is None else _lib.as_ptr(rcol, C.c_uint8),
        C.c_void_p(out.data_ptr()), C.c_void_p(counts.data_ptr()) if nl else None, C.c_void_p(rcounts.data_ptr()) if nr else None)
    r.ctx.synchronize()  # (a_dev / b_dev stay alive until the kernels have read them)
    return rc, out, counts[:, :nl], rcounts[:, :nr]


def _view(r, mesh, poses, size, frame, **kw):
    rc, out, counts, rcounts = _call(r, mesh, poses, size, frame, **kw)
    r.ctx.check(rc)
    img, cnt, rcnt = out.cpu().numpy(), counts.cpu().numpy(), rcounts.cpu().numpy()
    r.check()
    return img, cnt, rcnt


def _landmark_view(r, mesh, poses, size, frame, landmarks=None, radius=0.0, rgb=None):
    import torch

    from mvlm_amd import _lib
    from mvlm_amd.utils.render3d import upload_mesh

    rot = view_model.rotations(poses)
    n = rot.shape[0]
    fr = view_model.frames_for(n, frame)
    lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3) if landmarks is not None else np.zeros((0, 3))
    nl = lm.shape[0]
    col = np.ascontiguousarray(rgb, np.uint8).reshape(nl, 3) if rgb is not None else None
    dev = torch.device("cuda", r.ctx.device)
    out = torch.empty((n, size, size, 4), dtype=torch.uint8, device=dev)
    counts = torch.zeros((n, max(nl, 1)), dtype=torch.int32, device=dev)
    handle = upload_mesh(r.ctx, mesh)
    r.ctx.bind_current_stream(torch, dev)
    _set_mode(r)
    r.ctx.check(r.ctx.lib.mvlm_render_landmark_view(
        r.ctx.handle, handle, _lib.as_ptr(rot, C.c_double), n, size, _lib.as_ptr(fr, C.c_float),
        _lib.as_ptr(lm, C.c_double) if nl else None, nl, C.c_float(radius), None if col is None else _lib.as_ptr(col, C.c_uint8),
        C.c_void_p(out.data_ptr()), C.c_void_p(counts.data_ptr()) if nl else None))
    img, cnt = out.cpu().numpy(), counts[:, :nl].cpu().numpy()
    r.check()
    return img, cnt


def _mesh(name, mode="textured"):
    from mvlm_amd.utils import Mesh

    sc = SCENES[name]
    if mode == "textured":
        return Mesh(sc["verts"], sc["tris"], sc["uvs"], sc["tex"]), dict(uvs=sc["uvs"], texture=sc["tex"], colors=None)
    if mode == "vcolor":
        col = COLOURED[name]["colors"]
        return Mesh(sc["verts"], sc["tris"], colors=col), dict(uvs=None, texture=None, colors=col)
    return Mesh(sc["verts"], sc["tris"]), dict(uvs=None, texture=None, colors=None)


def _quad_mesh():
    from mvlm_amd.utils import Mesh

    verts, tris = view_model.quad(0.0)
    return verts, tris, Mesh(verts, tris, colors=view_model.QUAD_COLOURS)


# ---- equal to the model -----------------------------------------------------------------------------------------------------
def _face_rays():
    """84 x 8 rays as oracle.estimator draws them from seeded heat-map maxima of eight seeded poses, clipped to face40's surface"""
    from oracle.estimator import estimate_landmark_lines
    from oracle.surface import clip_rays_to_mesh

    sc = SCENES["face40"]
    rs = np.random.RandomState(11)
    poses = rs.uniform(-40.0, 40.0, (8, 3))
    stack = np.concatenate([rs.uniform(70.0, 186.0, (84, 8, 2)), np.ones((84, 8, 1))], axis=2).astype(np.float32)
    starts, ends = estimate_landmark_lines(256, stack, poses)
    ends, hit = clip_rays_to_mesh(np.asarray(sc["verts"]), np.asarray(sc["tris"]), starts, ends)
    assert hit.any()
    return starts.reshape(-1, 3), ends.reshape(-1, 3)


def _cases():
    c = {}
    # name: dict(starts, ends, ray_radius, [ray_rgb, landmarks, radius, rgb])   -- the quad at S = 256 with the unit frame
    c["horizontal_over_tile_borders"] = dict(starts=[[-90.0, 10.3, 5.0]], ends=[[90.0, 10.3, 5.0]], ray_radius=2.0)
    c["corner_to_corner"] = dict(starts=[[-128.0, -128.0, 5.0]], ends=[[128.0, 128.0, 9.0]], ray_radius=1.5)
    c["end_on"] = dict(starts=[[10.0, 20.0, 5.0]], ends=[[10.0, 20.0, 60.0]], ray_radius=4.0)
    for name, length in (("length_1e-4", 1e-4), ("length_1e-2", 1e-2), ("length_1", 1.0)):
        c[name] = dict(starts=[[10.0, 20.0, 5.0]], ends=[[10.0 + length, 20.0, 30.0]], ray_radius=4.0)
    c["zero_length"] = dict(starts=[[3.0, 4.0, 5.0]], ends=[[3.0, 4.0, 5.0]], ray_radius=3.0)
    c["radius_under_half_a_pixel"] = dict(starts=[[-50.0, 0.5, 5.0], [-40.0, -30.0, 5.0]], ends=[[50.0, 0.5, 5.0], [40.0, -22.0, 5.0]],
                                          ray_radius=0.3)
    c["pierces_the_quad"] = dict(starts=[[-60.0, 0.0, -30.0]], ends=[[60.0, 7.0, 30.0]], ray_radius=3.0)
    c["in_the_quads_plane"] = dict(starts=[[-60.0, -20.0, 0.0], [-60.0, 20.5, -2.0]], ends=[[60.0, -20.0, 0.0], [60.0, 20.5, -2.0]],
                                   ray_radius=2.0)
    c["through_a_sphere"] = dict(starts=[[-40.0, 0.0, 5.0]], ends=[[40.0, 0.0, 5.0]], ray_radius=2.0, landmarks=[[0.0, 0.0, 5.0]],
                                 radius=6.0)
    # crests at the same height, no equal depth at a pixel centre: on the shared pixels the sphere is nearer on some, the ray on others
    c["grazing_a_sphere"] = dict(starts=[[-40.0, 0.0, 9.0]], ends=[[40.0, 0.0, 9.0]], ray_radius=2.0, landmarks=[[0.0, 0.0, 5.0]],
                                 radius=6.0)
    # THE TIE WITH SPHERES: a ray drawn from its caps whose nearer end is the landmark, with the sphere's radius - the caps use the
    # sphere's arithmetic, so every covered pixel has the sphere's depth bit for bit, and the sphere, drawn later, owns them all
    c["equal_depth_with_a_sphere_end_on"] = dict(starts=[[10.3, 20.6, 5.0]], ends=[[10.3, 20.6, -40.0]], ray_radius=4.0,
                                                 ray_rgb=[[250, 10, 10]], landmarks=[[10.3, 20.6, 5.0]], radius=4.0)
    c["equal_depth_with_a_sphere_zero_length"] = dict(starts=[[-30.0, 7.5, 6.0], [50.0, 50.0, 3.0]], ends=[[-30.0, 7.5, 6.0], [70.0, 50.0, 3.0]],
                                                      ray_radius=3.0, ray_rgb=[[250, 10, 10], [10, 250, 10]],
                                                      landmarks=[[-30.0, 7.5, 6.0]], radius=3.0)
    c["coincident_rays"] = dict(starts=[[-30.0, 40.0, 5.0]] * 2, ends=[[30.0, 50.0, 8.0]] * 2, ray_radius=2.5,
                                ray_rgb=[[255, 0, 0], [0, 0, 255]])
    c["many_identical"] = dict(starts=[[20.0, -20.0, 3.0]] * 600, ends=[[27.0, -17.0, 4.0]] * 600, ray_radius=2.0,
                               ray_rgb=np.random.RandomState(5).randint(0, 256, (600, 3)))
    c["from_9000_units_outside"] = dict(starts=[[-9000.0, -3000.0, 5.0]], ends=[[200.0, 150.0, 5.0]], ray_radius=2.0)
    c["crosses_the_near_clip"] = dict(starts=[[-50.0, -20.0, 400.0]], ends=[[50.0, -20.0, 600.0]], ray_radius=2.0)
    c["nan_between_two_good_ones"] = dict(starts=[[-50.0, 30.0, 5.0], [-50.0, 40.0, 5.0], [-50.0, 50.0, 5.0]],
                                          ends=[[50.0, 30.0, 5.0], [50.0, float("nan"), 5.0], [50.0, 50.0, 5.0]], ray_radius=2.0)
    return c


CASES = _cases()
assert len(CASES["many_identical"]["starts"]) > RAY_LIST_CAPACITY


def _check(want, got, winner):
    w_img, w_cnt, w_rcnt = want
    g_img, g_cnt, g_rcnt = got
    nr = w_rcnt.shape[1]
    rays = ray_model.ray_of(winner)
    hist = np.stack([np.bincount(r[r >= 0].ravel(), minlength=nr)[:nr] for r in rays]) if nr else w_rcnt
    np.testing.assert_array_equal(w_rcnt, hist)  # (the model's own counts are its winners' histogram)
    np.testing.assert_array_equal(g_img, w_img)
    np.testing.assert_array_equal(g_cnt, w_cnt)
    np.testing.assert_array_equal(g_rcnt, w_rcnt)


@pytest.mark.parametrize("case", sorted(CASES))
def test_quad_cases_equal_the_model_bit_for_bit(model, case):
    kw = dict(CASES[case])
    verts, tris, mesh = _quad_mesh()
    lm, radius, rgb = kw.pop("landmarks", None), kw.pop("radius", 0.0), kw.pop("rgb", None)
    w_img, w_cnt, w_rcnt, winner, depth = model(verts, tris, None, None, FRONT, 256, frame=UNIT, landmarks=lm, radius=radius,
                                                lm_rgb=rgb, colors=view_model.QUAD_COLOURS, **kw)
    got = _view(_renderer(), mesh, FRONT, 256, UNIT, landmarks=lm, radius=radius, rgb=rgb, **kw)
    rays = ray_model.ray_of(winner)
    print(case, "mesh pixels", int((winner >= 0).sum()), "ray pixels", int((rays >= 0).sum()), "per ray", w_rcnt[0][:8])
    _check((w_img, w_cnt, w_rcnt), got, winner)
    for t in (0, 1):  # the quad: the pixel's colour is its winning triangle's
        assert (winner == t).any() and (w_img[winner == t][:, :3] == view_model.QUAD_COLOURS[3 * t]).all()
    assert (rays >= 0).any() or case == "equal_depth_with_a_sphere_end_on", "the case draws no ray"   # (there the sphere owns every pixel)
    cnt = w_rcnt[0]
    mesh_z = np.float32(500.0) / np.float32(1500.0)
    if case == "horizontal_over_tile_borders":
        cols = np.nonzero((rays[0] == 0).any(axis=0))[0]
        assert cols.min() // 16 + 5 <= cols.max() // 16          # several tile borders
    if case == "corner_to_corner":
        assert (rays[0][0, -3:] == 0).any() and (rays[0][-1, :3] == 0).any()   # top right and bottom left of the image
    if case == "pierces_the_quad":
        cols = np.nonzero((rays[0] == 0).any(axis=0))[0]
        assert 110 < cols.min() and cols.max() > 180 and winner[0][127, 80] >= 0   # in front on the right, hidden on the left
    if case == "in_the_quads_plane":
        assert cnt[0] > 0 and cnt[1] > 0                         # the second one's crest lies in the plane: the tie with the mesh
        assert (depth[0][rays[0] == 1] == mesh_z).any()
    if case in ("through_a_sphere", "grazing_a_sphere"):
        assert (winner <= -2).any() and (winner > ray_model.RAY_CODE_BASE).any() and cnt[0] > 0
    if case.startswith("equal_depth_with_a_sphere"):
        # from a ray-only and a sphere-only picture: equal depths exist on shared pixels; the sphere owns all of them
        ray_only = model(verts, tris, None, None, FRONT, 256, frame=UNIT, colors=view_model.QUAD_COLOURS, **kw)
        sph_only = model(verts, tris, None, None, FRONT, 256, frame=UNIT, landmarks=lm, radius=radius, lm_rgb=rgb,
                         colors=view_model.QUAD_COLOURS)
        shared = (ray_model.ray_of(ray_only[3]) == 0) & (sph_only[3] == -2)
        assert shared.sum() > 20 and (ray_only[4][shared] == sph_only[4][shared]).all()
        assert (ray_model.ray_of(ray_only[3]) == 0).sum() == shared.sum() == (sph_only[3] == -2).sum()
        assert (winner[shared] == -2).all() and cnt[0] == 0 and got[2][0, 0] == 0 and got[1][0, 0] == shared.sum()
        np.testing.assert_array_equal(got[0], sph_only[0] if len(cnt) == 1 else got[0])   # one ray: the picture is the sphere's
    if case == "coincident_rays":
        assert cnt[0] == 0 and cnt[1] > 0
    if case == "many_identical":
        assert cnt[-1] > 0 and (cnt[:-1] == 0).all()
    if case == "crosses_the_near_clip":
        cols = np.nonzero((rays[0] == 0).any(axis=0))[0]
        assert cols.min() <= 78 and 120 < cols.max() < 130       # drawn from x = -50 up to zv = 500 (x = 0, column 128) only
    if case == "nan_between_two_good_ones":
        assert cnt[1] == 0 and cnt[0] > 0 and cnt[0] == cnt[2]
    if case in ("end_on", "zero_length", "length_1e-4", "length_1e-2"):
        assert abs(int(cnt[0]) - np.pi * kw["ray_radius"] ** 2) < 12   # a disc


@pytest.fixture(scope="module")
def face_rays():
    return _face_rays()


@pytest.mark.parametrize("size", [400, 64])
def test_face_with_the_estimators_clipped_rays_equals_the_model(model, face_rays, size):
    sc = SCENES["face40"]
    mesh, extra = _mesh("face40", "textured")
    lm = view_model.surface_landmarks(sc["verts"], 84)
    fit = np.array([view_model.fit_frame(sc["verts"], lm, p) for p in THREE])
    starts, ends = face_rays
    assert starts.shape == (84 * 8, 3)
    kw = dict(landmarks=lm, radius=2.5, starts=starts, ends=ends, ray_radius=0.5)
    w_img, w_cnt, w_rcnt, winner, _ = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], THREE, size, frame=fit, **kw)
    got = _view(_renderer(), mesh, THREE, size, fit, **kw)
    print(size, "ray pixels", int((ray_model.ray_of(winner) >= 0).sum()), "rays visible", int((w_rcnt > 0).sum()))
    _check((w_img, w_cnt, w_rcnt), got, winner)
    assert (winner >= 0).any() and (winner <= -2).any() and (w_rcnt > 0).sum() > 84


def test_geometry_shading_and_four_subpixel_bits_follow_the_model(model, face_rays):
    sc = SCENES["face40"]
    mesh, extra = _mesh("face40", "textured")
    lm = view_model.surface_landmarks(sc["verts"], 20, 3)
    frame = view_model.fit_frame(sc["verts"], lm, FRONT[0])
    starts, ends = face_rays[0][:160], face_rays[1][:160]
    kw = dict(landmarks=lm, radius=3.0, starts=starts, ends=ends, ray_radius=0.7)
    w_img, w_cnt, w_rcnt, winner, _ = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], FRONT, 400, frame=frame, shading="geometry",
                                            subpixel_bits=4, **kw)
    got = _view(_renderer(4, "geometry"), mesh, FRONT, 400, frame, **kw)
    _check((w_img, w_cnt, w_rcnt), got, winner)
    assert (ray_model.ray_of(winner) >= 0).any()


# ---- list overflow ----------------------------------------------------------------------------------------------------------
def test_list_overflow_is_reported_and_the_next_view_is_clean(model, face_rays):
    """At S = 64 a view has 16 tiles and 4 * 16 + 8 * 16 = 192 list entries; 16 big triangles on all 16 tiles ask for 256.  The
    call returns 0 (the scatter drops what does not fit), mvlm_render_check says "overflowed", and the ray view after it on the
    same renderer is the model's bit for bit with a clean check."""
    from mvlm_amd import _lib
    from mvlm_amd.utils import Mesh

    n = 16  # test_gpu_round6.py's overflow triangles: each covers the whole window of a frame of half 50 about the origin
    rs = np.random.RandomState(2)
    verts = np.concatenate([np.array([[-400, -400, z], [400, -400, z], [0, 600, z]], np.float32) for z in rs.uniform(-50, 50, n)])
    huge = Mesh(verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3))
    r = _renderer()
    rc, _, _, _ = _call(r, huge, FRONT, 64, (0.0, 0.0, 50.0))
    assert rc == 0
    with pytest.raises(_lib.MvlmHipError, match="overflowed"):
        r.check()
    sc = SCENES["face40"]
    mesh, extra = _mesh("face40", "textured")
    lm = view_model.surface_landmarks(sc["verts"], 84)
    kw = dict(landmarks=lm, radius=4.0, starts=face_rays[0][:40], ends=face_rays[1][:40], ray_radius=0.5)
    w_img, w_cnt, w_rcnt, winner, _ = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], FRONT, 64, frame=view_model.NETWORK_FRAME, **kw)
    got = _view(r, mesh, FRONT, 64, view_model.NETWORK_FRAME, **kw)   # (_view's r.check() is clean)
    _check((w_img, w_cnt, w_rcnt), got, winner)
    assert (winner >= 0).any() and (ray_model.ray_of(winner) >= 0).any()


# ---- equal to mvlm_render_landmark_view --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["textured", "vcolor", "white"])
def test_no_rays_is_the_landmark_view_byte_for_byte(mode):
    sc = SCENES["face40"]
    r = _renderer()
    mesh, _ = _mesh("face40", mode)
    lm = view_model.surface_landmarks(sc["verts"], 84)
    fit = np.array([view_model.fit_frame(sc["verts"], lm, p) for p in THREE])
    rgb = np.random.RandomState(3).randint(0, 256, (84, 3))
    want, want_cnt = _landmark_view(r, mesh, THREE, 256, fit, lm, 2.5, rgb)
    got, cnt, _ = _view(r, mesh, THREE, 256, fit, landmarks=lm, radius=2.5, rgb=rgb)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cnt, want_cnt)
    assert (want_cnt > 0).any() and (want[..., :3] != 255).any()


def test_an_end_on_ray_is_the_sphere_at_its_nearer_end():
    verts, tris, mesh = _quad_mesh()
    r = _renderer()
    colour = [[200, 120, 30]]
    for a, b in (([10.0, 20.0, 5.0], [10.0, 20.0, 60.0]), ([-33.3, 7.7, 80.0], [-33.3, 7.7, -200.0])):
        near = a if a[2] > b[2] else b
        want, want_cnt = _landmark_view(r, mesh, FRONT, 256, UNIT, [near], 4.0, colour)
        got, _, rcnt = _view(r, mesh, FRONT, 256, UNIT, starts=[a], ends=[b], ray_radius=4.0, ray_rgb=colour)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(rcnt, want_cnt)
        assert want_cnt[0, 0] > 30


# ---- bad arguments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["negative_ray_radius", "nan_ray_radius", "too_many_rays", "too_many_records", "null_rays", "size_250",
                                  "negative_radius"])
def test_bad_arguments_return_an_error_and_launch_nothing(what):
    import torch

    r = _renderer()
    mesh, _ = _mesh("coarse")
    kw = dict(landmarks=[[0.0, 0.0, 0.0]], radius=2.0, starts=[[0.0, 0.0, 0.0]], ends=[[5.0, 5.0, 5.0]], ray_radius=1.0)
    size, poses = 64, FRONT
    if what == "negative_ray_radius":
        kw["ray_radius"] = -0.5
    elif what == "nan_ray_radius":
        kw["ray_radius"] = float("nan")
    elif what == "too_many_rays":
        kw["n_rays"] = 65537
    elif what == "too_many_records":
        kw["n_rays"], poses = 65536, np.zeros((17, 3))            # 17 x 65 536 > 1 048 576 records
    elif what == "null_rays":
        kw["null_rays"] = True
    elif what == "size_250":
        size = 250
    elif what == "negative_radius":
        kw["radius"] = -1.0
    out = torch.full((1, 64, 64, 4), 7, dtype=torch.uint8, device=torch.device("cuda", r.ctx.device))
    rc, out, counts, rcounts = _call(r, mesh, poses, size, UNIT, out=out, **kw)
    assert rc != 0
    assert r.ctx.lib.mvlm_last_error(r.ctx.handle).decode().startswith("ray view:")
    r.ctx.synchronize()
    assert (out.cpu().numpy() == 7).all() and (counts.cpu().numpy() == -7).all() and (rcounts.cpu().numpy() == -7).all()


# ---- the neighbours are left alone ------------------------------------------------------------------------------------------
def test_mvlm_render_and_the_landmark_view_after_a_ray_view_are_bit_equal(face_rays):
    sc = SCENES["face40"]
    poses = np.asarray(sc["poses"], np.float64)
    lm = view_model.surface_landmarks(sc["verts"], 84)
    for samples in (0, 4):
        r = _renderer()
        r.multisamples = samples
        mesh, _ = _mesh("face40")
        before = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        view_before, cnt_before = _landmark_view(r, mesh, poses[:2], 400, (10.0, -5.0, 120.0), lm, 3.0)
        _view(r, mesh, poses[:2], 256, (10.0, -5.0, 120.0), landmarks=lm, radius=3.0, starts=face_rays[0], ends=face_rays[1])
        after = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        view_after, cnt_after = _landmark_view(r, mesh, poses[:2], 400, (10.0, -5.0, 120.0), lm, 3.0)
        np.testing.assert_array_equal(after, before)
        np.testing.assert_array_equal(view_after, view_before)
        np.testing.assert_array_equal(cnt_after, cnt_before)
