"""-m gpu: mvlm_render_landmark_view (raster_view.hip) through the C ABI - against mvlm_render at the network's window, against
the CPU model of the contract (tests/native/landmark_view.c) bit for bit, its argument checks, and that it leaves mvlm_render
alone.

What "equal to the model" compares: the image and the per-landmark pixel counts.  The entry has no per-pixel winner output; the
model's winner plane is tied in through the counts, which must be its histogram of sphere winners, and through the image: the
face scenes are textured or coloured per vertex, and the quad's two triangles carry a colour each (view_model.QUAD_COLOURS), so a
pixel's colour names its winning triangle there.  Only `three_poses_three_frames` draws a white mesh (the white path).

The tile kernel's LDS sphere list holds VIEW_SPHERE_CAP = 256 spheres at a time (raster_view.hip); `many_at_one_point` puts 600
on one tile."""
import ctypes as C

import numpy as np
import pytest

import vcolor_contract
import view_model
from gl_contract import load

pytestmark = pytest.mark.gpu

_, SCENES = load()
_, COLOURED = vcolor_contract.load()
NAMES = ["face40", "coarse", "offscreen", "centres"]
SPHERE_LIST_CAPACITY = 256  # VIEW_SPHERE_CAP of raster_view.hip
UNIT = (0.0, 0.0, 128.0)    # at S = 256: k = 1, a pixel is a model unit
FRONT = [[0.0, 0.0, 0.0]]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    view_model.load(tmp_path_factory.mktemp("view_model_gpu"))
    return view_model.render


def _renderer(bits=8, shading="texture"):
    from mvlm_amd.utils import HipRenderer3D

    return HipRenderer3D(n_views=1, verbose=False, subpixel_bits=bits, shading=shading)


def _set_mode(r):
    lib, h = r.ctx.lib, r.ctx.handle
    r.ctx.check(lib.mvlm_set_render_shading(h, 1 if r.shading == "geometry" else 0))
    r.ctx.check(lib.mvlm_set_render_subpixel_bits(h, r.subpixel_bits))
    r.ctx._render_mode = None  # (the multisample setting is left as it is: the view does not read it)


def _call(r, mesh, poses, size, frame, landmarks=None, radius=0.0, rgb=None, out=None, want_counts=True):
    """mvlm_render_landmark_view itself -> (rc, image u8 [n,S,S,4] tensor, counts i32 [n,NL] tensor)"""
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
    if out is None:
        out = torch.empty((n, size, size, 4), dtype=torch.uint8, device=dev)
    counts = torch.full((n, max(nl, 1)), -7, dtype=torch.int32, device=dev)
    handle = upload_mesh(r.ctx, mesh)
    r.ctx.bind_current_stream(torch, dev)
    _set_mode(r)
    rc = r.ctx.lib.mvlm_render_landmark_view(
        r.ctx.handle, handle, _lib.as_ptr(rot, C.c_double), n, size, _lib.as_ptr(fr, C.c_float),
        _lib.as_ptr(lm, C.c_double) if nl else None, nl, C.c_float(radius), None if col is None else _lib.as_ptr(col, C.c_uint8),
        C.c_void_p(out.data_ptr()), C.c_void_p(counts.data_ptr()) if (want_counts and nl) else None)
    return rc, out, counts[:, :nl]


def _view(r, mesh, poses, size, frame, landmarks=None, radius=0.0, rgb=None):
    rc, out, counts = _call(r, mesh, poses, size, frame, landmarks, radius, rgb)
    r.ctx.check(rc)
    img, cnt = out.cpu().numpy(), counts.cpu().numpy()
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


# ---- equal to mvlm_render ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("name", NAMES)
def test_equal_to_mvlm_render_at_the_network_window(name, bits):
    poses = np.asarray(SCENES[name]["poses"], np.float64)
    for mode, shading in (("textured", "texture"), ("vcolor", "texture"), ("white", "texture"), ("textured", "geometry")):
        r = _renderer(bits, shading)
        mesh, _ = _mesh(name, mode)
        ref = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        want = np.round(ref[..., :3] * 255.0).astype(np.uint8)
        got, _ = _view(r, mesh, poses, 256, view_model.NETWORK_FRAME)
        np.testing.assert_array_equal(got[..., :3], want, err_msg=f"{mode} {shading}")
        assert (got[..., 3] == 255).all()
        assert name not in ("face40", "coarse") or mode == "white" or (want != 255).any()  # (something is drawn)


# ---- equal to the model -----------------------------------------------------------------------------------------------------
def _face_landmarks(n, seed=0):
    return view_model.surface_landmarks(SCENES["face40"]["verts"], n, seed)


def _cases():
    f40, coarse = SCENES["face40"], SCENES["coarse"]
    three = [[0.0, 0.0, 0.0], [10.0, -60.0, 5.0], [-25.0, 40.0, -10.0]]
    lm84 = _face_landmarks(84)
    fit = [view_model.fit_frame(f40["verts"], lm84, p) for p in three]
    quad = view_model.quad(0.0)
    c = {}
    # name: (scene or (verts, tris), mode, poses, size, frame, landmarks, radius, rgb)
    c["s64_subpixel_triangles"] = ("face40", "textured", three, 64, view_model.NETWORK_FRAME, lm84, 4.0, None)
    c["s400_fit"] = ("face40", "textured", three, 400, np.array(fit), lm84, 2.5, None)
    c["s1024_fit_478"] = ("face40", "textured", FRONT, 1024, fit[0], _face_landmarks(478, 1), 1.7, None)
    c["s2048_coarse_big_triangles"] = ("coarse", "textured", [coarse["poses"][0]], 2048, view_model.NETWORK_FRAME,
                                       view_model.surface_landmarks(coarse["verts"], 5), 6.0, None)
    c["off_centre_leaves_on_two_sides"] = ("face40", "vcolor", FRONT, 256, (60.0, 50.0, 70.0), lm84, 3.0, None)
    c["three_poses_three_frames"] = ("face40", "white", three, 128, np.array([[0, 0, 150], [30, -20, 90], [-40, 10, 200]], np.float32),
                                     lm84, 5.0, None)
    for n in (0, 1, 84, 478):
        c[f"n_lm_{n}"] = ("face40", "textured", three[:2], 256, np.array(fit[:2]), _face_landmarks(n, 2), 2.0,
                          None if n == 0 else np.random.RandomState(n).randint(0, 256, (n, 3)))
    c["window_corner"] = (quad, "white", FRONT, 256, UNIT, [[-127.0, 127.0, 5.0], [128.0, -128.0, 3.0]], 6.0, None)
    c["box_on_four_tiles"] = (quad, "white", FRONT, 256, UNIT, [[0.0, 0.0, 5.0], [16.0, -32.0, 1.0]], 3.0, None)
    c["radius_under_half_a_pixel"] = (quad, "white", FRONT, 256, UNIT, [[0.5, 0.5, 5.0], [3.0, 3.0, 5.0], [10.5, -7.5, 0.0]], 0.3, None)
    c["half_inside_the_surface"] = (quad, "white", FRONT, 256, UNIT, [[10.0, 10.0, 0.0], [-30.3, 5.2, -2.0], [40.0, -41.0, 2.5]], 5.0, None)
    c["equal_depths"] = (quad, "white", FRONT, 256, UNIT, [[7.0, 7.0, 4.0], [7.0, 7.0, 4.0], [12.0, 7.0, 4.0]], 5.0,
                         [[255, 0, 0], [0, 255, 0], [0, 0, 255]])
    c["many_at_one_point"] = (quad, "white", FRONT, 256, UNIT, np.tile([[20.0, -20.0, 3.0]], (600, 1)), 4.0,
                              np.random.RandomState(5).randint(0, 256, (600, 3)))
    return c


CASES = _cases()
assert len(CASES["many_at_one_point"][5]) > SPHERE_LIST_CAPACITY


@pytest.mark.parametrize("case", sorted(CASES))
def test_equal_to_the_model_bit_for_bit(model, case):
    from mvlm_amd.utils import Mesh

    scene, mode, poses, size, frame, lm, radius, rgb = CASES[case]
    if isinstance(scene, str):
        mesh, extra = _mesh(scene, mode)
        verts, tris = SCENES[scene]["verts"], SCENES[scene]["tris"]
    else:
        verts, tris = scene
        mesh, extra = Mesh(verts, tris, colors=view_model.QUAD_COLOURS), dict(uvs=None, texture=None, colors=view_model.QUAD_COLOURS)
    want, want_counts, winner = model(verts, tris, extra["uvs"], extra["texture"], poses, size, frame=frame, landmarks=lm,
                                      radius=radius, lm_rgb=rgb, colors=extra["colors"])
    got, counts = _view(_renderer(), mesh, poses, size, frame, lm, radius, rgb)
    nl = want_counts.shape[1]
    hist = np.stack([np.bincount((-2 - w[w <= -2]).ravel(), minlength=nl)[:nl] for w in winner]) if nl else want_counts
    np.testing.assert_array_equal(want_counts, hist)          # (the model's own counts are its winners' histogram)
    print(case, "mesh pixels", int((winner >= 0).sum()), "sphere pixels", int((winner <= -2).sum()), "visible", int((want_counts > 0).sum()))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(counts, want_counts)
    assert (winner >= 0).any()
    if not isinstance(scene, str):  # the quad: the pixel's colour is its winning triangle's
        for t in (0, 1):
            assert (winner == t).any() and (want[winner == t][:, :3] == view_model.QUAD_COLOURS[3 * t]).all()
    if nl:
        assert (winner <= -2).any()                           # a case that draws no sphere checks nothing of them
    if case == "many_at_one_point":
        assert counts[0, -1] > 0 and (counts[0, :-1] == 0).all()   # equal depths: the last one drawn wins every pixel
    if case == "equal_depths":
        assert counts[0, 0] == 0 and counts[0, 1] > 0 and counts[0, 2] > 0


def test_geometry_shading_and_four_subpixel_bits_follow_the_model(model):
    sc = SCENES["face40"]
    mesh, extra = _mesh("face40", "textured")
    lm = _face_landmarks(20, 3)
    frame = view_model.fit_frame(sc["verts"], lm, FRONT[0])
    for bits, shading in ((8, "geometry"), (4, "texture"), (4, "geometry")):
        want, wc, _ = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], FRONT, 400, frame=frame, landmarks=lm, radius=3.0,
                            shading=shading, subpixel_bits=bits)
        got, counts = _view(_renderer(bits, shading), mesh, FRONT, 400, frame, lm, 3.0)
        np.testing.assert_array_equal(got, want, err_msg=f"{bits} {shading}")
        np.testing.assert_array_equal(counts, wc)


# ---- list overflow ----------------------------------------------------------------------------------------------------------
def _window_filling_triangles(n=16):
    """n triangles that each cover the whole window of a frame of half 50 about the origin (test_gpu_round6.py's overflow mesh)"""
    from mvlm_amd.utils import Mesh

    rs = np.random.RandomState(2)
    verts = np.concatenate([np.array([[-400, -400, z], [400, -400, z], [0, 600, z]], np.float32) for z in rs.uniform(-50, 50, n)])
    return Mesh(verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3))


def test_list_overflow_is_reported_and_the_next_view_is_clean(model):
    """At S = 64 a view has 16 tiles and 4 * 16 + 8 * 16 = 192 list entries; 16 big triangles on all 16 tiles ask for 256.  The
    call returns 0 (the scatter drops what does not fit), mvlm_render_check says "overflowed", and the view after it on the same
    renderer is the model's bit for bit with a clean check."""
    from mvlm_amd import _lib

    r = _renderer()
    rc, _, _ = _call(r, _window_filling_triangles(), FRONT, 64, (0.0, 0.0, 50.0))
    assert rc == 0
    with pytest.raises(_lib.MvlmHipError, match="overflowed"):
        r.check()
    sc = SCENES["face40"]
    mesh, extra = _mesh("face40", "textured")
    lm = _face_landmarks(84)
    want, want_counts, winner = model(sc["verts"], sc["tris"], extra["uvs"], extra["texture"], FRONT, 64, frame=view_model.NETWORK_FRAME,
                                      landmarks=lm, radius=4.0)
    got, counts = _view(r, mesh, FRONT, 64, view_model.NETWORK_FRAME, lm, 4.0)   # (_view's r.check() is clean)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(counts, want_counts)
    assert (winner >= 0).any() and (winner <= -2).any()


# ---- bad arguments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["size_250", "size_4096", "half_0", "nan_landmark", "negative_radius", "nan_frame", "views_129"])
def test_bad_arguments_return_an_error_and_launch_nothing(what):
    import torch

    r = _renderer()
    mesh, _ = _mesh("coarse")
    size, frame, lm, radius = 64, UNIT, [[0.0, 0.0, 0.0]], 2.0
    if what == "size_250":
        size = 250
    elif what == "size_4096":
        size = 4096
    elif what == "half_0":
        frame = (0.0, 0.0, 0.0)
    elif what == "nan_landmark":
        lm = [[0.0, float("nan"), 0.0]]
    elif what == "negative_radius":
        radius = -1.0
    elif what == "nan_frame":
        frame = (float("nan"), 0.0, 100.0)
    poses = np.zeros((129, 3)) if what == "views_129" else FRONT
    out = torch.full((1, 64, 64, 4), 7, dtype=torch.uint8, device=torch.device("cuda", r.ctx.device))  # (never indexed by `size`)
    rc, out, counts = _call(r, mesh, poses, size, frame, lm, radius, out=out)
    assert rc != 0
    assert r.ctx.lib.mvlm_last_error(r.ctx.handle).decode().startswith("landmark view:")
    r.ctx.synchronize()
    assert (out.cpu().numpy() == 7).all() and (counts.cpu().numpy() == -7).all()


# ---- mvlm_render is left alone ----------------------------------------------------------------------------------------------
def test_mvlm_render_after_a_landmark_view_is_bit_equal():
    sc = SCENES["face40"]
    poses = np.asarray(sc["poses"], np.float64)
    for samples in (0, 4):
        r = _renderer()
        r.multisamples = samples
        mesh, _ = _mesh("face40")
        before = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        lm = _face_landmarks(84)
        _view(r, mesh, poses[:2], 400, (10.0, -5.0, 120.0), lm, 3.0)
        after = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        np.testing.assert_array_equal(after, before)
