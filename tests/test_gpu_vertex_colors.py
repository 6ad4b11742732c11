"""-m gpu: per-vertex colours (Mesh.colors, mvlm_mesh_upload_colors, raster_vc.hip) against the CPU model of the contract
(tests/native/vcolor_raster.c), against the OpenGL fixture (tests/golden/gl_raster_vcolor.npz), and through every layer."""
import ctypes as C

import numpy as np
import pytest

import vcolor_contract
import vcolor_model
from gl_contract import load

pytestmark = pytest.mark.gpu

_, SCENES = load()
META, COLOURED = vcolor_contract.load()
GL_BITS = META["gl"]["subpixel_bits"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    vcolor_model.load(tmp_path_factory.mktemp("vcolor_model"))
    return vcolor_model.render


def _hip(mesh, poses, bits=8, samples=0, shading="texture"):
    from mvlm_amd.utils import HipRenderer3D

    r = HipRenderer3D(n_views=len(poses), verbose=False, subpixel_bits=bits, multisamples=samples, shading=shading)
    out = r.render_device(mesh, poses).cpu().numpy()
    r.check()
    return out


def _coloured(name):
    """the geometry of a gl_raster.npz scene with the fixture's colours, every pose of the scene, no texture"""
    from mvlm_amd.utils import Mesh

    sc = SCENES[name]
    return Mesh(sc["verts"], sc["tris"], colors=COLOURED[name]["colors"]), sc["poses"]


@pytest.mark.parametrize("samples", [0, 4])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("name", ["face40", "coarse", "centres", "offscreen"])
def test_hip_equals_the_model_bit_for_bit(model, name, bits, samples):
    """face40: sub-pixel-free small triangles (classify's atomics, the 24-bit setup); coarse: triangles wider than 64 pixels (the
    64-bit setup, the binned path); centres: both windings (the b / c swap must swap the colours); offscreen: clipping"""
    mesh, poses = _coloured(name)
    want = model(mesh.verts, mesh.tris, None, None, poses, subpixel_bits=bits, samples=max(samples, 1), colors=mesh.colors)
    got = _hip(mesh, poses, bits, samples)
    np.testing.assert_array_equal(got, want)
    plain = model(mesh.verts, mesh.tris, None, None, poses, subpixel_bits=bits, samples=max(samples, 1))
    assert not np.array_equal(got[..., :3], plain[..., :3])
    np.testing.assert_array_equal(got[..., 3], plain[..., 3])           # the depth plane never sees a colour


@pytest.mark.parametrize("name", sorted(COLOURED))
def test_hip_against_the_opengl_fixture(name):
    from mvlm_amd.utils import Mesh
    from test_gl_vcolor_contract import INTERP_CAP, MEASURED

    sc = COLOURED[name]
    got = _hip(Mesh(sc["verts"], sc["tris"], colors=sc["colors"]), sc["poses"], GL_BITS, 0 if sc["samples"] == 1 else sc["samples"])
    r = vcolor_contract.compare(sc, got, GL_BITS)
    print(name, r)
    assert r["unexplained"] == 0, r
    clip, interp, ztie = MEASURED[name]
    assert r["clip"] <= clip and r["interp"] <= interp and r["ztie"] <= ztie, r
    assert r["interp"] <= INTERP_CAP * r["covered"], r


@pytest.mark.parametrize("samples", [0, 4])
def test_invariants(model, samples):
    from mvlm_amd.utils import Mesh

    sc = SCENES["face40"]
    n = len(sc["verts"])
    plain = _hip(Mesh(sc["verts"], sc["tris"]), sc["poses"], 8, samples)
    # all-255 colours: the white mesh, byte for byte
    white = _hip(Mesh(sc["verts"], sc["tris"], colors=np.full((n, 3), 255, np.uint8)), sc["poses"], 8, samples)
    np.testing.assert_array_equal(white, plain)
    # a constant colour stays constant bit for bit; uncovered pixels stay white; the depth plane is the uncoloured one
    const = _hip(Mesh(sc["verts"], sc["tris"], colors=np.tile(np.array([17, 200, 93], np.uint8), (n, 1))), sc["poses"], 8, samples)
    np.testing.assert_array_equal(const[..., 3], plain[..., 3])
    rgb = np.round(const[..., :3] * 255).astype(np.uint8)
    _, win_tri, _ = model(sc["verts"], sc["tris"], None, None, sc["poses"], samples=max(samples, 1), per_sample=True)
    full, none = (win_tri >= 0).all(-1)[:, ::-1], (win_tri < 0).all(-1)[:, ::-1]     # image rows
    assert full.any() and none.any()
    assert (rgb[full] == (17, 200, 93)).all() and (rgb[none] == 255).all()
    # texture + uvs + colours: the texture alone (precedence)
    some = np.random.RandomState(1).randint(0, 256, (n, 3)).astype(np.uint8)
    textured = _hip(Mesh(sc["verts"], sc["tris"], sc["uvs"], sc["tex"]), sc["poses"], 8, samples)
    both = Mesh(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], colors=some)
    np.testing.assert_array_equal(_hip(both, sc["poses"], 8, samples), textured)
    assert next(iter(both._device.values()))[2] is False               # (and the colours were not even uploaded)
    # uvs without a texture image: no usable texture, the colours show
    want = model(sc["verts"], sc["tris"], None, None, sc["poses"], samples=max(samples, 1), colors=some)
    np.testing.assert_array_equal(_hip(Mesh(sc["verts"], sc["tris"], sc["uvs"], None, colors=some), sc["poses"], 8, samples), want)
    # geometry shading ignores colours
    geo = _hip(Mesh(sc["verts"], sc["tris"]), sc["poses"], 8, samples, shading="geometry")
    np.testing.assert_array_equal(_hip(Mesh(sc["verts"], sc["tris"], colors=some), sc["poses"], 8, samples, shading="geometry"), geo)


def test_coloured_and_plain_meshes_alternate_on_one_context(model):
    """coloured, then an uncoloured mesh of the same size (its buffers come from the mesh pool), then coloured again, 0 and 4
    samples alternating: every render equals its own model - nothing of a previous mesh's colours shows"""
    from mvlm_amd.utils import HipRenderer3D, Mesh

    sc = SCENES["face40"]
    poses = sc["poses"][[0, 3]]
    rs = np.random.RandomState(5)
    r = HipRenderer3D(n_views=2, verbose=False)
    for k in range(6):
        colors = rs.randint(0, 256, (len(sc["verts"]), 3)).astype(np.uint8) if k % 2 == 0 else None
        r.multisamples = (0, 4)[(k // 2 + k) % 2]
        mesh = Mesh(sc["verts"], sc["tris"], colors=colors)
        got = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        want = model(sc["verts"], sc["tris"], None, None, poses, samples=max(r.multisamples, 1), colors=colors)
        np.testing.assert_array_equal(got, want, err_msg=f"step {k}")
        del mesh                                                       # its buffers go back to the pool for the next one


def test_upload_colors_rejects_bad_arguments():
    from mvlm_amd import _lib
    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.render3d import upload_mesh

    ctx = _lib.get_context(0)
    sc = SCENES["coarse"]
    mesh = Mesh(sc["verts"], sc["tris"])
    handle = upload_mesh(ctx, mesh)
    rgb = np.zeros((len(sc["verts"]) + 1, 3), np.uint8)
    assert ctx.lib.mvlm_mesh_upload_colors(ctx.handle, handle, _lib.as_ptr(rgb, C.c_uint8), len(sc["verts"]) + 1) != 0
    assert b"colours for a mesh of 9 points" in ctx.lib.mvlm_last_error(ctx.handle)
    assert ctx.lib.mvlm_mesh_upload_colors(ctx.handle, handle, None, len(sc["verts"])) != 0
    assert b"null pointer" in ctx.lib.mvlm_last_error(ctx.handle)
    assert ctx.lib.mvlm_mesh_upload_colors(ctx.handle, None, _lib.as_ptr(rgb, C.c_uint8), len(sc["verts"])) != 0
    with pytest.raises(ValueError, match="colours must be uint8"):
        upload_mesh(ctx, Mesh(sc["verts"], sc["tris"], colors=rgb))
    # the mesh is still what it was: white
    from oracle import raster

    np.testing.assert_array_equal(_hip(mesh, sc["poses"]), raster.multiview_render(sc["verts"], sc["tris"], None, None, sc["poses"]))


def test_a_coloured_obj_goes_through_every_layer(tmp_path, model):
    from mvlm_amd import pipeline
    from mvlm_amd.__main__ import main
    from mvlm_amd.utils import load_mesh
    from mvlm_amd.utils.mesh_io import load_obj
    from mvlm_amd.utils.synthetic import write_face_like_obj

    obj = write_face_like_obj(tmp_path / "f.obj", grid=41, tex_size=64, seed=2, vertex_colors=True)
    assert not obj.with_suffix(".jpg").exists()
    ref = load_obj(obj)
    assert ref.uvs is None and ref.colors is not None and len(np.unique(ref.colors, axis=0)) > 100
    pipe = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False)
    np.random.seed(3)
    images, poses, mesh = pipe.renderer_3d.multiview_render(obj)          # the slot protocol
    want = model(ref.verts, ref.tris, None, None, poses, colors=ref.colors)
    np.testing.assert_array_equal(images, want)
    assert (images[..., :3] != model(ref.verts, ref.tris, None, None, poses)[..., :3]).any(-1).mean() > 0.1   # not white
    np.random.seed(3)
    fused, _ = pipe.predict_mesh_device(mesh, poses)                      # the fused path
    np.random.seed(3)
    lms, _ = pipe.predictor_2d.predict_landmarks_from_images(images)
    starts, ends = pipe.estimator_3d.estimate_landmark_lines(images, lms, poses)
    raw, _ = pipe.estimator_3d.estimate_landmarks_from_lines(lms, starts, ends)
    np.testing.assert_array_equal(fused, pipe.estimator_3d.project_landmarks_to_surface(mesh, raw))
    np.random.seed(3)
    one = pipe.predict_one_file(obj)
    assert one.shape == (73, 3) and np.isfinite(one).all()
    out = tmp_path / "out"
    assert main(["-p", str(tmp_path), "-o", str(out), "-n", "8", "--weights", "synthetic:1", "--pipelines", "dtu3d", "--seed", "2"]) == 0
    lm = np.loadtxt(out / "f_dtu3d.txt", delimiter=",")
    assert lm.shape == (73, 3) and np.isfinite(lm).all()
    # the same mesh as a coloured .ply through load_mesh -> render_device
    with open(tmp_path / "f.ply", "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {ref.n_verts}\nproperty float x\nproperty float y\n"
                 f"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face {ref.n_tris}\n"
                 "property list uchar int vertex_indices\nend_header\n").encode())
        rec = np.zeros(ref.n_verts, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
        rec["p"], rec["c"] = ref.verts, ref.colors
        f.write(rec.tobytes())
        face = np.zeros(ref.n_tris, np.dtype([("n", "u1"), ("i", "<i4", 3)]))
        face["n"], face["i"] = 3, ref.tris
        f.write(face.tobytes())
    ply = load_mesh(tmp_path / "f.ply")
    np.testing.assert_array_equal(ply.colors, ref.colors)
    np.testing.assert_array_equal(pipe.renderer_3d.render_device(ply, poses).cpu().numpy(), images)
    pipe.renderer_3d.check()


def test_a_depth_only_pipeline_uploads_no_colours(tmp_path):
    from mvlm_amd import pipeline
    from mvlm_amd.utils.synthetic import write_face_like_obj

    obj = write_face_like_obj(tmp_path / "f.obj", grid=41, tex_size=64, seed=2, vertex_colors=True)
    sent = {}
    for mode in ("depth", "RGB"):
        pipe = pipeline.create_pipeline("bu3dfe", n_views=8, weights="synthetic:3", image_mode=mode, verbose=False)
        assert pipe._texture_needed() == (mode == "RGB")
        mesh = pipe.renderer_3d.load_mesh(obj, load_texture=pipe._texture_needed())
        assert mesh.colors is not None
        np.random.seed(1)
        lm, _ = pipe.predict_mesh_device(mesh, pipe.renderer_3d.generate_3d_transformations())
        assert np.isfinite(lm).all()
        (record,) = mesh._device.values()                               # (handle, owner, colours uploaded?)
        sent[mode] = record[2]
    assert sent == {"depth": False, "RGB": True}


def test_what_colours_do_to_the_landmarks():
    """The planted-peak detector end to end on the textured mesh and on the same mesh carrying its texture as per-vertex
    colours (no uvs, no texture): both take the inlier branch and stay as near the planted truth as
    test_landmarks_move_little_between_zero_and_four_samples asks of its runs; an uncoloured (white) mesh does not."""
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils import Mesh
    from test_planted_cpu import planted_scene

    mesh, pts, sd, poses = planted_scene(n_views=48)
    tex = mesh.texture
    th, tw = tex.shape[:2]
    tx = np.clip((mesh.uvs[:, 0] * tw).astype(np.int64), 0, tw - 1)
    ty = np.clip((mesh.uvs[:, 1] * th).astype(np.int64), 0, th - 1)
    coloured = Mesh(mesh.verts, mesh.tris, colors=np.ascontiguousarray(tex[th - 1 - ty, tx]))
    pipe = pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=48), weights=sd, verbose=False)
    lm, err = {}, {}
    for name, m in (("textured", mesh), ("coloured", coloured), ("white", Mesh(mesh.verts, mesh.tris))):
        np.random.seed(1)
        lm[name], err[name] = pipe.predict_mesh_device(m, poses)
    d = np.linalg.norm(lm["textured"] - lm["coloured"], axis=1)
    print(f"landmark movement textured -> coloured: median {np.median(d):.3f}, max {d.max():.3f} model units; RANSAC error "
          f"{err['textured']:.3f} / {err['coloured']:.3f} (white mesh: {err['white']:.3e})")
    for name in ("textured", "coloured"):
        assert err[name] < 10.0                                          # the inlier branch for every landmark
        assert np.median(np.linalg.norm(lm[name] - pts, axis=1)) < 4.0
    assert not np.array_equal(lm["white"], lm["coloured"])
