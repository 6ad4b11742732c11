"""-m gpu: 4-sample multisampled rendering (mvlm_set_render_multisamples, HipRenderer3D(multisamples=4)) against its CPU model
(tests/native/msaa_raster.c, tests/msaa_model.py), through every layer that sets it, and without disturbing the default."""
import ctypes as C

import numpy as np
import pytest

import msaa_model
from gl_contract import load

pytestmark = pytest.mark.gpu

META, SCENES = load()


@pytest.fixture(scope="session")
def model(tmp_path_factory):
    msaa_model.load(tmp_path_factory.mktemp("msaa_model"))
    return msaa_model.render


def _mesh(sc):
    from mvlm_amd.utils import Mesh

    return Mesh(sc["verts"], sc["tris"], sc["uvs"], sc["tex"])


def _hip(mesh, poses, bits=8, samples=4):
    from mvlm_amd.utils import HipRenderer3D

    r = HipRenderer3D(n_views=len(poses), verbose=False, subpixel_bits=bits, multisamples=samples)
    out = r.render_device(mesh, poses).cpu().numpy()
    r.check()
    return out


@pytest.mark.parametrize("bits", [4, 5, 6, 7, 8])
def test_four_samples_equal_the_model(model, bits):
    for name in ("face40", "face224", "coarse", "offscreen"):
        sc = SCENES[name]
        want = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=bits, samples=4)
        got = _hip(_mesh(sc), sc["poses"], bits)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} at {bits} bits")


def test_four_samples_on_the_bench_mesh_at_96_views(model):
    """the bench's 224-grid face (99 458 triangles, mostly sub-pixel) at 96 random views, texture and geometry shading"""
    from mvlm_amd.utils import HipRenderer3D
    from mvlm_amd.utils.synthetic import face_like_mesh

    mesh = face_like_mesh(224, 256, seed=0)
    r = HipRenderer3D(n_views=96, verbose=False, multisamples=4)
    np.random.seed(0)
    poses = r.generate_3d_transformations()
    got = {}
    for shading in ("texture", "geometry"):
        r.shading = shading
        got[shading] = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        want = model(mesh.verts, mesh.tris, mesh.uvs, mesh.texture, poses, shading=shading, samples=4)
        np.testing.assert_array_equal(got[shading], want, err_msg=shading)
    one = model(mesh.verts, mesh.tris, mesh.uvs, mesh.texture, poses, samples=1)
    covered = one[..., 3] != 1.0 / 255.0
    frac = float((got["texture"] != one)[..., :3].any(-1).sum() / covered.sum())
    print(f"covered pixels whose colour changes with 4 samples: {100 * frac:.1f} %")
    assert 0.01 < frac < 0.5   # multisampling does change the views


def test_switching_modes_on_one_context_keeps_both_key_planes_clean(model):
    """0 -> 4 -> 0 -> 4 samples with one renderer, and a 0-sample and a 4-sample renderer alternating on one GPU (they share
    the context): every render equals its own reference, so neither key plane carries anything over."""
    from mvlm_amd.utils import HipRenderer3D
    from mvlm_amd.utils.synthetic import face_like_mesh
    from oracle import raster

    mesh = face_like_mesh(60, 64, seed=4)
    rs = np.random.RandomState(7)
    poses = np.stack([rs.randint(-40, 40, 16), rs.randint(-80, 80, 16), rs.randint(-20, 20, 16)], 1).astype(np.float64)
    want = {0: raster.multiview_render(mesh.verts, mesh.tris, mesh.uvs, mesh.texture, poses),
            4: model(mesh.verts, mesh.tris, mesh.uvs, mesh.texture, poses, samples=4)}
    assert not np.array_equal(want[0], want[4])
    r = HipRenderer3D(n_views=16, verbose=False)
    for samples in (0, 4, 0, 4):
        r.multisamples = samples
        got = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        np.testing.assert_array_equal(got, want[samples], err_msg=f"{samples} samples")
    plain, ms = HipRenderer3D(n_views=16, verbose=False), HipRenderer3D(n_views=16, verbose=False, multisamples=4)
    assert plain.ctx is ms.ctx
    for r in (ms, plain, ms, plain):
        got = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        np.testing.assert_array_equal(got, want[r.multisamples])


def test_overflow_at_four_samples_is_reported_and_the_next_render_is_clean(model):
    """the overflow scene of test_render_overflow_is_reported_and_the_next_render_is_clean, multisampled"""
    from mvlm_amd import _lib
    from mvlm_amd.utils import HipRenderer3D, Mesh
    from mvlm_amd.utils.synthetic import face_like_mesh

    n = 100
    rs = np.random.RandomState(2)
    verts = np.concatenate([np.array([[-400, -400, z], [400, -400, z], [0, 600, z]], np.float32) for z in rs.uniform(-50, 50, n)])
    huge = Mesh(verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3))
    r = HipRenderer3D(n_views=8, verbose=False, multisamples=4)
    poses = r.generate_3d_transformations()
    r.render_device(huge, poses)
    with pytest.raises(_lib.MvlmHipError, match="overflowed"):
        r.check()
    face = face_like_mesh(40, 64, seed=1)
    got = r.render_device(face, poses).cpu().numpy()
    r.check()
    np.testing.assert_array_equal(got, model(face.verts, face.tris, face.uvs, face.texture, poses, samples=4))


def test_other_sample_counts_are_rejected():
    from mvlm_amd import _lib
    from mvlm_amd.utils import HipRenderer3D

    for bad in (2, 8, -1, 1):
        with pytest.raises(ValueError):
            HipRenderer3D(n_views=8, verbose=False, multisamples=bad)
    r = HipRenderer3D(n_views=8, verbose=False)
    with pytest.raises(ValueError):
        r.multisamples = 8
    ctx = _lib.get_context(0)
    for bad in (2, 8, -1):
        assert ctx.lib.mvlm_set_render_multisamples(ctx.handle, bad) != 0
        assert b"multisamples" in ctx.lib.mvlm_last_error(ctx.handle)
    for ok in (4, 0):
        assert ctx.lib.mvlm_set_render_multisamples(ctx.handle, ok) == 0
    ctx._render_mode = None   # (the renderers push their mode again)


def test_landmarks_move_little_between_zero_and_four_samples():
    """What multisampling does to the RESULT: the planted-peak detector end to end with 0 and with 4 samples, through
    Pipeline(render_multisamples=...).  At 0 samples every landmark takes the inlier branch; at 4 the blended silhouettes move
    some planted maxima far enough for a few landmarks to fall back (each adds 1e8 / NL to the error), the others stay as near
    the planted truth as at 0."""
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config
    from test_planted_cpu import planted_scene

    mesh, pts, sd, poses = planted_scene(n_views=48)
    pipe = pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=48), weights=sd, verbose=False,
                                render_multisamples=4)
    assert pipe.renderer_3d.multisamples == 4
    lm, err = {}, {}
    for samples in (0, 4):
        pipe.renderer_3d.multisamples = samples
        np.random.seed(1)
        lm[samples], err[samples] = pipe.predict_mesh_device(mesh, poses)
    d = np.linalg.norm(lm[0] - lm[4], axis=1)
    fell_back = int(round(err[4] * 73 / 1e8))
    print(f"landmark movement 0 -> 4 samples: median {np.median(d):.3f}, max {d.max():.3f} model units; RANSAC error "
          f"{err[0]:.3f} / {err[4]:.3f} (~{fell_back} of 73 landmarks fell back at 4 samples)")
    assert err[0] < 10.0                         # inlier branch for every landmark at 0 samples
    assert fell_back <= 12
    assert d.max() > 0.0 and np.median(d) < 1.0, (float(np.median(d)), float(d.max()))
    for samples in (0, 4):
        assert np.median(np.linalg.norm(lm[samples] - pts, axis=1)) < 4.0


def test_the_slot_protocol_and_the_fused_path_render_multisampled(tmp_path, model):
    """multiview_render (slot protocol) and the fused predict_mesh_device both go through render_device: 4-sample views"""
    from mvlm_amd import pipeline
    from mvlm_amd.utils.mesh_io import load_obj
    from mvlm_amd.utils.synthetic import write_face_like_obj

    obj = write_face_like_obj(tmp_path / "f.obj", grid=41, tex_size=64, seed=2)
    pipe = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False, render_multisamples=4)
    np.random.seed(3)
    images, poses, mesh = pipe.renderer_3d.multiview_render(obj)
    ref = load_obj(obj)
    np.testing.assert_array_equal(images, model(ref.verts, ref.tris, ref.uvs, ref.texture, poses, samples=4))
    np.random.seed(3)
    fused, _ = pipe.predict_mesh_device(mesh, poses)
    np.random.seed(3)
    lms, _ = pipe.predictor_2d.predict_landmarks_from_images(images)
    starts, ends = pipe.estimator_3d.estimate_landmark_lines(images, lms, poses)
    raw, _ = pipe.estimator_3d.estimate_landmarks_from_lines(lms, starts, ends)
    np.testing.assert_array_equal(fused, pipe.estimator_3d.project_landmarks_to_surface(mesh, raw))


def test_cli_with_four_samples_writes_landmark_files(tmp_path):
    from mvlm_amd.__main__ import main
    from mvlm_amd.utils.synthetic import write_face_like_obj

    write_face_like_obj(tmp_path / "a.obj", grid=30, tex_size=32, seed=1)
    out = tmp_path / "out"
    assert main(["-p", str(tmp_path), "-o", str(out), "-n", "8", "--weights", "synthetic:1", "--pipelines", "dtu3d",
                 "--multisamples", "4", "--seed", "2"]) == 0
    lm4 = np.loadtxt(out / "a_dtu3d.txt", delimiter=",")
    assert lm4.shape == (73, 3) and np.isfinite(lm4).all()
    with pytest.raises(SystemExit):
        main(["-p", str(tmp_path), "--multisamples", "2"])


@pytest.mark.parametrize("name", ["face40", "face224", "coarse", "centres", "uv_wrap", "offscreen", "ms_positions_lo",
                                  "ms_positions_hi", "ms_resolve", "ms_centre"])
def test_hip_against_opengl_with_four_samples(model, name):
    """at the GL's own sub-pixel precision: 0 unexplained pixels within the bounds the model meets (the model's per-sample
    winners classify the differences; the HIP image is the model's bit for bit)"""
    import msaa_contract
    from test_gl_msaa_contract import MEASURED, SCENES as MS

    sc = MS[name] if "verts" in MS[name] else SCENES[name]
    got = _hip(_mesh(sc), sc["poses"], bits=4)
    want, win_tri, win_rgb = model(sc["verts"], sc["tris"], sc["uvs"], sc["tex"], sc["poses"], subpixel_bits=4, samples=4,
                                   per_sample=True)
    np.testing.assert_array_equal(got, want)
    r = msaa_contract.compare(sc, got, win_tri, win_rgb, MS[name]["rgb"])
    print(name, r)
    clip, texel = MEASURED[name]
    assert r["unexplained"] == 0 and r["clip"] <= clip and r["texel"] <= texel, r
