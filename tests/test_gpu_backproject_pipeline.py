"""-m gpu: the surface heat from the pipeline down - Pipeline(visualize_surface=True) in the fused path, through both PNG encoders,
with the heat sheet beside it, and through the CLI with --surface-mesh.  The written file, decoded, equals
HipRenderer3D.render_landmark_view(vertex_colors=surface_heat(...)["colors"]) of the heatmaps the predictor makes of the same views."""
import shutil
from pathlib import Path

import numpy as np
import pytest

import backproject_model as bm

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    from mvlm_amd.utils.synthetic import write_face_like_obj

    return write_face_like_obj(tmp_path_factory.mktemp("surface_scan") / "face.obj", grid=41, tex_size=64)


def _pipeline(**kw):
    from mvlm_amd import pipeline

    return pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, **kw)


def _decoded(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))


def _rebuilt(pipe, path, final, **kw):
    """This scan's picture made again: the same mesh and poses rendered, the predictor's heatmaps of those views laid on the mesh,
    the mesh drawn with those colours and the final landmarks ``final``; ``kw``: surface_heat's options."""
    from mvlm_amd.utils.render3d import view_rotations
    from mvlm_amd.utils.viewer import heat_colours

    r3 = pipe.renderer_3d
    mesh = r3.load_mesh(path, load_texture=pipe._texture_needed())
    poses = r3.generate_3d_transformations()
    images = r3.render_device(mesh, poses).clone()
    heat = pipe.predictor_2d.heatmaps_device(images)
    res = r3.surface_heat(mesh, images, heat, view_rotations(poses), colors=heat_colours(int(heat.shape[1])), return_scores=True, **kw)
    picture = r3.render_landmark_view(mesh, final, size=256, vertex_colors=res["colors"])[0]
    return mesh, images, heat, res, picture


@pytest.fixture(scope="module")
def plain(scan):
    """The run with the flag off: landmarks, error, and the surface heat's scratch, which must not exist."""
    pipe = _pipeline()
    pipe.renderer_3d.release_surface_heat()                              # (earlier tests of this process may have left some)
    np.random.seed(1)
    landmarks = pipe.predict_one_file(scan)
    return landmarks, pipe.last_error, pipe.renderer_3d.scratch_bytes("backproject")


def test_the_flag_changes_nothing_and_writes_the_picture(scan, plain, tmp_path, monkeypatch):
    from mvlm_amd.utils.render3d import view_rotations
    from mvlm_amd.utils.viewer import heat_colours

    monkeypatch.chdir(tmp_path)
    want_lm, want_err, scratch_off = plain
    assert scratch_off == 0 and not (tmp_path / "visualization").exists()   # off: nothing is allocated, nothing written
    files = {}
    for encoder in ("host", "device"):
        pipe = _pipeline(visualize_surface=True, visualize_size=256, view_png_encoder=encoder, visualize_name=encoder)
        assert not pipe._groupable(2) and pipe.last_surface_path is None and pipe.last_surface_heat is None
        assert pipe.surface_depth_tol == 2 and pipe._texture_needed()
        np.random.seed(1)
        got = pipe.predict_one_file(scan)
        np.testing.assert_array_equal(_bits(got), _bits(want_lm))           # landmarks and RANSAC error: bit for bit
        assert pipe.last_error == want_err and "visualize_surface" in pipe.timings
        assert pipe.last_surface_path == Path("visualization") / f"face_{encoder}_surface.png"
        files[encoder] = _decoded(tmp_path / pipe.last_surface_path)
    assert files["host"].shape == (256, 256, 3) and int((files["host"] != files["device"]).sum()) == 0
    assert pipe.renderer_3d.scratch_bytes("backproject") > 0
    mesh, images, heat, res, picture = _rebuilt(pipe, scan, got)
    assert tuple(heat.shape) == (8, 73, 256, 256)
    differing = int((files["device"] != picture).sum())
    print(f"pipeline surface heat: {differing} differing bytes of {picture.size}")
    assert differing == 0
    assert (picture != pipe.renderer_3d.render_landmark_view(mesh, got, size=256)[0]).any()   # the heat shows
    # what the pass left: one entry per landmark, the distance from the surface peak's vertex to the final landmark
    left = pipe.last_surface_heat
    assert sorted(left) == ["distance", "peak_score", "peak_vertex"] and all(len(left[k]) == 73 for k in left)
    np.testing.assert_array_equal(left["peak_vertex"], res["peak_vertex"].cpu().numpy())
    np.testing.assert_array_equal(left["peak_score"], res["peak_score"].cpu().numpy())
    found = left["peak_vertex"] >= 0
    assert found.any() and np.isnan(left["distance"][~found]).all()
    want = np.linalg.norm(np.asarray(got)[found] - mesh.verts.astype(np.float64)[left["peak_vertex"][found]], axis=1)
    np.testing.assert_array_equal(left["distance"][found], want)
    # and the kernels on the network's own heatmaps, against the model
    model = bm.surface_heat(mesh, view_rotations(pipe.renderer_3d.generate_3d_transformations()), images.cpu().numpy(), heat.cpu().numpy(),
                            colors=heat_colours(73))
    for key in ("n_visible", "scores", "colors", "peak_vertex", "peak_score"):
        np.testing.assert_array_equal(res[key].cpu().numpy(), model[key], err_msg=key)


def test_the_heat_sheet_beside_it_and_the_options(scan, plain, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pipe = _pipeline(visualize_surface=True, visualize_heat=True, visualize_size=256, heat_landmarks=[3, 17, 40], heat_floor=0.4,
                     surface_depth_tol=0)
    calls = []
    heatmaps = pipe.predictor_2d.heatmaps_device
    pipe.predictor_2d.heatmaps_device = lambda images: calls.append(1) or heatmaps(images)
    np.random.seed(1)
    got = pipe.predict_one_file(scan)
    np.testing.assert_array_equal(_bits(got), _bits(plain[0]))
    assert len(calls) == 1                                                  # one second pass for both pictures
    assert (tmp_path / "visualization" / "face_dtu3d_heat.png").is_file()
    del pipe.predictor_2d.heatmaps_device
    _, _, _, _, picture = _rebuilt(pipe, scan, got, landmarks=[3, 17, 40], floor=0.4, depth_tol=0)
    assert int((_decoded(tmp_path / "visualization" / "face_dtu3d_surface.png") != picture).sum()) == 0


def test_refusals(scan, tmp_path):
    from mvlm_amd import parallel
    from mvlm_amd.prediction import PrecomputedPredictor
    from mvlm_amd.utils.synthetic import face_like_mesh

    pipe = _pipeline(visualize_surface=True, visualize_size=256)
    pipe.predictor_2d = PrecomputedPredictor(20, fn=lambda images: (np.zeros((20, 8, 3), np.float32), np.ones(8, bool)))
    with pytest.raises(ValueError, match="visualize_surface needs a predictor with heatmaps_device"):
        pipe.predict_one_file(scan)
    with pytest.raises(ValueError, match=r"heat_landmarks must lie in 0\.\.72"):
        _pipeline(visualize_surface=True, visualize_size=256, heat_landmarks=[73]).predict_one_file(scan)
    pipe = _pipeline(visualize_surface=True, visualize_size=256, shard_views=True)
    orig = parallel.is_distributed
    parallel.is_distributed = lambda: True
    try:
        with pytest.raises(ValueError, match="visualize_surface is not supported with shard_views"):
            pipe.predict_one_file(scan)
    finally:
        parallel.is_distributed = orig
    face = face_like_mesh(grid=41, tex_size=64, seed=2)
    cloud = tmp_path / "cloud.obj"
    cloud.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in face.verts.astype(np.float64)) + "\n")
    with pytest.raises(ValueError, match="is a point cloud: visualize_surface is not supported"):
        _pipeline(visualize_surface=True, visualize_size=256).predict_one_file(cloud)


def test_cli_writes_the_picture_and_the_coloured_mesh(scan, tmp_path, monkeypatch):
    from mvlm_amd.__main__ import main
    from mvlm_amd.utils.mesh_io import load_mesh

    folder = tmp_path / "scans"
    folder.mkdir()
    for f in scan.parent.glob("face.*"):
        shutil.copy(f, folder / f"one{f.suffix}")
    monkeypatch.chdir(tmp_path)
    assert main(["-p", str(folder), "--pipelines", "dtu3d", "--weights", "synthetic:5", "--seed", "2", "--visualize-surface",
                 "--surface-mesh", "--surface-depth-tol", "3", "--visualize-size", "256", "--heat-floor", "0.3"]) == 0
    landmarks = np.loadtxt(folder / "one_dtu3d.txt", delimiter=",")
    assert _decoded(tmp_path / "visualization" / "one_dtu3d_surface.png").shape == (256, 256, 3)
    written = load_mesh(folder / "one_dtu3d_surface.obj")
    pipe = _pipeline(visualize_surface=True, visualize_size=256)            # (the 8 fixed poses draw nothing from the RNG)
    mesh, _, _, res, picture = _rebuilt(pipe, folder / "one.obj", landmarks, floor=0.3, depth_tol=3)
    assert written.n_verts == mesh.n_verts and written.n_tris == mesh.n_tris and written.uvs is None
    np.testing.assert_array_equal(written.colors, res["colors"].cpu().numpy()[:, :3])    # the same colour bytes
    assert len(np.unique(written.colors, axis=0)) > 10
    assert int((_decoded(tmp_path / "visualization" / "one_dtu3d_surface.png") != picture).sum()) == 0
