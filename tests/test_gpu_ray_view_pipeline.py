"""-m gpu: the ray view from the pipeline down - Pipeline(visualize_rays_img=True), the CLI flag and RayVisualizer."""
import shutil
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSES = ((0, 0, 0), (0, 60, 0), (0, -60, 0))


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    from mvlm_amd.utils.synthetic import write_face_like_obj

    return write_face_like_obj(tmp_path_factory.mktemp("ray_scan") / "scan.obj", grid=40, tex_size=64, seed=3)


def _pipeline(**kw):
    from mvlm_amd import pipeline

    return pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:3", verbose=False, **kw)


def _spy(pipe, monkeypatch):
    """what the pipeline hands to HipRenderer3D.render_ray_view, recorded on the way through"""
    seen = {}
    draw = pipe.renderer_3d.render_ray_view

    def wrapper(mesh, landmarks, starts, ends, **kw):
        seen.update(landmarks=np.array(landmarks), starts=starts, ends=ends, **kw)
        return draw(mesh, landmarks, starts, ends, **kw)

    monkeypatch.setattr(pipe.renderer_3d, "render_ray_view", wrapper)
    return seen


def _pngs(folder, stem="scan", name="rays"):
    from PIL import Image

    return [np.asarray(Image.open(Path(folder) / f"{stem}_{name}_rays_{i}.png")) for i in range(len(POSES))]


def test_the_flag_changes_nothing_and_writes_a_picture_per_pose(scan, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    shots = tmp_path / "shots"
    off = _pipeline()
    on = _pipeline(visualize_rays_img=True, visualize_size=256, visualize_name="rays", screenshot_folder=shots)
    np.random.seed(1)
    want = off.predict_one_file(scan)
    assert not shots.exists() and not (tmp_path / "visualization").exists()   # off: nothing is written
    args = _spy(on, monkeypatch)
    np.random.seed(1)
    got = on.predict_one_file(scan)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert on.last_error == off.last_error
    assert on.last_ray_view_paths == [shots / f"scan_rays_rays_{i}.png" for i in range(3)]
    assert sorted(p.name for p in shots.iterdir()) == [f"scan_rays_rays_{i}.png" for i in range(3)]   # and no .npz
    images = _pngs(shots)
    assert on._ray_view is None                                                # nothing is kept behind the picture
    assert tuple(args["starts"].shape) == (len(got), 8, 3) and args["starts"].is_cuda
    mesh = on.renderer_3d.load_mesh(scan)
    ref, counts, ray_counts = on.renderer_3d.render_ray_view(mesh, got, args["starts"], args["ends"], poses=POSES, size=256,
                                                             return_pixels=True)
    for i in range(3):
        np.testing.assert_array_equal(images[i], ref[i])
    assert ray_counts.shape == (3, len(got) * 8) and (ray_counts > 0).any() and (counts > 0).any()
    plain = on.renderer_3d.render_landmark_view(mesh, got, poses=POSES, size=256)
    assert (plain != ref).any()                                                # the rays show
    # default folder, and predict_files at batch_scans = 1 draws too
    on.screenshot_folder = None
    np.random.seed(1)
    (f, again), = list(on.predict_files([scan], batch_scans=1))
    np.testing.assert_array_equal(_bits(again), _bits(want))
    for i, image in enumerate(_pngs(tmp_path / "visualization" / "ray_screenshots")):
        np.testing.assert_array_equal(image, ref[i])
    assert not on._groupable(2)
    # predict_mesh_device on its own has no file name: it draws nothing and leaves nothing behind
    before = sorted(p.name for p in (tmp_path / "visualization" / "ray_screenshots").iterdir())
    np.random.seed(1)
    on.predict_mesh_device(mesh, on.renderer_3d.generate_3d_transformations())
    assert on._ray_view is None and sorted(p.name for p in (tmp_path / "visualization" / "ray_screenshots").iterdir()) == before


def test_the_selection_draws_the_rays_the_dump_holds(scan, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    shots = tmp_path / "shots"
    pipe = _pipeline(visualize_rays_img=True, visualize_rays=True, visualize_size=256, visualize_name="rays", screenshot_folder=shots)
    np.random.seed(1)
    got = pipe.predict_one_file(scan, landmark_indices=[0, 5, -1], view_indices=[1, 2])
    dump = np.load(shots / "scan_rays.npz")
    assert dump["starts"].shape == (3, 2, 3) and bool(dump["clipped"])
    mesh = pipe.renderer_3d.load_mesh(scan)
    ref, _, ray_counts = pipe.renderer_3d.render_ray_view(mesh, got, dump["starts"], dump["ends"], poses=POSES, size=256,
                                                          return_pixels=True)
    assert ray_counts.shape == (3, 6) and (ray_counts > 0).any()                # six rays
    for i, image in enumerate(_pngs(shots)):
        np.testing.assert_array_equal(image, ref[i])
    # unclipped on request
    np.random.seed(1)
    pipe.predict_one_file(scan, landmark_indices=[0, 5, -1], view_indices=[1, 2], clip_rays_to_mesh=False)
    dump = np.load(shots / "scan_rays.npz")
    assert not bool(dump["clipped"])
    ref2 = pipe.renderer_3d.render_ray_view(mesh, got, dump["starts"], dump["ends"], poses=POSES, size=256)
    for i, image in enumerate(_pngs(shots)):
        np.testing.assert_array_equal(image, ref2[i])
    assert (ref2 != ref).any() or not np.load(shots / "scan_rays.npz")["hit"].any() and not dump["hit"].any()


def test_the_report_colours_the_rays(scan, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    shots = tmp_path / "shots"
    pipe = _pipeline(visualize_rays_img=True, visualize_size=256, visualize_name="rays", screenshot_folder=shots, landmark_report=True)
    args = _spy(pipe, monkeypatch)
    np.random.seed(1)
    got = pipe.predict_one_file(scan, view_indices=[0, 3, 7])
    rep = pipe.last_report
    want = rep.ray_colours(np.asarray(rep.view_indices)[[0, 3, 7]]).reshape(-1, 3)
    np.testing.assert_array_equal(args["ray_colors"], want)
    np.testing.assert_array_equal(args["colors"], rep.branch_colours())
    kinds = {tuple(c) for c in rep.ray_colours().reshape(-1, 3)}
    assert (26, 230, 26) in kinds and (160, 160, 160) in kinds                  # used and filtered rays both occur in this scan
    mesh = pipe.renderer_3d.load_mesh(scan)
    ref = pipe.renderer_3d.render_ray_view(mesh, got, args["starts"], args["ends"], poses=POSES, size=256, colors=rep.branch_colours(),
                                           ray_colors=want)
    for i, image in enumerate(_pngs(shots)):
        np.testing.assert_array_equal(image, ref[i])


def test_visualize_rays_alone_still_writes_only_the_dump(scan, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pipe = _pipeline(visualize_rays=True)
    np.random.seed(1)
    pipe.predict_one_file(scan)
    folder = tmp_path / "visualization" / "ray_screenshots"
    assert [p.name for p in folder.iterdir()] == ["scan_rays.npz"]
    assert pipe.last_ray_view_paths == []


def test_a_renderer_that_cannot_draw_is_refused_before_the_prediction(tmp_path):
    pipe = _pipeline(visualize_rays_img=True, visualize_size=64)
    pipe.renderer_3d = object()
    with pytest.raises(ValueError, match="visualize_rays_img needs a HipRenderer3D"):
        pipe.predict_one_file(tmp_path / "missing.obj")
    with pytest.raises(ValueError, match="visualize_size"):
        _pipeline(visualize_rays_img=True, visualize_size=100)


def test_the_slot_path_draws_too(scan, tmp_path, monkeypatch):
    from mvlm_amd.prediction import PrecomputedPredictor

    monkeypatch.chdir(tmp_path)
    nl, n = 20, 8
    rs = np.random.RandomState(3)
    lms = np.empty((nl, n, 3), np.float32)
    lms[:, :, :2] = rs.uniform(90, 170, (nl, n, 2))
    lms[:, :, 2] = rs.uniform(0.2, 0.9, (nl, n))
    pipe = _pipeline(visualize_rays_img=True, visualize_size=128, visualize_name="slots", landmark_report=True)
    pipe.predictor_2d = PrecomputedPredictor(nl, fn=lambda images: (lms, np.ones(n, bool)))
    assert not pipe._fusable()
    args = _spy(pipe, monkeypatch)
    np.random.seed(2)
    got = pipe.predict_one_file(scan)
    rep = pipe.last_report
    np.testing.assert_array_equal(args["ray_colors"], rep.ray_colours().reshape(-1, 3))
    assert tuple(args["starts"].shape) == (nl, n, 3)
    images = _pngs(tmp_path / "visualization" / "ray_screenshots", name="slots")
    assert images[0].shape == (128, 128, 3) and all((im != 255).any() for im in images)


def test_cli_writes_the_pictures(scan, tmp_path, monkeypatch):
    from PIL import Image

    from mvlm_amd.__main__ import main

    folder = tmp_path / "scans"
    folder.mkdir()
    for f in scan.parent.glob("scan.*"):
        shutil.copy(f, folder / f"one{f.suffix}")
    monkeypatch.chdir(tmp_path)
    assert main(["-p", str(folder), "--pipelines", "dtu3d", "--weights", "synthetic:3", "--seed", "2", "--visualize-rays",
                 "--visualize-size", "256"]) == 0
    assert (folder / "one_dtu3d.txt").is_file()
    for i in range(3):
        assert np.asarray(Image.open(tmp_path / "visualization" / "ray_screenshots" / f"one_dtu3d_rays_{i}.png")).shape == (256, 256, 3)
    assert not (tmp_path / "visualization" / "one_dtu3d.png").exists()


def test_ray_visualizer(scan, tmp_path, monkeypatch):
    from mvlm_amd.utils import HipEstimator3D, HipRenderer3D, RayVisualizer, RayVisualizerConfig
    from mvlm_amd.utils.mesh_io import load_mesh
    from oracle.estimator import estimate_landmark_lines

    monkeypatch.chdir(tmp_path)
    mesh = load_mesh(scan)
    rs = np.random.RandomState(4)
    poses = rs.uniform(-30.0, 30.0, (4, 3))
    stack = np.concatenate([rs.uniform(100.0, 156.0, (5, 4, 2)), np.ones((5, 4, 1))], axis=2).astype(np.float32)
    starts, ends = estimate_landmark_lines(256, stack, poses)
    lm = np.asarray(mesh.verts, np.float64)[::300][:5]
    assert len(lm) == 5
    cfg = RayVisualizerConfig(size=128, ray_color=(1.0, 0.0, 0.0), landmark_radius=2.0, ray_radius=0.8, poses=((0, 0, 0), (0, 45, 0)))
    paths = RayVisualizer(cfg).show(mesh, starts, ends, landmarks=lm, landmark_indices=[1, -1], view_indices=[0, 2, 3])
    assert paths == [Path("visualization") / "ray_screenshots" / f"scan_rays_{i}.png" for i in range(2)]
    clipped, hit = HipEstimator3D(verbose=False).clip_rays_to_mesh(mesh, starts[np.ix_([1, 4], [0, 2, 3])], ends[np.ix_([1, 4], [0, 2, 3])])
    assert hit.any()
    ref = HipRenderer3D(n_views=1, verbose=False).render_ray_view(
        mesh, lm, starts[np.ix_([1, 4], [0, 2, 3])], clipped, poses=cfg.poses, size=128, radius=2.0, ray_radius=0.8,
        colors=np.tile(np.array([[26, 26, 230]], np.uint8), (5, 1)), ray_colors=np.tile(np.array([[255, 0, 0]], np.uint8), (6, 1)))
    from PIL import Image

    for i, p in enumerate(paths):
        np.testing.assert_array_equal(np.asarray(Image.open(p)), ref[i])
    with pytest.raises(TypeError):
        RayVisualizer().show(object(), starts, ends)
