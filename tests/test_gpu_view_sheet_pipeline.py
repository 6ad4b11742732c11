"""-m gpu: the view sheet from the pipeline down - Pipeline(visualize_sheet=True) in the fused path and the slot protocol, with
the report, with a depth-only model, on a point cloud, through both PNG encoders and the CLI.  The written file, decoded, equals
tests/sheet_model.py applied to inputs rebuilt for the fixed 8-pose table."""
import shutil
from pathlib import Path

import numpy as np
import pytest

import sheet_model as sm

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    from mvlm_amd.utils.synthetic import write_face_like_obj

    return write_face_like_obj(tmp_path_factory.mktemp("sheet_scan") / "face.obj", grid=41, tex_size=64)


def _pipeline(**kw):
    from mvlm_amd import pipeline

    return pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, **kw)


def _rebuilt(pipe, path, landmarks, **kw):
    """The model's sheet for this scan: render_device of the same mesh and poses, predict_device on those images, the landmarks."""
    from mvlm_amd.utils.render3d import view_rotations

    r3 = pipe.renderer_3d
    mesh = r3.load_mesh(path, load_texture=pipe._texture_needed())
    poses = r3.generate_3d_transformations()
    images = r3.render_device(mesh, poses)
    maxima = pipe.predictor_2d.predict_device(images)
    images, maxima = images.cpu().numpy(), maxima.cpu().numpy()
    r3.check()
    return sm.render(images, maxima, view_rotations(poses), landmarks, **kw)


def _decoded(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def plain(scan):
    """The run with the flag off: landmarks and error."""
    pipe = _pipeline()
    np.random.seed(1)
    return pipe.predict_one_file(scan), pipe.last_error


def test_the_flag_changes_nothing_and_writes_the_sheet(scan, plain, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    want_lm, want_err = plain
    assert not (tmp_path / "visualization").exists()                    # off: nothing is written
    pipe = _pipeline(visualize_sheet=True)
    assert not pipe._groupable(2)
    np.random.seed(1)
    got = pipe.predict_one_file(scan)
    np.testing.assert_array_equal(_bits(got), _bits(want_lm))
    assert pipe.last_error == want_err
    png = tmp_path / "visualization" / "face_dtu3d_views.png"
    assert png.is_file() and pipe.last_sheet_path == Path("visualization") / "face_dtu3d_views.png"
    image = _decoded(png)
    assert image.shape == (3 * 256 + 4 * 2,) * 2 + (3,)
    want = _rebuilt(pipe, scan, got)
    differing = int((image != want).sum())
    print(f"pipeline sheet: {differing} differing bytes of {want.size}")
    assert differing == 0
    assert (image == sm.BLUE).all(axis=2).sum() > 73 and (image == sm.RED).all(axis=2).any()
    # predict_files at batch_scans = 1 draws too; two scans with the flag set go one by one
    png.unlink()
    np.random.seed(1)
    (f, again), = list(pipe.predict_files([scan], batch_scans=2))
    np.testing.assert_array_equal(_bits(again), _bits(want_lm))
    np.testing.assert_array_equal(_decoded(png), want)


def test_the_device_encoder_writes_the_same_pixels(scan, plain, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pipe = _pipeline(visualize_sheet=True, sheet_scale=2, view_png_encoder="device", visualize_name="dev")
    np.random.seed(1)
    got = pipe.predict_one_file(scan)
    np.testing.assert_array_equal(_bits(got), _bits(plain[0]))
    image = _decoded(tmp_path / "visualization" / "face_dev_views.png")
    want = _rebuilt(pipe, scan, got, scale=2)
    assert image.shape == want.shape == (3 * 512 + 8, 3 * 512 + 8, 3)
    assert int((image != want).sum()) == 0


def test_with_the_report_rings_and_colours_follow_it(scan, tmp_path, monkeypatch):
    from mvlm_amd.utils.report import VIEW_KEPT

    monkeypatch.chdir(tmp_path)
    pipe = _pipeline(visualize_sheet=True, landmark_report=True)
    np.random.seed(1)
    got = pipe.predict_one_file(scan)
    rep = pipe.last_report
    used = ((rep.view_flags & VIEW_KEPT) != 0).astype(np.uint8)
    assert used.shape == (73, 8) and 0 < used.sum() < used.size          # the score filter drops some views: rings and discs
    want = _rebuilt(pipe, scan, got, colors=rep.branch_colours(), used=used)
    image = _decoded(tmp_path / "visualization" / "face_dtu3d_views.png")
    assert int((image != want).sum()) == 0
    assert (want != _rebuilt(pipe, scan, got)).any()                     # ... which the plain sheet does not show


def test_a_depth_only_model_gets_the_depth_background(scan, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    pipe = _pipeline(visualize_sheet=True, image_mode="depth")
    assert [int(c) for c in pipe.predictor_2d.chan_sel] == [3] and not pipe._texture_needed()
    np.random.seed(1)
    got = pipe.predict_one_file(scan)
    image = _decoded(tmp_path / "visualization" / "face_dtu3d_views.png")
    assert int((image != _rebuilt(pipe, scan, got, background="depth")).sum()) == 0
    plain_pixels = ~((image == sm.BLUE).all(axis=2) | (image == sm.RED).all(axis=2))
    assert (image[plain_pixels][:, 0] == image[plain_pixels][:, 1]).all()  # a grey


def test_the_slot_protocol_draws_from_numpy_arrays(scan, tmp_path, monkeypatch):
    from mvlm_amd.prediction import PrecomputedPredictor
    from mvlm_amd.utils.render3d import view_rotations

    monkeypatch.chdir(tmp_path)
    nl, n = 20, 8
    rs = np.random.RandomState(3)
    table = np.empty((nl, n, 3), np.float32)
    table[:, :, :2] = rs.uniform(60, 200, (nl, n, 2))
    table[:, :, 2] = rs.uniform(0.2, 0.9, (nl, n))
    pipe = _pipeline(visualize_sheet=True, visualize_name="slots")
    pipe.predictor_2d = PrecomputedPredictor(nl, fn=lambda images: (table, np.ones(n, bool)))
    assert not pipe._fusable()
    np.random.seed(2)
    got = pipe.predict_one_file(scan)
    images, poses, _ = pipe.renderer_3d.multiview_render(scan)
    want = sm.render(images, table, view_rotations(poses), got)
    assert int((_decoded(tmp_path / "visualization" / "face_slots_views.png") != want).sum()) == 0


def test_a_point_cloud_writes_a_sheet(tmp_path, monkeypatch):
    from mvlm_amd.utils.synthetic import face_like_mesh

    monkeypatch.chdir(tmp_path)
    face = face_like_mesh(grid=41, tex_size=64, seed=2)
    obj = tmp_path / "cloud.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in face.verts.astype(np.float64)) + "\n")
    pipe = _pipeline(visualize_sheet=True)
    np.random.seed(1)
    got = pipe.predict_one_file(obj)
    assert got.shape == (73, 3)
    image = _decoded(tmp_path / "visualization" / "cloud_dtu3d_views.png")
    assert int((image != _rebuilt(pipe, obj, got)).sum()) == 0


def test_refusals(scan, tmp_path):
    from mvlm_amd import parallel

    with pytest.raises(ValueError, match="largest scale that fits is 1"):
        from mvlm_amd import pipeline

        pipeline.create_pipeline("dtu3d", n_views=96, weights="synthetic:5", verbose=False, visualize_sheet=True, sheet_scale=2)
    pipe = _pipeline(visualize_sheet=True)
    pipe.renderer_3d = object()
    with pytest.raises(ValueError, match="HipRenderer3D"):
        pipe.predict_one_file(tmp_path / "missing.obj")
    pipe = _pipeline(visualize_sheet=True, shard_views=True)
    orig = parallel.is_distributed
    parallel.is_distributed = lambda: True
    try:
        with pytest.raises(ValueError, match="shard_views"):
            pipe.predict_one_file(scan)
    finally:
        parallel.is_distributed = orig


def test_cli_writes_the_sheet(scan, tmp_path, monkeypatch):
    from mvlm_amd.__main__ import main

    folder = tmp_path / "scans"
    folder.mkdir()
    for f in scan.parent.glob("face.*"):
        shutil.copy(f, folder / f"one{f.suffix}")
    monkeypatch.chdir(tmp_path)
    assert main(["-p", str(folder), "--pipelines", "dtu3d", "--weights", "synthetic:5", "--seed", "2", "--visualize-sheet",
                 "--sheet-scale", "2"]) == 0
    assert (folder / "one_dtu3d.txt").is_file()
    assert _decoded(tmp_path / "visualization" / "one_dtu3d_views.png").shape == (3 * 512 + 8, 3 * 512 + 8, 3)
