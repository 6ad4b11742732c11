"""-m gpu: the heat sheet from the pipeline down - Pipeline(visualize_heat=True) in the fused path, through both PNG encoders, with
a landmark selection, on a point cloud and through the CLI.  The written file, decoded, equals HipRenderer3D.render_heat_sheet of
the heatmaps the predictor makes of the same views, and tests/heat_model.py applied to them."""
import shutil
from pathlib import Path

import numpy as np
import pytest

import heat_model as hm

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    from mvlm_amd.utils.synthetic import write_face_like_obj

    return write_face_like_obj(tmp_path_factory.mktemp("heat_scan") / "face.obj", grid=41, tex_size=64)


def _pipeline(**kw):
    from mvlm_amd import pipeline

    return pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, **kw)


def _rebuilt(pipe, path):
    """This scan's views and their heatmaps, made again: render_device of the same mesh and poses, heatmaps_device on those images."""
    r3 = pipe.renderer_3d
    mesh = r3.load_mesh(path, load_texture=pipe._texture_needed())
    images = r3.render_device(mesh, r3.generate_3d_transformations()).clone()
    heat = pipe.predictor_2d.heatmaps_device(images)
    r3.check()
    return images, heat


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
    from mvlm_amd.utils.viewer import heat_colours

    monkeypatch.chdir(tmp_path)
    want_lm, want_err = plain
    assert not (tmp_path / "visualization").exists()                    # off: nothing is written
    pipe = _pipeline(visualize_heat=True)
    assert not pipe._groupable(2) and pipe.last_heat_path is None
    np.random.seed(1)
    got = pipe.predict_one_file(scan)
    np.testing.assert_array_equal(_bits(got), _bits(want_lm))           # landmarks and RANSAC error: bit for bit
    assert pipe.last_error == want_err
    png = tmp_path / "visualization" / "face_dtu3d_heat.png"
    assert png.is_file() and pipe.last_heat_path == Path("visualization") / "face_dtu3d_heat.png"
    assert "visualize_heat" in pipe.timings
    image = _decoded(png)
    assert image.shape == (3 * 256 + 4 * 2,) * 2 + (3,)
    images, heat = _rebuilt(pipe, scan)
    assert tuple(heat.shape) == (8, 73, 256, 256)
    kw = dict(colors=heat_colours(73), background="rgb", floor=0.25)
    want = pipe.renderer_3d.render_heat_sheet(images, heat, **kw)
    differing = int((image != want).sum())
    print(f"pipeline heat sheet: {differing} differing bytes of {want.size}")
    assert differing == 0
    model = hm.render(images.cpu().numpy(), heat.cpu().numpy(), **kw)
    print(f"against the model: {int((image != model).sum())} differing bytes")
    assert int((image != model).sum()) == 0
    assert (image != pipe.renderer_3d.render_view_sheet(images)).any()  # the heat shows
    # predict_files at batch_scans = 1 draws too; two scans with the flag set go one by one
    png.unlink()
    np.random.seed(1)
    (f, again), = list(pipe.predict_files([scan], batch_scans=2))
    np.testing.assert_array_equal(_bits(again), _bits(want_lm))
    np.testing.assert_array_equal(_decoded(png), want)


def test_the_device_encoder_writes_the_same_pixels_and_one_landmark_shows_only_its_colour(scan, plain, tmp_path, monkeypatch):
    from mvlm_amd.utils.viewer import heat_colours

    monkeypatch.chdir(tmp_path)
    k = 17
    files = {}
    for encoder in ("host", "device"):
        pipe = _pipeline(visualize_heat=True, heat_landmarks=[k], heat_floor=0.5, sheet_scale=2, view_png_encoder=encoder,
                         visualize_name=encoder)
        np.random.seed(1)
        got = pipe.predict_one_file(scan)
        np.testing.assert_array_equal(_bits(got), _bits(plain[0]))
        files[encoder] = _decoded(tmp_path / "visualization" / f"face_{encoder}_heat.png")
    assert files["host"].shape == (3 * 512 + 8, 3 * 512 + 8, 3)
    assert int((files["host"] != files["device"]).sum()) == 0
    images, heat = _rebuilt(pipe, scan)
    colours = heat_colours(73)
    want = pipe.renderer_3d.render_heat_sheet(images, heat, landmarks=[k], colors=colours, scale=2, floor=0.5)
    assert int((files["device"] != want).sum()) == 0
    # only landmark k's colour: the picture is the one drawn from that plane alone, and where it differs from the views alone it
    # has moved towards that colour in every channel
    alone = pipe.renderer_3d.render_heat_sheet(images, heat[:, k:k + 1].contiguous(), colors=colours[k:k + 1], scale=2, floor=0.5)
    assert int((want != alone).sum()) == 0
    views = pipe.renderer_3d.render_view_sheet(images, scale=2).astype(np.int32)
    changed = (want != views).any(axis=2)
    assert changed.any()
    before = np.abs(views[changed] - colours[k].astype(np.int32))
    after = np.abs(want[changed].astype(np.int32) - colours[k].astype(np.int32))
    assert (after <= before).all() and (after < before).any(axis=1).all()


def test_a_point_cloud_writes_a_heat_sheet(tmp_path, monkeypatch):
    from mvlm_amd.utils.synthetic import face_like_mesh
    from mvlm_amd.utils.viewer import heat_colours

    monkeypatch.chdir(tmp_path)
    face = face_like_mesh(grid=41, tex_size=64, seed=2)
    obj = tmp_path / "cloud.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in face.verts.astype(np.float64)) + "\n")
    pipe = _pipeline(visualize_heat=True)
    np.random.seed(1)
    got = pipe.predict_one_file(obj)
    assert got.shape == (73, 3)
    image = _decoded(tmp_path / "visualization" / "cloud_dtu3d_heat.png")
    images, heat = _rebuilt(pipe, obj)
    want = pipe.renderer_3d.render_heat_sheet(images, heat, colors=heat_colours(73))
    assert int((image != want).sum()) == 0


def test_refusals(scan, tmp_path):
    from mvlm_amd import parallel, pipeline
    from mvlm_amd.prediction import PrecomputedPredictor

    with pytest.raises(ValueError, match="largest scale that fits is 1"):
        pipeline.create_pipeline("dtu3d", n_views=96, weights="synthetic:5", verbose=False, visualize_heat=True, sheet_scale=2)
    pipe = _pipeline(visualize_heat=True)
    pipe.renderer_3d = object()
    with pytest.raises(ValueError, match="HipRenderer3D"):
        pipe.predict_one_file(tmp_path / "missing.obj")
    pipe = _pipeline(visualize_heat=True)
    pipe.predictor_2d = PrecomputedPredictor(20, fn=lambda images: (np.zeros((20, 8, 3), np.float32), np.ones(8, bool)))
    with pytest.raises(ValueError, match="heatmaps_device"):
        pipe.predict_one_file(scan)
    with pytest.raises(ValueError, match=r"heat_landmarks must lie in 0\.\.72"):
        _pipeline(visualize_heat=True, heat_landmarks=[73]).predict_one_file(scan)
    pipe = _pipeline(visualize_heat=True, shard_views=True)
    orig = parallel.is_distributed
    parallel.is_distributed = lambda: True
    try:
        with pytest.raises(ValueError, match="shard_views"):
            pipe.predict_one_file(scan)
    finally:
        parallel.is_distributed = orig


def test_cli_writes_the_heat_sheet(scan, tmp_path, monkeypatch):
    from mvlm_amd.__main__ import main

    folder = tmp_path / "scans"
    folder.mkdir()
    for f in scan.parent.glob("face.*"):
        shutil.copy(f, folder / f"one{f.suffix}")
    monkeypatch.chdir(tmp_path)
    assert main(["-p", str(folder), "--pipelines", "dtu3d", "--weights", "synthetic:5", "--seed", "2", "--visualize-heat",
                 "--heat-landmarks", "3,17,40", "--heat-floor", "0.3", "--sheet-scale", "2"]) == 0
    assert (folder / "one_dtu3d.txt").is_file()
    assert _decoded(tmp_path / "visualization" / "one_dtu3d_heat.png").shape == (3 * 512 + 8, 3 * 512 + 8, 3)
