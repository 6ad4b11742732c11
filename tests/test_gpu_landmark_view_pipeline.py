"""-m gpu: the landmark view from the pipeline down - Pipeline(visualize_img=True), the CLI flag and LandmarkViewer."""
import shutil
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def planted_scan(tmp_path_factory):
    """The planted-peak scene of tests/planted.py at 8 views, written as an OBJ + JPEG pair."""
    from mvlm_amd.utils.mesh_io import write_obj
    from test_planted_cpu import planted_scene

    mesh, pts, sd, poses = planted_scene(n_views=8)
    path = tmp_path_factory.mktemp("planted_scan") / "scan.obj"
    write_obj(path, mesh.verts, mesh.tris, mesh.uvs, mesh.texture)
    return path, sd


def _planted_pipeline(sd, **kw):
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config

    return pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=8), weights=sd, verbose=False, **kw)


def test_the_flag_changes_nothing_and_writes_the_picture(planted_scan, tmp_path, monkeypatch):
    from PIL import Image

    path, sd = planted_scan
    monkeypatch.chdir(tmp_path)
    off = _planted_pipeline(sd)
    on = _planted_pipeline(sd, visualize_img=True, visualize_size=256, visualize_name="planted")
    np.random.seed(1)
    want = off.predict_one_file(path)
    assert not (tmp_path / "visualization").exists()             # off: nothing is written
    np.random.seed(1)
    got = on.predict_one_file(path)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert on.last_error == off.last_error
    png = tmp_path / "visualization" / "scan_planted.png"
    assert png.is_file() and on.last_view_path == Path("visualization") / "scan_planted.png"
    image = np.asarray(Image.open(png))
    assert image.shape == (256, 256, 3)
    mesh = on.renderer_3d.load_mesh(path)
    assert getattr(mesh, "to_original", None) is None          # (no pre-align here: the result is in the mesh's own space)
    ref, counts = on.renderer_3d.render_landmark_view(mesh, got, size=256, return_pixels=True)
    np.testing.assert_array_equal(image, ref[0])
    assert (counts > 0).sum() > len(got) // 2 and (image != 255).any()
    # predict_files at batch_scans = 1 draws too
    png.unlink()
    np.random.seed(1)
    (f, again), = list(on.predict_files([path], batch_scans=1))
    np.testing.assert_array_equal(_bits(again), _bits(want))
    np.testing.assert_array_equal(np.asarray(Image.open(png)), ref[0])


def test_the_report_colours_the_spheres_by_branch(planted_scan, tmp_path, monkeypatch):
    from PIL import Image

    from mvlm_amd.utils.report import BRANCH_COLOURS

    path, sd = planted_scan
    monkeypatch.chdir(tmp_path)
    pipe = _planted_pipeline(sd, visualize_img=True, visualize_size=256, visualize_name="planted", landmark_report=True)
    np.random.seed(1)
    got = pipe.predict_one_file(path)
    rep = pipe.last_report
    assert BRANCH_COLOURS == {1: (0, 0, 255), 2: (255, 165, 0), 0: (255, 0, 0)}
    colours = rep.branch_colours()
    assert colours.shape == (len(got), 3) and all(tuple(c) == BRANCH_COLOURS[int(b)] for c, b in zip(colours, rep.branch))
    mesh = pipe.renderer_3d.load_mesh(path)
    ref = pipe.renderer_3d.render_landmark_view(mesh, got, size=256, colors=colours)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "visualization" / "scan_planted.png")), ref[0])


def test_the_slot_path_colours_every_scan_by_its_own_report(tmp_path, monkeypatch):
    """Two different scans through the slot protocol (a host predictor between HipRenderer3D and HipEstimator3D) with both flags
    on: each picture carries the branch colours of ITS scan's report.  The predictor gives scan 1's landmarks 0..9 and scan 2's
    landmarks 10..19 views above the median, so the two reports' branches differ."""
    from PIL import Image

    from mvlm_amd import pipeline
    from mvlm_amd.prediction import PrecomputedPredictor
    from mvlm_amd.utils.synthetic import write_face_like_obj

    monkeypatch.chdir(tmp_path)
    nl, n = 20, 12
    rs = np.random.RandomState(3)
    tables = []
    for rows in (slice(0, 10), slice(10, 20)):
        lms = np.empty((nl, n, 3), np.float32)
        lms[:, :, :2] = rs.uniform(60, 200, (nl, n, 2))
        lms[:, :, 2] = 0.25
        lms[rows, :5, 2] = 0.75
        tables.append(lms)
    calls = []

    def fn(images):
        calls.append(len(calls))
        return tables[len(calls) - 1], np.ones(n, bool)

    pipe = pipeline.create_pipeline("dtu3d", n_views=n, weights="synthetic:1", verbose=False, landmark_report=True,
                                    visualize_img=True, visualize_size=128, visualize_name="slots")
    pipe.predictor_2d = PrecomputedPredictor(nl, fn=fn)
    assert not pipe._fusable()
    branches = []
    for k, seed in enumerate((3, 4)):
        path = write_face_like_obj(tmp_path / f"scan{k}.obj", grid=40, tex_size=64, seed=seed)
        np.random.seed(2)
        got = pipe.predict_one_file(path)
        rep = pipe.last_report
        branches.append(rep.branch.copy())
        mesh = pipe.renderer_3d.load_mesh(path)
        finite = np.isfinite(got).all(axis=1)
        ref = pipe.renderer_3d.render_landmark_view(mesh, got[finite], size=128, colors=rep.branch_colours()[finite])
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "visualization" / f"scan{k}_slots.png")), ref[0], err_msg=str(k))
    assert len(calls) == 2 and not np.array_equal(branches[0], branches[1])
    assert (branches[0][10:] == 0).all() and (branches[0][:10] != 0).all() and (branches[1][:10] == 0).all()


def test_a_renderer_that_cannot_draw_is_refused_before_the_prediction(tmp_path):
    from mvlm_amd import pipeline

    pipe = pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:1", verbose=False, visualize_img=True, visualize_size=64)
    pipe.renderer_3d = object()
    with pytest.raises(ValueError, match="HipRenderer3D"):
        pipe.predict_one_file(tmp_path / "missing.obj")


def test_with_a_pre_align_block_the_points_sit_on_the_drawn_surface(planted_scan, tmp_path, monkeypatch):
    """The planted detector with BU_3DFE-depth's pre-align block (configs[0]: centre of mass, scale 20) on a copy of the scan
    that is 20 times smaller and off the origin: the picture is drawn in the space the mesh was uploaded in, with the landmarks
    before the inverse mapping - every one shows in a front, left or right view at frame="fit"."""
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils.mesh_io import load_obj, write_obj
    from mvlm_amd.utils.prealign import landmarks_to_original_space
    from mvlm_amd.utils.synthetic import unaligned_copy

    path, sd = planted_scan
    monkeypatch.chdir(tmp_path)
    cfg = config.default_config("DTU3D", "RGB", n_views=8)
    cfg["pre-align"] = dict(config.default_config("BU_3DFE-depth")["pre-align"], write_pre_aligned=False)
    raw = unaligned_copy(load_obj(path, decode="host"), cfg["pre-align"])
    small = tmp_path / "small.obj"
    write_obj(small, raw.verts, raw.tris, raw.uvs, raw.texture)
    pipe = pipeline_from_config(cfg, weights=sd, verbose=False, visualize_img=True, visualize_size=256, visualize_name="planted")
    seen = {}
    draw = pipe._draw_landmark_view
    monkeypatch.setattr(pipe, "_draw_landmark_view", lambda mesh, lm, *a: (seen.update(mesh=mesh, lm=np.array(lm)), draw(mesh, lm, *a))[1])
    np.random.seed(4)
    got = pipe.predict_one_file(small)
    assert (tmp_path / "visualization" / "small_planted.png").is_file()
    mesh, lm = seen["mesh"], seen["lm"]
    assert mesh.to_original is not None
    np.testing.assert_array_equal(landmarks_to_original_space(lm, mesh.to_original), got)   # drawn: before the inverse mapping
    assert np.abs(lm - got).max() > 1.0
    poses = [[0, 0, 0], [0, -60, 0], [0, 60, 0]]
    _, counts = pipe.renderer_3d.render_landmark_view(mesh, lm, poses=poses, size=256, frame="fit", return_pixels=True)
    print("pixels per landmark, best of front / left / right:", counts.max(axis=0).tolist())
    assert (counts.max(axis=0) > 0).all(), np.nonzero(counts.max(axis=0) == 0)


def test_cli_writes_the_picture(planted_scan, tmp_path, monkeypatch):
    from PIL import Image

    from mvlm_amd.__main__ import main

    path, _ = planted_scan
    folder = tmp_path / "scans"
    folder.mkdir()
    for f in path.parent.glob("scan.*"):
        shutil.copy(f, folder / f"one{f.suffix}")
    monkeypatch.chdir(tmp_path)
    assert main(["-p", str(folder), "--pipelines", "dtu3d", "--weights", "synthetic:3", "--seed", "2", "--visualize-img",
                 "--visualize-size", "256"]) == 0
    assert (folder / "one_dtu3d.txt").is_file()
    assert np.asarray(Image.open(tmp_path / "visualization" / "one_dtu3d.png")).shape == (256, 256, 3)


def test_landmark_viewer(planted_scan, tmp_path, monkeypatch):
    from PIL import Image

    from mvlm_amd.utils import HipRenderer3D, LandmarkViewer
    from mvlm_amd.utils.mesh_io import load_mesh

    path, _ = planted_scan
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="interactive"):
        LandmarkViewer(path, save=False)
    assert not (tmp_path / "visualization").exists()
    mesh = load_mesh(path)
    lm = np.asarray(mesh.verts, np.float64)[::997]
    v = LandmarkViewer(path, lm, pname="demo", size=128)
    ref = HipRenderer3D(n_views=1, verbose=False).render_landmark_view(mesh, lm, size=128)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "visualization" / "scan_demo.png")), ref[0])
    LandmarkViewer(path, None, size=64)
    assert np.asarray(Image.open(tmp_path / "visualization" / "scan.png")).shape == (64, 64, 3)
    with pytest.raises(ValueError):
        HipRenderer3D(n_views=1, verbose=False).render_landmark_view(mesh, lm, size=250)
    # radius: 0.008 x the landmarks' diagonal; one landmark: 0.008 x the mesh's diagonal
    r = HipRenderer3D(n_views=1, verbose=False)
    assert r.landmark_view_arguments(mesh, lm)[3] == pytest.approx(0.008 * np.linalg.norm(lm.max(0) - lm.min(0)))
    v = np.asarray(mesh.verts, np.float64)
    assert r.landmark_view_arguments(mesh, lm[:1])[3] == pytest.approx(0.008 * np.linalg.norm(v.max(0) - v.min(0)))
    assert r.landmark_view_arguments(mesh, None)[3] == 0.0
