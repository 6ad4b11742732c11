"""-m gpu: point_surface="mesh" through the pipeline - a coloured face-like cloud, written as a `v x y z r g b` file, gets its
triangles on the device and then everything a mesh has, all options at once; and what comes out is, byte for byte, what
predict_mesh_device gives for the Mesh built by hand from the same points, the model's triangles (tests/cloud_mesh_model.py, fed the
device's table and normals) and the same colours - through predict_one_file, predict_files and the command line."""
import numpy as np
import pytest

import cloud_mesh_model as cm
from test_gpu_cloud_mesh import _cloud, _prepare

pytestmark = pytest.mark.gpu

EVERYTHING = dict(landmark_report=True, visualize_img=True, visualize_rays_img=True, visualize_sheet=True, visualize_surface=True,
                  render_multisamples=4)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """(the cloud's file, its Mesh as the loader reads it)"""
    from mvlm_amd.utils.mesh_io import load_obj
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=41, tex_size=64, seed=2, vertex_colors=True)
    folder = tmp_path_factory.mktemp("scan")
    obj = folder / "f.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f} {r:.6f} {g:.6f} {b:.6f}" for (x, y, z), (r, g, b)
                             in zip(face.verts.astype(np.float64), face.colors.astype(np.float64) / 255.0)) + "\n")
    ref = load_obj(obj)
    assert ref.n_tris == 0 and ref.n_verts == 41 * 41 and ref.colors is not None
    return obj, ref


@pytest.fixture(scope="module")
def by_hand(scan):
    """the Mesh the pipeline must be working on: the cloud's points, the model's triangles, the cloud's colours"""
    from mvlm_amd.utils import HipRenderer3D, Mesh

    _, ref = scan
    r = HipRenderer3D(n_views=1, verbose=False)
    _, _, normals, table = _prepare(r, _cloud(ref.verts))
    tris = cm.triangulate(ref.verts, normals, table)
    assert len(tris) > 3000 and cm.edge_uses(tris).max() <= 2
    return Mesh(np.ascontiguousarray(ref.verts), tris, colors=ref.colors)


def _pipe(**kw):
    from mvlm_amd import pipeline

    return pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, **kw)


def _same_report(a, b):
    np.testing.assert_array_equal(a.rows(), b.rows())
    for name in ("landmarks", "raw", "snapped", "tri", "bary", "uv", "scores", "view_dist2", "view_flags", "branch", "cov"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


# ---- 1. every option at once ----------------------------------------------------------------------------------------------------
def test_every_option_at_once(scan, tmp_path, monkeypatch):
    obj, ref = scan
    monkeypatch.chdir(tmp_path)
    pipe = _pipe(point_surface="mesh", **EVERYTHING)
    np.random.seed(4)
    landmarks = pipe.predict_one_file(obj)
    assert landmarks.shape == (73, 3) and np.isfinite(landmarks).all()
    report = pipe.last_report
    assert report is not None and len(report) == 73 and (report.tri >= 0).all()          # attached to triangles
    written = [pipe.last_view_path, pipe.last_sheet_path, pipe.last_surface_path] + list(pipe.last_ray_view_paths)
    assert len(written) == 3 + len(pipe.visualize_rays_poses)
    for path in written:
        assert path is not None and path.exists() and path.stat().st_size > 1000, path
    # the landmarks lie on the triangulated surface, not necessarily on a point
    d = np.linalg.norm(landmarks[:, None, :] - ref.verts[None].astype(np.float64), axis=2).min(axis=1)
    assert d.max() < 10.0 and (d > 1e-6).any()


@pytest.mark.parametrize("kw,match", [({"landmark_report": True}, "landmark_report"), ({"visualize_img": True}, "visualize_img"),
                                      ({"visualize_rays_img": True}, "visualize_rays_img"),
                                      ({"visualize_surface": True}, "visualize_surface"), ({"render_multisamples": 4}, "render_multisamples")])
def test_the_default_still_refuses(scan, kw, match):
    obj, ref = scan
    pipe = _pipe(**kw)
    assert pipe.point_surface == "splats"
    with pytest.raises(ValueError, match=match) as e:
        pipe.predict_one_file(obj)
    assert "is a point cloud" in str(e.value)
    with pytest.raises(ValueError, match=match):
        pipe.predict_mesh_device(_cloud(ref.verts, ref.colors), pipe.renderer_3d.generate_3d_transformations())


# ---- 2. equal to the mesh built by hand -----------------------------------------------------------------------------------------
def test_landmarks_and_report_equal_the_hand_built_mesh(scan, by_hand, tmp_path, monkeypatch):
    from mvlm_amd.__main__ import main

    obj, ref = scan
    monkeypatch.chdir(tmp_path)
    want_pipe = _pipe(landmark_report=True)
    poses = want_pipe.renderer_3d.generate_3d_transformations()                           # (8 views: the fixed table)
    np.random.seed(2)
    want, want_err = want_pipe.predict_mesh_device(by_hand, poses)
    want_report = want_pipe.last_report
    assert np.isfinite(want).all()

    pipe = _pipe(point_surface="mesh", landmark_report=True)
    np.random.seed(2)
    got, err = pipe.predict_mesh_device(_cloud(ref.verts, ref.colors), poses)
    np.testing.assert_array_equal(got, want)
    assert err == want_err
    _same_report(pipe.last_report, want_report)

    np.random.seed(2)
    np.testing.assert_array_equal(pipe.predict_one_file(obj), want)
    _same_report(pipe.last_report, want_report)

    np.random.seed(2)
    (file, landmarks), = list(pipe.predict_files([obj]))
    np.testing.assert_array_equal(landmarks, want)
    _same_report(pipe.last_report, want_report)

    np.random.seed(2)
    (landmarks, _), = pipe.predict_meshes_device([_cloud(ref.verts, ref.colors)])
    np.testing.assert_array_equal(landmarks, want)

    # the command line: the same landmarks and the same report file, and the picture
    out = tmp_path / "out"
    args = ["-p", str(obj.parent), "-o", str(out), "-n", "8", "--weights", "synthetic:5", "--pipelines", "dtu3d", "--seed", "2"]
    assert main(args + ["--point-surface", "mesh", "--report", "--visualize-img"]) == 0
    np.testing.assert_array_equal(np.loadtxt(out / "f_dtu3d.txt", delimiter=","), want)
    want_report.to_csv(tmp_path / "want.csv")
    assert (out / "f_dtu3d_report.csv").read_bytes() == (tmp_path / "want.csv").read_bytes()
    png = tmp_path / "visualization" / "f_dtu3d.png"
    assert png.exists() and png.stat().st_size > 1000
    # ... and without the flag the same command is refused as ever
    with pytest.raises(ValueError, match="is a point cloud: landmark_report is not supported"):
        main(args + ["--report"])


def test_the_slot_protocol_renders_the_triangulation(scan, by_hand):
    """multiview_render, the reference's renderer slot: under "mesh" the file's cloud is triangulated there too."""
    from mvlm_amd.utils import HipRenderer3D

    obj, _ = scan
    r = HipRenderer3D(n_views=8, verbose=False, point_surface="mesh")
    images, poses, mesh = r.multiview_render(obj)
    assert mesh.n_tris == by_hand.n_tris
    np.testing.assert_array_equal(mesh.tris, by_hand.tris)
    np.testing.assert_array_equal(images, r.render_device(by_hand, poses).cpu().numpy())
    splats, _, cloud = HipRenderer3D(n_views=8, verbose=False).multiview_render(obj)
    assert cloud.n_tris == 0 and not np.array_equal(splats, images)
