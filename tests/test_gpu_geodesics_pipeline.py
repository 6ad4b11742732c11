"""-m gpu: landmark_distances through the pipeline - on a synthetic face with planted weights every prediction leaves
``last_distances``, equal to a direct HipRenderer3D.landmark_geodesics call on the landmarks it returned; the pair list; the command
line's CSV; a pre-align scale divided out; a cloud refused and, with point_surface="mesh", measured; and with the option off the
landmarks of before, bit for bit, and not a byte of the feature's scratch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [(0, 16), (8, 27)]


def _write_obj(path, verts, tris=None):
    lines = [f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in np.asarray(verts, np.float64)]
    if tris is not None:
        lines += [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in np.asarray(tris)]
    path.write_text("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """(the scan's file, its Mesh as the loader reads it, the same points as a cloud's file)"""
    from mvlm_amd.utils.mesh_io import load_obj
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=41, tex_size=64, seed=2)
    folder = tmp_path_factory.mktemp("scan")
    _write_obj(folder / "f.obj", face.verts, face.tris)
    cloud_folder = tmp_path_factory.mktemp("cloud")
    _write_obj(cloud_folder / "c.obj", face.verts)
    ref = load_obj(folder / "f.obj")
    assert ref.n_tris == face.n_tris > 3000
    return folder / "f.obj", ref, cloud_folder / "c.obj"


def _pipe(**kw):
    from mvlm_amd import pipeline

    return pipeline.create_pipeline("dtu3d", n_views=8, weights="synthetic:5", verbose=False, **kw)


def _same(a, b):
    for name in ("snapped", "tri", "euclidean", "directed", "sweeps"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


@pytest.fixture(scope="module")
def measured(scan):
    """one prediction with the option on: (the pipeline, its landmarks, its distances)"""
    obj, _, _ = scan
    pipe = _pipe(landmark_distances=True)
    np.random.seed(3)
    landmarks = pipe.predict_one_file(obj)
    return pipe, landmarks, pipe.last_distances


def test_last_distances_equal_a_direct_call(scan, measured):
    _, ref, _ = scan
    pipe, landmarks, found = measured
    assert landmarks.shape == (73, 3) and found is not None and found.directed.shape == (73, 73)
    direct = pipe.renderer_3d.landmark_geodesics(ref, landmarks)
    _same(found, direct)
    off = ~np.eye(73, dtype=bool)
    assert (found.tri >= 0).all() and np.isfinite(found.directed).all() and (np.diag(found.directed) == 0).all()
    assert (found.geodesic[off] >= found.euclidean[off] * (1 - 1e-12)).all()           # never below the straight distance
    far = found.euclidean > 20
    assert (found.geodesic[far] <= found.euclidean[far] * 3).all()                      # ... and a distance along a face
    assert "distances" in pipe.timings
    # predict_files and predict_meshes_device: the scans go one by one, each leaves its own
    np.random.seed(3)
    (_, again), = list(pipe.predict_files([scan[0]]))
    np.testing.assert_array_equal(again, landmarks)
    _same(pipe.last_distances, found)
    pipe.last_distances = None
    np.random.seed(3)
    (again, _), = pipe.predict_meshes_device([ref])
    np.testing.assert_array_equal(again, landmarks)
    _same(pipe.last_distances, found)
    assert not pipe._groupable(2)


def test_with_the_option_off_nothing_changes(scan, measured):
    obj, _, _ = scan
    _, landmarks, _ = measured
    pipe = _pipe()
    # (renderers of one device share one context: what the pipeline of `measured` left there is given back first)
    pipe.renderer_3d.release_geodesics()
    assert pipe.renderer_3d.scratch_bytes("geodesic") == 0
    np.random.seed(3)
    np.testing.assert_array_equal(pipe.predict_one_file(obj), landmarks)
    assert pipe.last_distances is None and "distances" not in pipe.timings
    assert pipe.renderer_3d.scratch_bytes("geodesic") == 0


def test_the_pair_list(scan, measured):
    obj, _, _ = scan
    _, landmarks, full = measured
    pipe = _pipe(landmark_distances=True, distance_pairs=PAIRS)
    np.random.seed(3)
    np.testing.assert_array_equal(pipe.predict_one_file(obj), landmarks)
    found = pipe.last_distances
    rows = found.rows()
    assert [r[:2] for r in rows] == PAIRS
    for i, j, e, g, gij, gji in rows:
        assert (e, gij, gji) == (full.euclidean[i, j], full.directed[i, j], full.directed[j, i]) and g == full.geodesic[i, j]
    assert np.isnan(found.directed).sum() == 73 * 73 - 4
    with pytest.raises(ValueError, match=r"distance_pairs: landmark indices must lie in 0\.\.72"):
        _pipe(landmark_distances=True, distance_pairs=[(0, 73)]).predict_one_file(obj)


def test_the_command_line_writes_the_table(scan, measured, tmp_path):
    from mvlm_amd.__main__ import main

    obj, _, _ = scan
    _, landmarks, full = measured
    args = ["-p", str(obj.parent), "-n", "8", "--weights", "synthetic:5", "--pipelines", "dtu3d", "--seed", "3", "--distances"]
    assert main(args + ["-o", str(tmp_path / "all")]) == 0
    np.testing.assert_array_equal(np.loadtxt(tmp_path / "all" / "f_dtu3d.txt", delimiter=","), landmarks)
    full.to_csv(tmp_path / "want.csv")
    got = (tmp_path / "all" / "f_dtu3d_distances.csv").read_text()
    assert got == (tmp_path / "want.csv").read_text()
    lines = got.splitlines()
    assert lines[0] == "i,j,euclidean,geodesic,geodesic_ij,geodesic_ji" and len(lines) == 1 + 73 * 72 // 2 and lines[1].startswith("0,1,")
    assert main(args + ["-o", str(tmp_path / "two"), "--distance-pairs", "0-16,8-27"]) == 0
    table = np.genfromtxt(tmp_path / "two" / "f_dtu3d_distances.csv", delimiter=",", names=True)
    assert table["i"].tolist() == [0, 8] and table["j"].tolist() == [16, 27]
    assert table["geodesic"].tolist() == [full.geodesic[0, 16], full.geodesic[8, 27]]
    assert table["euclidean"].tolist() == [full.euclidean[0, 16], full.euclidean[8, 27]]


def test_a_pre_align_scale_divides_out(scan):
    from mvlm_amd.utils.prealign import aligned

    obj, ref, _ = scan
    block = {"align_center_of_mass": False, "rot_x": 0, "rot_y": 0, "rot_z": 0, "scale": 0.5}
    pipe = _pipe(landmark_distances=True)
    pipe.pre_align = block
    small = aligned(ref, block)
    assert small.to_original is not None
    poses = pipe.renderer_3d.generate_3d_transformations()
    np.random.seed(5)
    in_model_space, _ = pipe.predict_mesh_device(small, poses)
    found = pipe.last_distances
    direct = pipe.renderer_3d.landmark_geodesics(small, in_model_space)
    np.testing.assert_array_equal(found.directed, direct.directed / 0.5)
    np.testing.assert_array_equal(found.euclidean, direct.euclidean / 0.5)
    # in the scan's own units: the straight distances of the landmarks the caller gets, up to the mapping's rounding
    np.random.seed(5)
    landmarks = pipe.predict_one_file(obj)
    np.testing.assert_array_equal(pipe.last_distances.directed, found.directed)
    straight = np.sqrt(((landmarks[:, None, :] - landmarks[None, :, :]) ** 2).sum(axis=2))
    np.testing.assert_allclose(pipe.last_distances.euclidean, straight, rtol=0, atol=1e-9 * np.abs(landmarks).max())


def test_a_cloud_is_refused_and_its_mesh_is_measured(scan):
    _, _, cloud = scan
    with pytest.raises(ValueError, match=r"c\.obj is a point cloud: landmark_distances is not supported \("):
        _pipe(landmark_distances=True).predict_one_file(cloud)
    pipe = _pipe(landmark_distances=True, point_surface="mesh")
    np.random.seed(3)
    landmarks = pipe.predict_one_file(cloud)
    found = pipe.last_distances
    assert np.isfinite(landmarks).all() and found is not None and (found.tri >= 0).all()
    close = found.euclidean < 30
    assert np.isfinite(found.directed[close]).all() and not np.isnan(found.directed).any()
