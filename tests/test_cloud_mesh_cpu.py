"""A point cloud's triangulation without a GPU: what the numpy statement of the contract (tests/cloud_mesh_model.py, fed the
brute-force neighbour table and normals of tests/cloud_normals_model.py) makes of a flat scan grid, of a face-like height field, of
duplicates and a NaN point and of the smallest clouds; and the option that turns the triangulation on - its parsing, what
Pipeline._check_cloud lets through under it (a stub renderer: no device), the command-line flag."""
import types

import numpy as np
import pytest

import cloud_mesh_model as cm
import cloud_normals_model as cn

NO_TRIS = np.zeros((0, 3), np.int32)


def _inputs(verts):
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    table = cn.neighbors(verts)
    return verts, cn.normals(verts, table)[0].astype(np.float32), table


def _triangulate(verts):
    verts, normals, table = _inputs(verts)
    return cm.triangulate(verts, normals, table)


@pytest.fixture(scope="module")
def face():
    from mvlm_amd.utils.synthetic import face_like_mesh

    return face_like_mesh(grid=25, tex_size=16, seed=1)


def _is_a_surface(tris, n_points):
    assert tris.dtype == np.int32 and tris.ndim == 2 and tris.shape[1] == 3
    assert (tris[:, 0] < tris[:, 1]).all() and (tris[:, 1] < tris[:, 2]).all() and tris.min() >= 0 and tris.max() < n_points
    order = np.lexsort((tris[:, 2], tris[:, 1], tris[:, 0]))
    np.testing.assert_array_equal(order, np.arange(len(tris)))                       # ascending, so no row twice
    assert len(np.unique(tris, axis=0)) == len(tris)
    assert cm.edge_uses(tris).max() <= 2                                             # no edge in more than two triangles


def test_a_flat_grid_is_triangulated_exactly():
    """21 x 21 points 10 apart: 2 * 20 * 20 triangles that tile the square - every co-circular tie of the grid broken one way."""
    verts = cm.flat_grid(21, 21, 10.0)
    tris = _triangulate(verts)
    _is_a_surface(tris, len(verts))
    assert len(tris) == 800
    assert cm.area(verts, tris) == 40000.0
    assert int((cm.edge_uses(tris) == 1).sum()) == 80


def test_a_flat_grid_turned_out_of_the_axes():
    """The same grid rotated: the same counts.  The rotated coordinates are rounded to float32 (2^-24 relative, of coordinates up
    to 142: 8.5e-6 absolute); the tiles still cover the outline, whose 80 boundary points each moved by at most that in a square of
    side 200: the area differs from 40 000 by less than 80 * 10 * 8.5e-6 = 6.8e-3, 1.7e-7 relative."""
    verts = cm.tilt(cm.flat_grid(21, 21, 10.0))
    tris = _triangulate(verts)
    _is_a_surface(tris, len(verts))
    assert len(tris) == 800
    assert int((cm.edge_uses(tris) == 1).sum()) == 80
    assert abs(cm.area(verts, tris) - 40000.0) <= 6.8e-3


def test_a_grid_turned_by_an_exact_rotation_keeps_its_area_exactly():
    """cm.exact_tilt: a rotation with rational entries and a step that makes every coordinate a float32 - no rounding at all."""
    verts = cm.exact_tilt(cm.flat_grid(21, 21, 8.125))
    tris = _triangulate(verts)
    _is_a_surface(tris, len(verts))
    assert len(tris) == 800
    assert abs(cm.area(verts, tris) - 400 * 8.125 ** 2) <= 1e-9 * 400 * 8.125 ** 2


def test_a_face_like_height_field(face):
    tris = _triangulate(face.verts)
    _is_a_surface(tris, face.n_verts)
    assert len(tris) == 1147 and face.n_tris == 1152
    share = cm.area(face.verts, tris) / cm.area(face.verts, face.tris)
    assert 0.99 <= share <= 1.0 + 1e-9, share


def test_a_jittered_height_field(face):
    verts = cm.jittered(face.verts)
    tris = _triangulate(verts)
    _is_a_surface(tris, len(verts))
    assert len(tris) > 1100


def test_the_sign_of_a_normal_does_not_matter(face):
    verts, normals, table = _inputs(cm.jittered(face.verts))
    want = cm.triangulate(verts, normals, table)
    flips = np.random.RandomState(0).choice([-1.0, 1.0], size=(len(verts), 1)).astype(np.float32)
    assert (flips == -1.0).sum() > 100
    np.testing.assert_array_equal(cm.triangulate(verts, normals * flips, table), want)
    np.testing.assert_array_equal(cm.triangulate(verts, normals * np.float32(-4.0), table), want)   # nor a power of two: 4 n is exact


def test_duplicates_and_a_nan_point():
    verts = cm.duplicates_and_nan()
    assert len(verts) == 206 and np.isnan(verts[100, 0])
    tris = _triangulate(verts)
    _is_a_surface(tris, len(verts))
    assert len(tris) > 250
    assert not (tris == 100).any()                                                   # the NaN point is in no triangle


def test_the_smallest_clouds():
    pts = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.float32)
    assert _triangulate(pts[:1]).shape == (0, 3)
    assert _triangulate(pts[:2]).shape == (0, 3)
    # three points: no covariance has a least direction worth the name, the plane's normal is what a scanner would give
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (3, 1))
    np.testing.assert_array_equal(cm.triangulate(pts, normals, cn.neighbors(pts)), [[0, 1, 2]])
    np.testing.assert_array_equal(_triangulate(pts), [[0, 1, 2]])                    # ... and so is the estimate's
    assert cm.triangulate(pts, np.zeros((3, 3), np.float32), cn.neighbors(pts)).shape == (0, 3)    # zero normals: empty stars
    assert cm.triangulate(pts, np.full((3, 3), np.nan, np.float32), cn.neighbors(pts)).shape == (0, 3)


def test_the_perturbation_depends_on_the_point_alone():
    assert cm.hash_units(0) != cm.hash_units(1)
    h = np.array([cm.hash_units(p) for p in range(2000)])
    assert h.min() >= -1.0 and h.max() < 1.0 and abs(h.mean()) < 0.05
    verts, _, table = _inputs(cm.flat_grid(5, 5, 4.0))
    u = cm.perturbed(verts, table)
    d = np.abs(u - verts.astype(np.float64)).max(axis=1)
    assert (d > 0).all() and (d <= 4.0 / 256.0).all()                                # 1/256 of the nearest-neighbour distance


# ---- the option --------------------------------------------------------------------------------------------------------------
def test_the_option_is_parsed():
    from mvlm_amd.__main__ import build_parser
    from mvlm_amd.utils.render3d import POINT_SURFACES, check_point_surface

    assert POINT_SURFACES == ("splats", "mesh")
    assert check_point_surface("splats") == "splats" and check_point_surface("mesh") == "mesh"
    for bad in ("Mesh", "triangles", None, 1):
        with pytest.raises(ValueError, match="'splats' or 'mesh'"):
            check_point_surface(bad)
    assert build_parser().parse_args(["-p", "x"]).point_surface == "splats"
    assert build_parser().parse_args(["-p", "x", "--point-surface", "mesh"]).point_surface == "mesh"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-p", "x", "--point-surface", "hull"])


def test_the_pipeline_refuses_another_value_before_it_builds_anything():
    from mvlm_amd import config, pipeline

    with pytest.raises(ValueError, match="point_surface must be 'splats' or 'mesh', not 'hull'"):
        pipeline.create_pipeline("dtu3d", point_surface="hull", verbose=False)
    with pytest.raises(ValueError, match="point_surface must be 'splats' or 'mesh', not 'hull'"):
        pipeline.pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=8), point_surface="hull", verbose=False)


def _stub_pipeline(point_surface=None, **kw):
    r3 = types.SimpleNamespace(shading="texture", point_normals="file", multisamples=kw.pop("multisamples", 0))
    fields = dict(landmark_report=False, visualize_img=False, visualize_rays_img=False, visualize_surface=False, renderer_3d=r3)
    fields.update(kw)
    if point_surface is not None:
        fields["point_surface"] = point_surface
    return types.SimpleNamespace(**fields)


REFUSED = (({"landmark_report": True}, "landmark_report is not supported"), ({"visualize_img": True}, "visualize_img is not supported"),
           ({"visualize_rays_img": True}, "visualize_rays_img is not supported"),
           ({"visualize_surface": True}, "visualize_surface is not supported"), ({"multisamples": 4}, "render_multisamples=4"))


@pytest.mark.parametrize("kw,match", REFUSED)
def test_check_cloud_under_both_values(kw, match):
    from mvlm_amd.pipeline.general_pipeline import Pipeline
    from mvlm_amd.utils import Mesh

    verts = cm.flat_grid(3, 3)
    cloud, mesh = Mesh(verts, NO_TRIS), Mesh(verts, np.array([[0, 1, 3]], np.int32))
    check = Pipeline._check_cloud
    for stub in (_stub_pipeline(None, **dict(kw)), _stub_pipeline("splats", **dict(kw))):     # the default: refused as ever
        with pytest.raises(ValueError, match=match) as e:
            check(stub, cloud)
        assert "is a point cloud" in str(e.value)
        check(stub, mesh)
    check(_stub_pipeline("mesh", **dict(kw)), cloud)                                            # the cloud will have triangles
    check(_stub_pipeline("mesh", **dict(kw)), mesh)


def test_every_option_at_once_passes_under_mesh():
    from mvlm_amd.pipeline.general_pipeline import Pipeline
    from mvlm_amd.utils import Mesh

    cloud = Mesh(cm.flat_grid(3, 3), NO_TRIS)
    everything = dict(landmark_report=True, visualize_img=True, visualize_rays_img=True, visualize_surface=True, multisamples=4)
    Pipeline._check_cloud(_stub_pipeline("mesh", **dict(everything)), cloud)
    with pytest.raises(ValueError, match="is a point cloud"):
        Pipeline._check_cloud(_stub_pipeline("splats", **dict(everything)), cloud)


def test_the_surface_hook_leaves_meshes_and_the_default_alone():
    from mvlm_amd.pipeline.general_pipeline import Pipeline
    from mvlm_amd.utils import Mesh

    verts = cm.flat_grid(3, 3)
    cloud, mesh = Mesh(verts, NO_TRIS), Mesh(verts, np.array([[0, 1, 3]], np.int32))
    made = Mesh(verts, np.array([[0, 1, 4]], np.int32))
    r3 = types.SimpleNamespace(triangulate_point_cloud=lambda m: made)
    splats, as_mesh = types.SimpleNamespace(point_surface="splats", renderer_3d=r3), types.SimpleNamespace(point_surface="mesh", renderer_3d=r3)
    assert Pipeline._surface(splats, cloud) is cloud and Pipeline._surface(splats, mesh) is mesh
    assert Pipeline._surface(as_mesh, mesh) is mesh and Pipeline._surface(as_mesh, None) is None
    assert Pipeline._surface(as_mesh, cloud) is made
    with pytest.raises(ValueError, match="needs a renderer that triangulates"):
        Pipeline._surface(types.SimpleNamespace(point_surface="mesh", renderer_3d=types.SimpleNamespace()), cloud)


def test_the_mesh_class_carries_point_ids():
    from mvlm_amd.utils import Mesh

    assert Mesh(cm.flat_grid(2, 2), NO_TRIS).point_ids is None
    ids = np.arange(4, dtype=np.int32)
    assert Mesh(cm.flat_grid(2, 2), NO_TRIS, point_ids=ids).point_ids is ids
