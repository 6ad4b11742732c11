"""-m gpu: normals of point clouds on the device - the geometry shade of a cloud's splats against the numpy statement of the
contract (tests/cloud_normals_model.py) bit for bit, the neighbour table of the estimate against brute force, the estimated normals
against numpy.linalg.eigh, determinism, the refusals, and a cloud with a file's normals and one with estimated ones through every
layer down to the command line.  All clouds are small: the brute-force model is O(V^2)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cloud_normals_model as cm
import points_model as pm

pytestmark = pytest.mark.gpu

NO_TRIS = np.zeros((0, 3), np.int32)
FRONT = np.zeros((1, 6), np.float32)
FAR = np.float32(1.0) / np.float32(255.0)


def _cloud(verts, normals=None, radius=None):
    from mvlm_amd.utils import Mesh

    return Mesh(np.ascontiguousarray(verts, np.float32).reshape(-1, 3), NO_TRIS, normals=normals, point_radius=radius)


def _renderer(n_views=1, **kw):
    from mvlm_amd.utils import HipRenderer3D

    return HipRenderer3D(n_views=n_views, verbose=False, **kw)


def _hip(mesh, poses, **kw):
    r = _renderer(len(poses), **kw)
    out = r.render_device(mesh, np.asarray(poses)).cpu().numpy()
    r.check()
    return out


def _face():
    from mvlm_amd.utils.synthetic import face_like_mesh

    return face_like_mesh(grid=41, tex_size=16, seed=1).verts


@functools.lru_cache(maxsize=None)
def _points(name):
    """The clouds of the search tests, by name (float32 [V,3], read-only)."""
    rs = np.random.RandomState(17)
    if name == "face":                      # a regular 5-unit grid in xy: most 16th places are exact ties decided by id
        v = _face()
    elif name == "lattice":                 # 12 x 12 x 3 integer lattice x 4: ties in all directions
        v = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 4.0
    elif name in ("10", "16", "17"):        # fewer than, exactly and one more than K points
        v = rs.uniform(-50, 50, size=(int(name), 3))
    elif name == "cluster":                 # 500 points in a 1e-3 cube and 50 over +-100: shells expand far, the cell cap bites
        v = np.concatenate([rs.uniform(0, 1e-3, size=(500, 3)) + [3.0, -2.0, 7.0], rs.uniform(-100, 100, size=(50, 3))])
        v = v[rs.permutation(len(v))]
    elif name == "coincident":              # 40 coincident points among 200 others
        v = rs.uniform(-60, 60, size=(240, 3))
        v[rs.choice(240, 40, replace=False)] = [12.5, -7.25, 3.0]
    elif name == "holes":                   # the face with every 7th point NaN or inf
        v = _face().copy()
        v[::14, 0] = np.nan
        v[7::14, 2] = np.inf
    elif name == "line":                    # 300 collinear points: two zero extents
        v = np.stack([np.linspace(-90, 90, 300), np.full(300, 4.0), np.full(300, -2.0)], axis=1)
    elif name == "one":
        v = np.array([[1.0, 2.0, 3.0]])
    elif name == "sphere":
        g = np.random.default_rng(7).normal(size=(1500, 3))
        v = 80.0 * g / np.linalg.norm(g, axis=1, keepdims=True)
    elif name == "plane":
        lin = (np.arange(30) - 14.5) * 4.0
        x, y = np.meshgrid(lin, lin)
        v = np.stack([x.ravel(), y.ravel(), np.full(x.size, 5.0)], axis=1)
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _model(name):
    """(table, normals float64, eigenvalues) of the brute-force model, computed once per cloud."""
    v = _points(name)
    table = cm.neighbors(v)
    n, lam = cm.normals(v, table)
    for a in (table, n, lam):
        a.setflags(write=False)
    return table, n, lam


@functools.lru_cache(maxsize=None)
def _estimate(name):
    """(normals, table) of the device for the cloud, estimated once."""
    n, t = _renderer().estimate_point_normals(_cloud(_points(name)), return_neighbors=True)
    n.setflags(write=False)
    t.setflags(write=False)
    return n, t


# ---- 1. the shade, exact ----------------------------------------------------------------------------------------------------
def _face_normals():
    v = _face().astype(np.float64)
    z = v[:, 2].reshape(41, 41)
    dzdy, dzdx = np.gradient(z, 5.0)                      # rows run along y, columns along x
    n = np.stack([-dzdx.ravel(), -dzdy.ravel(), np.ones(41 * 41)], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n = n.astype(np.float32)
    n[820] = 0.0                                          # a zero normal: shade 0
    n[861] = [np.nan, 0.0, 1.0]                           # a NaN normal: shade 0
    n[902] *= np.float32(7.5)                             # not of unit length: the shade divides
    return n


@pytest.mark.parametrize("radius_px", [None, 3.0])
def test_the_shade_of_given_normals_is_the_models(radius_px):
    verts, normals = _face(), _face_normals()
    poses = np.array([[0, 0, 0, 0, 0, 0], [25, -40, 10, 0, 0, 0], _renderer(8).generate_3d_transformations()[2]], np.float32)
    radius = None if radius_px is None else pm.px_to_model(radius_px)
    got = _hip(_cloud(verts, normals, radius), poses, shading="geometry")
    texture_mode = pm.render(verts, poses, radius)
    np.testing.assert_array_equal(got[..., 3], texture_mode[..., 3])                        # the depth plane, and with it ...
    covered = got[..., 3] != FAR
    np.testing.assert_array_equal(covered, texture_mode[..., 3] != FAR)                      # ... the covered set
    np.testing.assert_array_equal(got[..., 0], got[..., 1])
    np.testing.assert_array_equal(got[..., 0], got[..., 2])
    want = cm.render(verts, normals, poses, radius)
    np.testing.assert_array_equal(got, want)
    assert (got[..., 0][~covered] == 1.0).all()                                             # white background
    shades = np.rint(want[..., 0][covered] * 255).astype(int)
    assert shades.min() == 0 and shades.max() > 250 and len(np.unique(shades)) > 50         # the planted zeros show; a real picture
    # the same cloud in texture mode on the same context afterwards: the key plane came back EMPTY
    np.testing.assert_array_equal(_hip(_cloud(verts, normals, radius), poses), texture_mode)


# ---- 2. the neighbours, exact -----------------------------------------------------------------------------------------------
SEARCH_CLOUDS = ["face", "lattice", "10", "16", "17", "cluster", "coincident", "holes", "line", "one"]


@pytest.mark.parametrize("name", SEARCH_CLOUDS)
def test_the_neighbour_table_is_brute_force(name):
    want = _model(name)[0]
    got = _estimate(name)[1]
    assert got.dtype == np.int32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    if name == "lattice":   # what makes the case worth having: the 16th place is an exact tie that the id decides
        v = _points(name).astype(np.float64)
        centre = int(np.argmin(np.abs(v - [24.0, 24.0, 4.0]).sum(axis=1)))
        d2 = ((v - v[centre]) ** 2).sum(axis=1)
        assert (d2 == np.sort(d2)[15]).sum() > 1 and (d2 < np.sort(d2)[15]).sum() < 15
    if name == "holes":
        bad = ~np.isfinite(_points(name)).all(axis=1)
        assert bad.sum() > 200 and (got[bad] == -1).all() and not np.isin(got, np.nonzero(bad)[0]).any()


# ---- 3. the normals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["face", "lattice", "sphere"])
def test_estimated_normals_are_eighs(name):
    """Bound 1e-6 on |n_gpu x n_model| and on | |n_gpu| - 1 |, derived: storing a unit vector as float32 moves it by at most
    sqrt(3) 2^-24 = 1.0e-7, a float64 solve at an eigenvalue gap of (l1 - l0) >= 0.05 l2 adds about 1e-14."""
    _, want, lam = _model(name)
    got = _estimate(name)[0].astype(np.float64)
    assert np.isfinite(lam).all()
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    print(f"{name}: least (l1 - l0) / l2 = {gap.min():.4f}")
    assert (lam[:, 1] - lam[:, 0] >= 0.05 * lam[:, 2]).all()                                # no point is excluded
    length = np.linalg.norm(got, axis=1)
    cross = np.linalg.norm(np.cross(got / length[:, None], want / np.linalg.norm(want, axis=1, keepdims=True)), axis=1)
    print(f"{name}: worst |n_gpu x n_model| = {cross.max():.3e}, worst | |n_gpu| - 1 | = {np.abs(length - 1).max():.3e}")
    assert cross.max() <= 1e-6
    assert np.abs(length - 1.0).max() <= 1e-6
    if name == "sphere":                                                                    # and they are the sphere's normals
        radial = np.abs((got * _points(name).astype(np.float64)).sum(axis=1)) / 80.0
        assert radial.min() > 0.99


@pytest.mark.parametrize("name", ["10", "coincident", "holes", "one"])
def test_degenerate_rows_are_exactly_zero(name):
    _, want, _ = _model(name)
    got = _estimate(name)[0]
    zero = ~want.any(axis=1)                                # non-finite point, fewer than 3 neighbours, zero covariance
    assert got.dtype == np.float32 and (got[zero] == 0.0).all()
    assert (np.abs(np.linalg.norm(got[~zero].astype(np.float64), axis=1) - 1.0) <= 1e-6).all()
    expect = {"10": 0, "coincident": 40, "holes": int((~np.isfinite(_points(name)).all(axis=1)).sum()), "one": 1}[name]
    assert int(zero.sum()) == expect


def test_a_plane_seen_from_the_front_is_white():
    verts = _points("plane")
    mesh = _cloud(verts)
    r = _renderer(point_normals="estimate", shading="geometry")
    got = r.render_device(mesh, FRONT).cpu().numpy()        # estimated by the upload: no normals on the host
    r.check()
    assert mesh.normals is None
    covered = got[0, :, :, 3] != FAR
    assert covered.sum() > 5000 and (got[0, :, :, 0][covered] == 1.0).all()                 # shade 255 on every covered pixel
    np.testing.assert_array_equal(got[0, :, :, 3], pm.render(verts, FRONT)[0, :, :, 3])
    n = r.estimate_point_normals(mesh)
    np.testing.assert_array_equal(np.abs(n), np.tile(np.float32([0, 0, 1]), (len(verts), 1)))
    assert mesh.normals is n


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["face", "cluster"])
def test_estimating_twice_gives_the_same_bytes(name):
    verts = _points(name)
    poses = np.array([[0, 0, 0, 0, 0, 0], [-30, 45, 0, 0, 0, 0]], np.float32)
    r = _renderer(2, shading="geometry")
    seen = []
    for _ in range(2):
        mesh = _cloud(verts)
        n, t = r.estimate_point_normals(mesh, return_neighbors=True)
        views = r.render_device(mesh, poses).cpu().numpy()
        r.check()
        seen.append((n.tobytes(), t.tobytes(), views.tobytes()))
    assert seen[0] == seen[1]
    np.testing.assert_array_equal(np.frombuffer(seen[0][1], np.int32).reshape(-1, 16), _estimate(name)[1])


# ---- 5. refusals, and the context afterwards ----------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    from mvlm_amd import _lib
    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.render3d import upload_mesh
    from mvlm_amd.utils.synthetic import face_like_mesh

    face = face_like_mesh(grid=12, tex_size=16, seed=1)
    cloud = _cloud(face.verts)
    want = pm.render(cloud.verts, FRONT)
    r = _renderer()
    lib, h = r.ctx.lib, r.ctx.handle
    nrm = np.ascontiguousarray(np.tile(np.float32([0, 0, 1]), (face.n_verts, 1)))

    def still_renders():
        np.testing.assert_array_equal(_hip(cloud, FRONT), want)

    tri_mesh = Mesh(face.verts, face.tris)
    tri_handle = upload_mesh(r.ctx, tri_mesh)
    assert lib.mvlm_mesh_upload_normals(h, tri_handle, _lib.as_ptr(nrm, C.c_float), face.n_verts) != 0
    assert "has triangles" in lib.mvlm_last_error(h).decode()
    still_renders()
    assert lib.mvlm_mesh_estimate_normals(h, tri_handle, None) != 0
    assert "has triangles" in lib.mvlm_last_error(h).decode()
    with pytest.raises(ValueError, match="has triangles"):
        r.estimate_point_normals(tri_mesh)
    still_renders()
    handle = upload_mesh(r.ctx, cloud)
    for bad in (face.n_verts - 1, face.n_verts + 1, 0):
        assert lib.mvlm_mesh_upload_normals(h, handle, _lib.as_ptr(nrm, C.c_float), bad) != 0
        assert "normals for a mesh of" in lib.mvlm_last_error(h).decode()
    host = np.empty((face.n_verts, 3), np.float32)
    assert lib.mvlm_mesh_copy_normals(h, handle, _lib.as_ptr(host, C.c_float)) != 0         # nothing attached by the refused calls
    still_renders()
    with pytest.raises(ValueError, match="float32 \\[V,3\\]"):
        _hip(_cloud(face.verts, nrm[:-1]), FRONT, shading="geometry")
    still_renders()
    with pytest.raises(ValueError, match="geometry shading of a point cloud") as e:         # no normals, point_normals="file"
        _hip(_cloud(face.verts), FRONT, shading="geometry")
    assert "point cloud" in str(e.value) and "point_normals" in str(e.value)
    still_renders()
    with pytest.raises(ValueError, match="multisampled rendering of a point cloud"):        # with normals too
        _hip(_cloud(face.verts, nrm), FRONT, shading="geometry", multisamples=4)
    still_renders()
    with pytest.raises(ValueError, match="point_normals"):
        _renderer(point_normals="guess")
    # a mesh with triangles and normals renders under geometry shading as the same mesh without
    np.testing.assert_array_equal(_hip(Mesh(face.verts, face.tris, normals=nrm), FRONT, shading="geometry"),
                                  _hip(Mesh(face.verts, face.tris), FRONT, shading="geometry"))
    still_renders()


# ---- 6. every layer -----------------------------------------------------------------------------------------------------------
def _write_ply(path, verts, normals):
    with open(path, "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\n"
                 "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n").encode())
        rec = np.zeros(len(verts), np.dtype([("p", "<f4", 3), ("n", "<f4", 3)]))
        rec["p"], rec["n"] = verts, normals
        f.write(rec.tobytes())


def _is_a_point_of(landmarks, verts):
    rows = {r.tobytes() for r in np.asarray(verts, np.float32).astype(np.float64)}
    return all(np.ascontiguousarray(lm, np.float64).tobytes() in rows for lm in landmarks)


def test_clouds_with_normals_go_through_every_layer(tmp_path):
    from mvlm_amd import config
    from mvlm_amd.__main__ import main
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils import load_mesh
    from mvlm_amd.utils.mesh_io import load_obj

    verts, normals = _face(), _face_normals()
    cfg = config.default_config("DTU3D", "geometry+depth", n_views=8)
    # (a) a .ply that carries normals: no option needed
    ply = tmp_path / "scan.ply"
    _write_ply(ply, verts, normals)
    pipe = pipeline_from_config(cfg, weights="synthetic:5", verbose=False)
    assert pipe.renderer_3d.shading == "geometry" and pipe.renderer_3d.point_normals == "file"
    poses = pipe.renderer_3d.generate_3d_transformations()
    mesh = load_mesh(ply)
    np.testing.assert_array_equal(mesh.normals, normals)
    images = pipe.renderer_3d.render_device(mesh, poses).cpu().numpy()
    pipe.renderer_3d.check()
    np.testing.assert_array_equal(images, cm.render(verts, normals, poses))
    np.random.seed(3)
    lm_a, _ = pipe.predict_mesh_device(mesh, poses)
    np.random.seed(3)
    lm_b, _ = pipe.predict_mesh_device(load_mesh(ply), poses)
    np.testing.assert_array_equal(lm_a, lm_b)
    assert lm_a.shape == (73, 3) and np.isfinite(lm_a).all() and _is_a_point_of(lm_a, verts)
    # (b) an .obj of bare v lines: refused without the option, estimated with it
    work = tmp_path / "scans"
    work.mkdir()
    obj = work / "f.obj"
    obj.write_text("\n".join(f"v {x:.6f} {y:.6f} {z:.6f}" for x, y, z in verts.astype(np.float64)) + "\n")
    with pytest.raises(ValueError, match="geometry") as e:
        pipe.predict_one_file(obj)
    assert "point_normals" in str(e.value)
    with pytest.raises(ValueError, match="geometry"):
        pipe.predict_mesh_device(load_obj(obj), poses)
    est = pipeline_from_config(cfg, weights="synthetic:5", verbose=False, point_normals="estimate")
    assert est.renderer_3d.point_normals == "estimate"
    ref = load_obj(obj)
    assert ref.n_tris == 0 and ref.normals is None
    images, poses2, slot_mesh = est.renderer_3d.multiview_render(obj)                       # the slot protocol
    np.testing.assert_array_equal(poses2, poses)
    estimated = _renderer().estimate_point_normals(_cloud(ref.verts))
    np.testing.assert_array_equal(images, cm.render(ref.verts, estimated, poses))
    shades = np.rint(images[..., 0][images[..., 3] != FAR] * 255).astype(int)
    assert len(np.unique(shades)) > 50                                                      # not a white silhouette
    np.random.seed(3)
    one = est.predict_one_file(obj)
    np.random.seed(3)
    fused, _ = est.predict_mesh_device(load_obj(obj), poses)
    np.random.seed(3)
    listed = [lm for _, lm in est.predict_files([obj])]
    np.testing.assert_array_equal(one, fused)
    np.testing.assert_array_equal(one, listed[0])
    assert one.shape == (73, 3) and np.isfinite(one).all() and _is_a_point_of(one, ref.verts)
    # the file's normals win over the estimate: the .ply's views are the same under "estimate"
    np.testing.assert_array_equal(est.renderer_3d.render_device(load_mesh(ply), poses).cpu().numpy(), cm.render(verts, normals, poses))
    # the command line
    out = tmp_path / "out"
    args = ["-p", str(work), "-o", str(out), "-c", "DTU3D-geometry+depth", "-n", "8", "--weights", "synthetic:5", "--seed", "3"]
    with pytest.raises(ValueError, match="geometry"):
        main(args)
    assert main(args + ["--point-normals", "estimate"]) == 0
    lm = np.loadtxt(out / "f_DTU3D-geometry+depth.txt", delimiter=",")
    assert lm.shape == (73, 3) and np.isfinite(lm).all()
