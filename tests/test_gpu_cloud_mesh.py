"""-m gpu: a point cloud's triangulation on the device (cloud_mesh.hip: mvlm_mesh_triangulate_points) against the numpy statement
of its contract (tests/cloud_mesh_model.py) row for row - the model is fed the device's own neighbour table and normals, so what
is compared is the triangulation alone -, a grid past the scan's block size and one past a slice of its block sums checked by what
they must be, the count-only call and a cap that is too small, the refusals, the stage times, and the Mesh that
HipRenderer3D.triangulate_point_cloud returns."""
import ctypes as C

import numpy as np
import pytest

import cloud_mesh_model as cm

pytestmark = pytest.mark.gpu

NO_TRIS = np.zeros((0, 3), np.int32)
FRONT = np.zeros((1, 6), np.float32)
UNWRITTEN = -7


def _cloud(verts, colors=None, normals=None):
    from mvlm_amd.utils import Mesh

    return Mesh(np.ascontiguousarray(verts, np.float32).reshape(-1, 3), NO_TRIS, colors=colors, normals=normals)


@pytest.fixture(scope="module")
def renderer():
    from mvlm_amd.utils import HipRenderer3D

    return HipRenderer3D(n_views=1, verbose=False)


def _table(r, verts):
    """the device's neighbour table of these points (and its estimate of their normals), through a cloud of its own"""
    normals, table = r.estimate_point_normals(_cloud(verts), return_neighbors=True)
    return normals, np.ascontiguousarray(table, np.int32)


def _prepare(r, cloud, file_normals=False):
    """-> (device handle, the table as a device tensor, the device copy's normals, the table on the host): the estimate, then - with
    ``file_normals`` - the cloud's own normals over it.  The handle is the cloud's device copy, freed with the Mesh object: a caller
    that goes on to use it keeps ``cloud`` alive."""
    import torch

    from mvlm_amd import _lib
    from mvlm_amd.utils.render3d import upload_mesh

    ctx = r.ctx
    dev = torch.device("cuda", ctx.device)
    own = cloud.normals if file_normals else None
    cloud.normals = None
    handle = upload_mesh(ctx, cloud)
    ctx.bind_current_stream(torch, dev)
    table = torch.empty((cloud.n_verts, 16), dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.mvlm_mesh_estimate_normals(ctx.handle, handle, C.c_void_p(table.data_ptr())))
    if own is not None:
        own = np.ascontiguousarray(own, np.float32)
        ctx.check(ctx.lib.mvlm_mesh_upload_normals(ctx.handle, handle, _lib.as_ptr(own, C.c_float), cloud.n_verts))
    normals = np.empty((cloud.n_verts, 3), np.float32)
    ctx.check(ctx.lib.mvlm_mesh_copy_normals(ctx.handle, handle, _lib.as_ptr(normals, C.c_float)))
    if own is not None:
        np.testing.assert_array_equal(normals.view(np.uint32), own.view(np.uint32))
    return handle, table, normals, table.cpu().numpy()


def _call(r, handle, table, cap, rows=None, with_tris=True):
    """one mvlm_mesh_triangulate_points -> (return code, the count, the caller's buffer of ``rows`` rows, pre-filled)"""
    import torch

    dev = torch.device("cuda", r.ctx.device)
    rows = cap if rows is None else rows
    tris = torch.full((max(rows, 1), 3), UNWRITTEN, dtype=torch.int32, device=dev)
    count = torch.full((1,), UNWRITTEN, dtype=torch.int32, device=dev)
    r.ctx.bind_current_stream(torch, dev)
    rc = r.ctx.lib.mvlm_mesh_triangulate_points(r.ctx.handle, handle, None if table is None else C.c_void_p(table.data_ptr()),
                                                C.c_void_p(tris.data_ptr()) if with_tris else None, C.c_longlong(cap),
                                                C.c_void_p(count.data_ptr()))
    torch.cuda.synchronize()
    return rc, int(count.item()), tris.cpu().numpy()[:rows]


def _device_tris(r, cloud, file_normals=False):
    """-> (the device's triangle array, the model's from the same table and normals)"""
    handle, table, normals, table_host = _prepare(r, cloud, file_normals)
    cap = 3 * cloud.n_verts + 1024
    rc, n, tris = _call(r, handle, table, cap)
    assert rc == 0, r.ctx.lib.mvlm_last_error(r.ctx.handle).decode()
    assert 0 <= n <= cap
    assert (tris[n:] == UNWRITTEN).all()
    return tris[:n], cm.triangulate(cloud.verts, normals, table_host)


def _face(grid=25):
    from mvlm_amd.utils.synthetic import face_like_mesh

    return face_like_mesh(grid=grid, tex_size=32, seed=1, vertex_colors=True)


def _render(r, mesh):
    out = r.render_device(mesh, FRONT).cpu().numpy()
    r.check()
    return out


# ---- 1. the device's array is the model's --------------------------------------------------------------------------------------
def test_a_tilted_flat_grid(renderer):
    verts = cm.tilt(cm.flat_grid(21, 21, 10.0))
    got, want = _device_tris(renderer, _cloud(verts))
    np.testing.assert_array_equal(got, want)
    assert len(got) == 800 and cm.edge_uses(got).max() == 2 and int((cm.edge_uses(got) == 1).sum()) == 80


def test_a_jittered_face_with_colours(renderer):
    face = _face()
    got, want = _device_tris(renderer, _cloud(cm.jittered(face.verts), face.colors))
    np.testing.assert_array_equal(got, want)
    assert len(got) > 1100 and cm.edge_uses(got).max() <= 2


def test_duplicates_and_a_nan_point(renderer):
    verts = cm.duplicates_and_nan()
    got, want = _device_tris(renderer, _cloud(verts))
    np.testing.assert_array_equal(got, want)
    assert len(got) > 250 and not (got == 100).any()


@pytest.mark.parametrize("n_points,n_tris", [(1, 0), (2, 0), (3, 1), (4, 2)])
def test_the_smallest_clouds(renderer, n_points, n_tris):
    verts = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 10, 1]], np.float32)[:n_points]
    got, want = _device_tris(renderer, _cloud(verts))
    np.testing.assert_array_equal(got, want)
    assert len(got) == n_tris


def test_a_files_normals_take_the_place_of_the_estimate(renderer):
    """Scaled and sign-flipped normals, and normals of another direction altogether: whatever the device copy holds is what the
    model is fed; flipping signs alone (and scaling by powers of two) changes no row."""
    face = _face()
    verts = cm.jittered(face.verts, seed=9)
    estimate, _ = _table(renderer, verts)
    plain, want = _device_tris(renderer, _cloud(verts))
    np.testing.assert_array_equal(plain, want)
    rs = np.random.RandomState(5)
    signs = rs.choice([-1.0, 1.0], size=(len(verts), 1)).astype(np.float32)
    pow2 = (2.0 ** rs.randint(-3, 4, size=(len(verts), 1))).astype(np.float32)
    got, want = _device_tris(renderer, _cloud(verts, normals=estimate * signs * pow2), file_normals=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, plain)
    scaled = estimate * signs * rs.uniform(0.3, 3.0, size=(len(verts), 1)).astype(np.float32)
    got, want = _device_tris(renderer, _cloud(verts, normals=scaled), file_normals=True)
    np.testing.assert_array_equal(got, want)
    tilted = estimate + rs.normal(scale=0.2, size=estimate.shape).astype(np.float32)
    tilted[7] = 0.0                                                                   # a point without a normal: an empty star
    tilted[11] = np.nan
    got, want = _device_tris(renderer, _cloud(verts, normals=tilted), file_normals=True)
    np.testing.assert_array_equal(got, want)
    assert not (got == 7).any() and not (got == 11).any() and len(got) > 1000


# ---- 2. past the scan's block size, checked without the model -----------------------------------------------------------------
def test_a_grid_past_a_scan_block(renderer):
    """82 x 50 = 4 100 points, four past a scan block of 4 096, turned by a rotation that leaves every coordinate an exact float32:
    the triangles tile the rectangle."""
    step = 8.125
    verts = cm.exact_tilt(cm.flat_grid(82, 50, step))
    cloud = _cloud(verts)                                                             # (the device copy lives as long as its Mesh)
    handle, table, _, _ = _prepare(renderer, cloud)
    rc, n, tris = _call(renderer, handle, table, 3 * len(verts) + 1024)
    assert rc == 0 and n == 2 * 81 * 49
    tris = tris[:n]
    assert (tris[:, 0] < tris[:, 1]).all() and (tris[:, 1] < tris[:, 2]).all()
    rect = 81 * 49 * step * step
    assert abs(cm.area(verts, tris) - rect) <= 1e-9 * rect
    uses = cm.edge_uses(tris)
    assert uses.max() == 2 and int((uses == 1).sum()) == 2 * (81 + 49)


def test_a_grid_past_a_slice_of_block_sums(renderer):
    """1 025 x 1 024 points: 257 scan blocks, one past the 256 whose sums the top kernel scans at a time.  The rows must come out
    strictly ascending with every slot below the count written - a start that is off by a carry would overlap or leave a gap."""
    nx, ny = 1025, 1024
    x, y = np.meshgrid(np.arange(nx, dtype=np.float32), np.arange(ny, dtype=np.float32))
    verts = np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny, np.float32)], axis=1)
    cloud = _cloud(verts)
    handle, table, _, _ = _prepare(renderer, cloud)
    cap = 2 * nx * ny
    rc, n, tris = _call(renderer, handle, table, cap)
    assert rc == 0 and n == 2 * (nx - 1) * (ny - 1)
    tris = tris[:n].astype(np.int64)
    assert tris.min() >= 0 and tris.max() < nx * ny
    assert (tris[:, 0] < tris[:, 1]).all() and (tris[:, 1] < tris[:, 2]).all()
    key = (tris[:, 0] << 42) | (tris[:, 1] << 21) | tris[:, 2]
    assert (key[1:] > key[:-1]).all()
    x = np.cross(verts[tris[:, 1]].astype(np.float64) - verts[tris[:, 0]], verts[tris[:, 2]].astype(np.float64) - verts[tris[:, 0]])
    assert (np.abs(x[:, 2]) == 1.0).all()                                             # every one half a grid cell


# ---- 3. the count, the cap ----------------------------------------------------------------------------------------------------
def test_count_only_and_a_cap_that_is_too_small(renderer):
    face = _face()
    cloud = _cloud(cm.jittered(face.verts, seed=2))
    handle, table, normals, table_host = _prepare(renderer, cloud)
    want = cm.triangulate(cloud.verts, normals, table_host)
    rc, n, full = _call(renderer, handle, table, len(want) + 10)
    assert rc == 0 and n == len(want)
    np.testing.assert_array_equal(full[:n], want)
    assert (full[n:] == UNWRITTEN).all()
    rc, n, none = _call(renderer, handle, table, 0, rows=len(want) + 10, with_tris=False)     # tris_dev == NULL: only the count
    assert rc == 0 and n == len(want)
    rc, n, none = _call(renderer, handle, table, 0, rows=len(want) + 10)                      # cap 0: no row
    assert rc == 0 and n == len(want) and (none == UNWRITTEN).all()
    for cap in (1, 100, len(want) - 1, len(want)):
        rc, n, part = _call(renderer, handle, table, cap, rows=len(want) + 10)
        assert rc == 0 and n == len(want)                                                      # always the full count
        np.testing.assert_array_equal(part[:cap], want[:cap])
        assert (part[cap:] == UNWRITTEN).all()                                                 # nothing beyond the cap


def test_two_runs_give_the_same_bytes(renderer):
    face = _face()
    verts = cm.jittered(face.verts, seed=3)
    first, _ = _device_tris(renderer, _cloud(verts))
    second, _ = _device_tris(renderer, _cloud(verts))
    assert first.tobytes() == second.tobytes()


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_context_usable(renderer):
    import torch

    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.render3d import upload_mesh

    r = renderer
    lib, h = r.ctx.lib, r.ctx.handle
    face = _face(12)
    cloud = _cloud(face.verts, face.colors)
    before = _render(r, cloud)
    handle, table, _, _ = _prepare(r, cloud)
    bare = _cloud(face.verts, face.colors)
    bare_handle = upload_mesh(r.ctx, bare)                                             # a cloud without normals
    tri_mesh = Mesh(face.verts, face.tris)
    tri_handle = upload_mesh(r.ctx, tri_mesh)
    dev = torch.device("cuda", r.ctx.device)

    def refused(rc_n_tris, what):
        rc, n, tris = rc_n_tris
        msg = lib.mvlm_last_error(h).decode()
        assert rc != 0 and msg.startswith("triangulate points:") and what in msg, msg
        assert n == UNWRITTEN and (tris == UNWRITTEN).all()                            # nothing was launched
        np.testing.assert_array_equal(_render(r, cloud), before)                       # ... and the context renders on

    refused(_call(r, tri_handle, table, 100), "has triangles")
    refused(_call(r, bare_handle, table, 100), "no normals")
    refused(_call(r, handle, None, 100), "null")
    refused(_call(r, handle, table, -1, rows=100), "negative cap")
    tris = torch.full((100, 3), UNWRITTEN, dtype=torch.int32, device=dev)
    assert lib.mvlm_mesh_triangulate_points(h, handle, C.c_void_p(table.data_ptr()), C.c_void_p(tris.data_ptr()), C.c_longlong(100), None) != 0
    assert lib.mvlm_last_error(h).decode().startswith("triangulate points:")
    torch.cuda.synchronize()
    assert (tris.cpu().numpy() == UNWRITTEN).all()
    # a call that works changes nothing about the cloud's render either (the device copy, the key plane)
    rc, n, _ = _call(r, handle, table, 4 * cloud.n_verts)
    assert rc == 0 and n > 200
    np.testing.assert_array_equal(_render(r, cloud), before)
    with pytest.raises(ValueError, match="has triangles"):
        r.triangulate_point_cloud(Mesh(face.verts, face.tris))


# ---- 5. the stage times -------------------------------------------------------------------------------------------------------
def test_stage_times_under_profiling(renderer):
    r = renderer
    lib, h = r.ctx.lib, r.ctx.handle
    face = _face()
    cloud = _cloud(face.verts)
    handle, table, _, _ = _prepare(r, cloud)
    lib.mvlm_render_set_profiling(h, 1)
    try:
        rc, n, _ = _call(r, handle, table, 4 * face.n_verts)
        assert rc == 0 and n > 1000
        ms = r.cloud_mesh_stage_ms()
    finally:
        lib.mvlm_render_set_profiling(h, 0)
    assert ms.shape == (3,) and np.isfinite(ms).all() and (ms >= 0.0).all() and ms.sum() > 0.0


# ---- 6. the Mesh that comes back ----------------------------------------------------------------------------------------------
def test_triangulate_point_cloud_returns_the_documented_mesh(renderer):
    r = renderer
    face = _face()
    verts = cm.jittered(face.verts, seed=8)
    verts[40] = [np.nan, 0.0, 0.0]                                                     # a NaN point and an infinite one
    verts[333] = [0.0, np.inf, 0.0]
    to_original = np.eye(4)
    cloud = _cloud(verts, face.colors)
    cloud.path, cloud.to_original, cloud.point_radius = "scan.ply", to_original, 2.0
    out = r.triangulate_point_cloud(cloud)
    assert r.triangulate_point_cloud(cloud) is out                                     # kept on the cloud object
    finite = np.isfinite(verts).all(axis=1)
    assert finite.sum() == len(verts) - 2
    np.testing.assert_array_equal(out.verts, verts[finite])
    np.testing.assert_array_equal(out.colors, face.colors[finite])
    assert out.point_ids.dtype == np.int32
    np.testing.assert_array_equal(out.point_ids, np.nonzero(finite)[0])
    assert out.path == "scan.ply" and out.to_original is to_original
    assert out.point_radius is None and out.normals is None and out.uvs is None and out.texture is None
    assert out.tris.dtype == np.int32 and out.n_tris > 1000
    # the triangles: the model's on the cloud's own numbering, from the device's table and normals
    handle, table, normals, table_host = _prepare(r, _cloud(verts))
    want = cm.triangulate(verts, normals, table_host)
    np.testing.assert_array_equal(out.point_ids[out.tris], want)
    assert not np.isin(want, [40, 333]).any()
    # with the cloud's own normals: those, not the estimate
    own = normals + np.random.RandomState(1).normal(scale=0.3, size=normals.shape).astype(np.float32)
    with_own = _cloud(verts, face.colors, normals=own)
    out2 = r.triangulate_point_cloud(with_own)
    np.testing.assert_array_equal(with_own.normals, own)
    np.testing.assert_array_equal(out2.point_ids[out2.tris], cm.triangulate(verts, own, table_host))
    # ... and it renders and snaps as a mesh
    img = _render(r, out)
    assert (img[0, :, :, :3] != 1.0).any()
