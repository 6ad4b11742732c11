"""-m gpu: the surface distances between landmarks on the device (geodesic.hip: mvlm_landmark_geodesics) against the numpy statement
of the rule (tests/geodesic_model.py) BIT FOR BIT: the fields, D, E and the sweep counts.  The model is fed the device's own
attachment (snapped point and triangle, which tests/test_gpu_report.py checks), so what is compared is the distance computation.

Why exact equality holds: the sweep is Jacobi (every read of the previous buffer), a vertex's value is a min - exact and
commutative, so neither scheduling nor the order of a vertex's triangle list reaches it -, both sides follow the operation order
of csrc/geodesic_math.h, nothing is contracted, and float64 + - * / and sqrt are correctly rounded on both sides.

Shapes: the smallest where something can go wrong - one triangle, two, a 9 x 9 grid, sliver triangles, the 642-vertex sphere with 1,
84 and 130 sources (130: a last block of sources that is not full), 257 and 1025 vertices (a vertex chunk plus one), the 2 x 600
strip (about 600 sweeps: several host batches and the convergence read), two components, a pair list, a scratch cap that forces
three source groups, max_sweeps too small, the argument errors."""
import ctypes as C

import numpy as np
import pytest

import geodesic_model as gm

pytestmark = pytest.mark.gpu


def _mesh(verts, tris):
    from mvlm_amd.utils import Mesh

    return Mesh(np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(tris, np.int32).reshape(-1, 3))


@pytest.fixture(scope="module")
def renderer():
    from mvlm_amd.utils import HipRenderer3D

    return HipRenderer3D(n_views=1, verbose=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    """bit for bit, any NaN counting as the one NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype == np.float64:
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
        keep = ~np.isnan(want)
        np.testing.assert_array_equal(_bits(got[keep]), _bits(want[keep]), err_msg=what)
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


def _check(r, verts, tris, points, **kw):
    """one call with the fields -> the result, after comparing everything with the model"""
    res = r.landmark_geodesics(_mesh(verts, tris), points, return_fields=True, **kw)
    model_kw = {k: v for k, v in kw.items() if k in ("init_rings", "pairs", "max_sweeps")}
    D, E, sweeps, fields = gm.geodesics(verts, tris, res.snapped, res.tri, **model_kw)
    _same(res.euclidean, E, "E")
    _same(res.sweeps, sweeps, "sweeps")
    _same(res.fields.cpu().numpy(), fields, "fields")
    _same(res.directed, D, "D")
    return res


def _sphere():
    if not hasattr(_sphere, "mesh"):
        _sphere.mesh = gm.icosphere(3)
    return _sphere.mesh


def test_single_triangle(renderer):
    verts = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32)
    tris = np.array([[0, 1, 2]], np.int32)
    pts = np.array([[1.0, 1.0, 0.5], [2.0, 0.5, -1.0], [0.25, 2.0, 0.0]])
    res = _check(renderer, verts, tris, pts)
    assert (res.tri == 0).all()
    # both in one triangle: the straight distance itself
    _same(res.directed[0, 1:], res.euclidean[0, 1:], "same triangle")
    assert (np.diag(res.directed) == 0).all()


def test_two_triangles(renderer):
    verts, tris = gm.grid(2, 2)
    pts, _ = gm.plant(verts, tris, [0, 1], [[0.2, 0.5, 0.3], [0.3, 0.3, 0.4]])
    res = _check(renderer, verts, tris, pts)
    assert sorted(res.tri.tolist()) == [0, 1] and np.isfinite(res.directed).all()


@pytest.mark.parametrize("rings", [0, 2, 8])
def test_grid_9x9(renderer, rings):
    verts, tris = gm.grid(9, 9)
    pts, _ = gm.spread(verts, tris, 7, seed=1)
    res = _check(renderer, verts, tris, pts, init_rings=rings)
    assert np.isfinite(res.directed).all()


def test_sliver_grid(renderer):
    verts, tris = gm.grid(9, 17, 1.0, 0.125, jitter=0.2, seed=4)
    pts, _ = gm.spread(verts, tris, 9, seed=2)
    _check(renderer, verts, tris, pts)


@pytest.mark.parametrize("n", [1, 84, 130])
def test_sphere(renderer, n):
    verts, tris = _sphere()
    assert verts.shape[0] == 642
    pts, _ = gm.spread(verts, tris, n, seed=n)
    res = _check(renderer, verts, tris, pts * 1.01)  # (a little off the surface: the attachment brings them back)
    assert np.isfinite(res.directed).all() and (res.sweeps > 0).all()


@pytest.mark.parametrize("nx,ny,drop", [(129, 2, 1), (41, 25, 0)])
def test_a_vertex_chunk_plus_one(renderer, nx, ny, drop):
    """257 and 1025 vertices: the last workgroup of a sweep holds one vertex"""
    verts, tris = gm.grid(nx, ny)
    if drop:  # (2 x 129 without its last vertex and that vertex's triangles)
        verts = verts[:-drop]
        tris = tris[(tris < verts.shape[0]).all(axis=1)]
    assert verts.shape[0] % 256 == 1
    pts, _ = gm.spread(verts, tris, 5, seed=5)
    _check(renderer, verts, tris, pts)


def test_strip_needs_several_batches(renderer):
    verts, tris = gm.strip(600)
    pts, _ = gm.plant(verts, tris, [0, 300, len(tris) - 1], [[0.4, 0.3, 0.3]] * 3)
    res = _check(renderer, verts, tris, pts)
    assert res.sweeps.max() > 400  # (32 sweeps a batch: more than a dozen reads of the settled flags)


def test_two_components(renderer):
    verts, tris = gm.two_components()
    half = len(tris) // 2
    pts, _ = gm.plant(verts, tris, [3, 11, half + 2, half + 20], [[0.3, 0.3, 0.4]] * 4)
    res = _check(renderer, verts, tris, pts)
    assert np.isinf(res.directed[:2, 2:]).all() and np.isinf(res.directed[2:, :2]).all()
    assert np.isfinite(res.directed[:2, :2]).all() and (res.sweeps >= 0).all()


def test_nan_vertex_unattached_landmark_and_repeated_index(renderer):
    verts, tris = gm.grid(7, 7)
    verts = verts.copy()
    verts[24] = np.nan  # the middle vertex: its six triangles are ignored
    tris = np.concatenate([tris, [[0, 0, 1]]]).astype(np.int32)  # a triangle with a repeated index
    pts, _ = gm.plant(verts, tris, [0, 70, 35], [[0.3, 0.3, 0.4]] * 3)
    pts = np.concatenate([pts, [[np.nan, 0.0, 0.0]]])  # a landmark that is nowhere
    res = _check(renderer, verts, tris, pts)
    assert res.tri[3] == -1 and np.isnan(res.directed[3]).all() and np.isnan(res.directed[:, 3]).all() and res.sweeps[3] == -1
    assert np.isfinite(res.directed[:3, :3]).all()
    assert np.isinf(res.fields[0, 24].item())


def test_pairs_leave_sources_out(renderer):
    verts, tris = _sphere()
    pts, _ = gm.spread(verts, tris, 12, seed=7)
    pairs = [(0, 5), (5, 9), (11, 2)]
    res = _check(renderer, verts, tris, pts, pairs=pairs)
    asked = np.zeros((12, 12), bool)
    for i, j in pairs:
        asked[i, j] = asked[j, i] = True
    assert np.isfinite(res.directed[asked]).all() and np.isnan(res.directed[~asked]).all()
    assert (res.sweeps[[0, 2, 5, 9, 11]] > 0).all() and (res.sweeps[[1, 3, 4, 6, 7, 8, 10]] == -1).all()
    full = renderer.landmark_geodesics(_mesh(verts, tris), pts)
    _same(res.directed[asked], full.directed[asked], "pairs against all")
    assert len(res.rows()) == 3 and res.rows()[0][:2] == (0, 5) and res.rows()[1][:2] == (2, 11)


def test_scratch_cap_forces_three_groups(renderer):
    verts, tris = _sphere()
    V, n = verts.shape[0], 10
    pts, _ = gm.spread(verts, tris, n, seed=8)
    one = _check(renderer, verts, tris, pts)
    renderer.release_geodesics()
    assert renderer.scratch_bytes("geodesic") == 0
    cap = 16 * V * 4 * 5 // 4 + 256 + 16  # four sources' two buffers with the scratch's headroom: groups of 4, 4, 2
    three = _check(renderer, verts, tris, pts, max_scratch_bytes=cap)
    assert 0 < renderer.scratch_bytes("geodesic.field") <= cap
    _same(three.directed, one.directed, "three groups against one")
    _same(three.fields.cpu().numpy(), one.fields.cpu().numpy(), "fields")
    with pytest.raises(ValueError, match="geodesics: max_scratch_bytes"):
        renderer.landmark_geodesics(_mesh(verts, tris), pts, max_scratch_bytes=1000)


def test_max_sweeps_too_small_is_an_error(renderer):
    verts, tris = gm.strip(100)
    pts, _ = gm.plant(verts, tris, [0, len(tris) - 1], [[0.4, 0.3, 0.3]] * 2)
    with pytest.raises(gm.NotSettled):
        gm.geodesics(verts, tris, pts, [0, len(tris) - 1], max_sweeps=40)
    with pytest.raises(ValueError, match=r"geodesics: source landmark \d+ did not settle"):
        renderer.landmark_geodesics(_mesh(verts, tris), pts, max_sweeps=40)
    res = _check(renderer, verts, tris, pts, max_sweeps=int(gm.geodesics(verts, tris, pts, [0, len(tris) - 1])[2].max()) + 1)
    assert np.isfinite(res.directed).all()


def test_stage_times_and_release(renderer):
    verts, tris = gm.grid(9, 9)
    pts, _ = gm.spread(verts, tris, 4, seed=3)
    lib, handle = renderer.ctx.lib, renderer.ctx.handle
    renderer.ctx.check(lib.mvlm_render_set_profiling(handle, 1))
    try:
        renderer.landmark_geodesics(_mesh(verts, tris), pts)
        ms = renderer.geodesic_stage_ms()
    finally:
        renderer.ctx.check(lib.mvlm_render_set_profiling(handle, 0))
    assert ms.shape == (4,) and (ms >= 0).all() and ms.sum() > 0
    assert renderer.scratch_bytes("geodesic") > 0
    renderer.release_geodesics()
    assert renderer.scratch_bytes("geodesic") == 0


def test_argument_errors_launch_nothing(renderer):
    import torch

    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.render3d import upload_mesh

    ctx = renderer.ctx
    dev = torch.device("cuda", ctx.device)
    verts, tris = gm.grid(5, 5)
    mesh = _mesh(verts, tris)
    cloud = Mesh(verts, np.zeros((0, 3), np.int32))
    n, V = 3, verts.shape[0]
    pts = torch.from_numpy(gm.spread(verts, tris, n, seed=1)[0]).to(dev)
    out = {"snapped": torch.full((n, 3), -7.0, dtype=torch.float64, device=dev), "tri": torch.full((n,), -7, dtype=torch.int32, device=dev),
           "D": torch.full((n, n), -7.0, dtype=torch.float64, device=dev), "E": torch.full((n, n), -7.0, dtype=torch.float64, device=dev),
           "sweeps": torch.full((n,), -7, dtype=torch.int32, device=dev)}
    ctx.bind_current_stream(torch, dev)
    handles = {"mesh": upload_mesh(ctx, mesh), "cloud": upload_mesh(ctx, cloud)}
    bad_pairs = np.array([[0, 3]], np.int32)

    def call(which="mesh", p=None, count=n, rings=2, sweeps=0, cap=0, pairs=None, **ptr):
        a = {k: v.data_ptr() for k, v in out.items()}
        a["pts"] = pts.data_ptr() if p is None else p
        a.update(ptr)
        return ctx.lib.mvlm_landmark_geodesics(
            ctx.handle, handles[which], C.c_void_p(a["pts"]), count, rings, sweeps, C.c_longlong(cap),
            pairs.ctypes.data_as(C.POINTER(C.c_int32)) if pairs is not None else None, 0 if pairs is None else len(pairs),
            C.c_void_p(a["snapped"]), C.c_void_p(a["tri"]), C.c_void_p(a["D"]), C.c_void_p(a["E"]), C.c_void_p(a["sweeps"]), None)

    cases = {"point cloud": dict(which="cloud"), "null pointer": dict(D=0), "null points": dict(p=0), "aligned": dict(E=out["E"].data_ptr() + 4),
             "4-byte": dict(tri=out["tri"].data_ptr() + 2), "landmarks per call": dict(count=0), "65536": dict(count=65537),
             "init_rings": dict(rings=9), "init_rings must": dict(rings=-1), "max_sweeps": dict(sweeps=-1), "max_scratch_bytes": dict(cap=-1),
             "pair index": dict(pairs=bad_pairs)}
    for text, kw in cases.items():
        assert call(**kw) != 0, text
        msg = ctx.lib.mvlm_last_error(ctx.handle).decode()
        assert msg.startswith("geodesics:") and (text in msg or text in ("null points", "65536", "init_rings must")), (text, msg)
    torch.cuda.synchronize()
    for name, t in out.items():
        assert (t == -7).all(), name  # nothing was launched
    with pytest.raises(ValueError, match="point cloud"):
        renderer.landmark_geodesics(cloud, pts)
    for kw in (dict(init_rings=9), dict(init_rings=True), dict(max_sweeps=0), dict(pairs=[(0, 0)]), dict(pairs=[(0, 3)]), dict(pairs=[])):
        with pytest.raises(ValueError, match="landmark_geodesics"):
            renderer.landmark_geodesics(mesh, pts, **kw)
    assert call() == 0  # and the same arguments, all good, run
    torch.cuda.synchronize()
    assert (out["sweeps"] >= 0).all() and (torch.diagonal(out["D"]) == 0).all()
