"""-m gpu: the opt-in landmark report.  mvlm_consensus_report against mvlm_consensus_solve (bit for bit) and against the numpy
model of tests/report_model.py (which tests/test_report_cpu.py pins to the reference's recorded results), mvlm_surface_attach
against mvlm_project_to_surface (bit for bit) and the model, and ``Pipeline(..., landmark_report=True)`` through every layer."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import report_model as rm

pytestmark = pytest.mark.gpu

P = C.c_void_p


def _ptr(t):
    return P(t.data_ptr())


@pytest.fixture(scope="module")
def e3():
    from mvlm_amd.utils import HipEstimator3D

    return HipEstimator3D(verbose=False)


def _solve_and_report(e3, starts, ends, masks, draws):
    """The same device inputs through mvlm_consensus_solve and mvlm_consensus_report -> (solve point, solve error, report arrays)."""
    from mvlm_amd.utils.report import ReportLayout

    dev = torch.device("cuda", 0)
    nl, n = masks.shape
    s = torch.from_numpy(np.ascontiguousarray(starts)).to(dev)
    e = torch.from_numpy(np.ascontiguousarray(ends)).to(dev)
    m = torch.from_numpy(masks.astype(np.uint8)).to(dev)
    d = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.int32)).to(dev)
    count = torch.from_numpy(masks.sum(1).astype(np.int32)).to(dev)
    out = torch.full((nl, 3), -7.0, dtype=torch.float64, device=dev)
    err = torch.full((nl,), -7.0, dtype=torch.float64, device=dev)
    e3._torch()
    e3.ctx.check(e3.ctx.lib.mvlm_consensus_solve(e3.ctx.handle, _ptr(s), _ptr(e), _ptr(m), _ptr(count), _ptr(d), n, nl, _ptr(out), _ptr(err)))
    layout = ReportLayout(nl, n)
    buf = torch.full((layout.nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    e3.report_device(s, e, m, d, views=layout.device_views(buf))
    return out.cpu().numpy(), err.cpu().numpy(), layout.host_arrays(buf.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_against_model(got, want, label):
    from mvlm_amd.utils.report import LandmarkReport

    rep = LandmarkReport({**got, "snapped": got["raw"]})
    for name, mine in (("k", rep.n_kept), ("n_inliers", rep.n_inliers), ("n_used", rep.n_used), ("branch", rep.branch),
                       ("flags", rep.view_flags)):
        np.testing.assert_array_equal(mine, want[name], err_msg=f"{label}: {name}")     # exactly, nothing excluded
    for name, mine in (("dist2", rep.view_dist2), ("rms", rep.rms), ("max_dist", rep.max_dist), ("sigma2", rep.sigma2)):
        w = want[name]
        np.testing.assert_array_equal(np.isnan(mine), np.isnan(w), err_msg=f"{label}: NaN positions of {name}")
        tol = 1e-9 * np.maximum(1.0, np.abs(w))
        bad = np.abs(mine - w) > tol
        assert not bad[~np.isnan(w)].any(), (label, name, float(np.nanmax(np.abs(mine - w) / np.maximum(1.0, np.abs(w)))))
    np.testing.assert_array_equal(np.isnan(rep.cov), np.isnan(want["cov"]), err_msg=f"{label}: NaN positions of cov")
    for lm in range(len(rep)):
        w = want["cov"][lm]
        if not np.isnan(w).any():
            assert np.abs(rep.cov[lm] - w).max() <= 1e-9 * np.abs(w).max(), (label, lm, rep.cov[lm], w)


# ---- the consensus report ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", rm.FIXTURE_TAGS)
def test_report_on_the_reference_cases(golden, e3, tag):
    g = golden("estimator.npz")
    scores, starts, ends, masks, draws, _ = rm.fixture_case(g, tag)
    want = rm.consensus_report(starts, ends, masks, draws)
    assert want["gap"].min() > 0.0083     # no surviving line near the inlier threshold: flags compare exactly
    point, err, got = _solve_and_report(e3, starts, ends, masks, draws)
    np.testing.assert_array_equal(_bits(got["raw"]), _bits(point))     # bit-equal to mvlm_consensus_solve
    np.testing.assert_array_equal(_bits(got["error"]), _bits(err))
    diff = np.abs(got["raw"] - g[f"fuse_{tag}_out"]).max()
    print(f"{tag}: max |point - fuse_out| = {diff:.3g}")
    assert diff <= 1e-9
    _check_against_model(got, want, tag)


# seeds of report_model.synthetic_rays whose every sample-fit distance stays 1e-3 away from the threshold (asserted below)
SYNTHETIC = [(nl, n, 100 * nl + n + 1000 * (0 if (nl, n) == (1, 3) else 2)) for nl in (1, 73) for n in (1, 2, 3, 65, 1024)]


@pytest.mark.parametrize("nl,n,seed", SYNTHETIC)
def test_report_on_synthetic_rays(e3, nl, n, seed):
    starts, ends, masks, draws = rm.synthetic_rays(nl, n, seed)
    want = rm.consensus_report(starts, ends, masks, draws)
    assert want["gap"].min() >= 1e-3, want["gap"].min()
    if nl > 2:
        assert want["k"][1] == 0 and want["k"][2] == 1      # a landmark whose mask is all zero, one with a single line
    if nl > 2 and n >= 65:
        assert all((want["branch"] == b).any() for b in (0, 1, 2))
    point, err, got = _solve_and_report(e3, starts, ends, masks, draws)
    np.testing.assert_array_equal(_bits(got["raw"]), _bits(point))
    np.testing.assert_array_equal(_bits(got["error"]), _bits(err))
    _check_against_model(got, want, f"nl {nl} n {n}")


def test_report_of_three_parallel_lines(e3):
    """Three lines along exactly (0, 0, 1): A = diag(3, 3, 0) in both arithmetics, the pseudo-inverse drops the z direction -
    the covariance has a zero zz row and column."""
    xy = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 8.0]])
    starts = np.concatenate([xy, np.full((3, 1), 500.0)], 1)[None]
    ends = np.concatenate([xy, np.full((3, 1), -500.0)], 1)[None]
    masks, draws = np.ones((1, 3), bool), np.array([[0, 1, 2, 0, 1, 2, 0, 1]])
    want = rm.consensus_report(starts, ends, masks, draws)
    assert want["n_used"][0] == 3 and np.isfinite(want["sigma2"][0]) and want["sigma2"][0] > 0
    point, err, got = _solve_and_report(e3, starts, ends, masks, draws)
    np.testing.assert_array_equal(_bits(got["raw"]), _bits(point))
    _check_against_model(got, want, "parallel")
    from mvlm_amd.utils.report import LandmarkReport

    cov = LandmarkReport({**got, "snapped": got["raw"]}).cov[0]
    assert (cov[2, :] == 0).all() and (cov[:, 2] == 0).all() and cov[0, 0] > 0 and cov[1, 1] > 0
    np.testing.assert_allclose(cov, want["cov"][0], rtol=0, atol=1e-9 * np.abs(want["cov"][0]).max())


# ---- the surface attachment ------------------------------------------------------------------------------------------------
def _grid(nx, ny, seed=0, size=100.0):
    """A bumpy height field of 2 nx ny triangles with texture coordinates."""
    rs = np.random.RandomState(seed)
    x, y = np.meshgrid(np.linspace(-size, size, nx + 1), np.linspace(-size, size, ny + 1), indexing="ij")
    z = 10.0 * np.sin(x / 17.0) * np.cos(y / 23.0) + rs.uniform(-1, 1, x.shape)
    verts = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)
    uvs = rs.uniform(0, 1, (len(verts), 2)).astype(np.float32)
    return verts, tris, uvs


def _attach_and_check(e3, verts, tris, uvs, pts, label):
    from mvlm_amd.utils import Mesh

    dev = torch.device("cuda", 0)
    mesh = Mesh(verts, tris, uvs=uvs)
    p = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)
    snap = e3.project_device(mesh, p).cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in e3.attach_device(mesh, p).items()}
    np.testing.assert_array_equal(_bits(got["snapped"]), _bits(snap), err_msg=label)     # bit-equal to mvlm_project_to_surface
    wsnap, wtri, wbary, wuv = rm.attach(verts, tris, uvs, np.asarray(pts, dtype=np.float64))
    np.testing.assert_array_equal(got["tri"], wtri, err_msg=label)                         # exact, lowest id on ties
    np.testing.assert_array_equal(np.isnan(got["bary"]), np.isnan(wbary), err_msg=label)
    np.testing.assert_array_equal(np.isnan(got["uv"]), np.isnan(wuv), err_msg=label)
    ok = wtri >= 0
    assert np.abs(got["bary"][ok] - wbary[ok]).max(initial=0) <= 1e-9, label
    assert (got["bary"][ok] >= 0).all() and np.abs(got["bary"][ok].sum(1) - 1).max(initial=0) <= 1e-12, label
    v = verts.astype(np.float64)
    recon = np.einsum("ij,ijk->ik", got["bary"][ok], v[tris[got["tri"][ok]]])
    assert np.abs(recon - got["snapped"][ok]).max(initial=0) <= 1e-9, label
    if uvs is not None:
        assert np.abs(got["uv"][ok] - wuv[ok]).max(initial=0) <= 1e-9, label
    else:
        assert np.isnan(got["uv"]).all(), label
    assert np.isnan(got["bary"][~ok]).all() and np.isnan(got["uv"][~ok]).all()
    np.testing.assert_array_equal(_bits(got["snapped"][~ok]), _bits(np.asarray(pts, dtype=np.float64)[~ok]))   # passed through
    return got


def test_attach_in_all_seven_regions_of_one_triangle(e3):
    verts = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.float32)
    tris = np.array([[0, 1, 2]], np.int32)
    uvs = np.array([[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]], np.float32)
    pts = np.array([[-3, -2, 1], [14, -1, 2], [-1, 13, -1],      # the three vertex regions
                    [4, -5, 1], [-6, 3, 2], [8, 9, -3],          # the three edge regions: ab, ac, bc
                    [2, 3, 7], [np.nan, 1, 1]], np.float64)      # the face; a landmark without a finite distance
    got = _attach_and_check(e3, verts, tris, uvs, pts, "one triangle")
    zeros = (got["bary"][:7] == 0).sum(1)
    assert zeros.tolist() == [2, 2, 2, 1, 1, 1, 0]
    assert got["tri"].tolist() == [0] * 7 + [-1]
    # ... and without texture coordinates: uv is NaN
    _attach_and_check(e3, verts, tris, None, pts, "one triangle, no uvs")


def test_attach_ties_take_the_lowest_triangle(e3):
    """Two triangles sharing the edge (0,0,0)-(10,0,0), listed so that the one a careless search would prefer comes second; a fan
    of four around a shared vertex.  A landmark straight above the shared edge / vertex is equally far from all of them."""
    verts = np.array([[0, 0, 0], [10, 0, 0], [5, 8, 0], [5, -8, 0]], np.float32)
    tris = np.array([[0, 3, 1], [0, 1, 2]], np.int32)
    got = _attach_and_check(e3, verts, tris, None, np.array([[5.0, 0.0, 3.0], [2.0, 0.0, -1.0]]), "shared edge")
    assert got["tri"].tolist() == [0, 0]
    verts = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [-10, 0, 0], [0, -10, 0]], np.float32)
    tris = np.array([[0, 2, 3], [0, 1, 2], [0, 3, 4], [0, 4, 1]], np.int32)
    got = _attach_and_check(e3, verts, tris, None, np.array([[0.0, 0.0, 4.0]]), "shared vertex")
    assert got["tri"].tolist() == [0]


@pytest.mark.parametrize("nx,ny,n_points", [(25, 20, 5), (16, 32, 5), (70, 72, 1), (70, 72, 8), (70, 72, 9), (70, 72, 84)])
def test_attach_on_grids(e3, nx, ny, n_points):
    """1 000 triangles (one chunk of the snap's first pass), 1 024 + 1 (two), and about 10 000 with point counts around the
    pass's group of 8 landmarks."""
    verts, tris, uvs = _grid(nx, ny, seed=nx)
    if (nx, ny) == (16, 32):
        tris = np.concatenate([tris, tris[:1]])          # 1 025 triangles; the repeated one ties with triangle 0
        assert len(tris) == 1025
    rs = np.random.RandomState(n_points + ny)
    pts = rs.uniform(-110, 110, (n_points, 3)) * np.array([1, 1, 0.2])
    pts[0] = verts[tris[0]].astype(np.float64).mean(0) + [0, 0, 2.0]     # above the (possibly repeated) first triangle
    got = _attach_and_check(e3, verts, tris, uvs, pts, f"grid {nx}x{ny}, {n_points} points")
    assert got["tri"][0] == 0


def test_attach_with_a_degenerate_triangle_and_a_stray_vertex(e3):
    verts, tris, uvs = _grid(6, 6, seed=3)
    tris = np.concatenate([np.array([[5, 5, 20]], np.int32), tris])      # a == b: the segment ac
    stray = np.array([[30.0, 30.0, 40.0]], np.float32)                   # a vertex no triangle uses, nearest the landmark
    verts = np.concatenate([verts, stray])
    uvs = np.concatenate([uvs, np.array([[0.5, 0.5]], np.float32)])
    pts = np.array([[30.0, 30.0, 39.0], [-80.0, 10.0, 5.0], verts[5].astype(np.float64) + [0, 0, 1e-3]])
    got = _attach_and_check(e3, verts, tris, uvs, pts, "degenerate + stray")
    assert (got["tri"] >= 0).all()


def test_report_entries_refuse_bad_arguments(e3):
    """Null pointers and 0 or 1025 views: a status code and a message, and nothing is launched (the outputs keep their fill)."""
    from mvlm_amd import _lib
    from mvlm_amd.utils import Mesh
    from mvlm_amd.utils.render3d import upload_mesh

    dev = torch.device("cuda", 0)
    fresh = _lib.Context(0)
    lib = fresh.lib
    nl, n = 2, 1025      # buffers large enough for every view count asked below
    s = torch.zeros((nl, n, 3), dtype=torch.float64, device=dev)
    m = torch.ones((nl, n), dtype=torch.uint8, device=dev)
    d = torch.zeros((nl, 8), dtype=torch.int32, device=dev)
    out = torch.full((64 + nl * n,), 7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((nl, 4), 7, dtype=torch.int32, device=dev)
    fl = torch.full((nl, n), 7, dtype=torch.uint8, device=dev)
    o = [_ptr(out[:6]), _ptr(out[8:10]), _ptr(out[16:34]), _ptr(cnt), _ptr(out[40:]), _ptr(fl)]
    torch.cuda.synchronize()
    for views in (0, 1025, -1):
        assert lib.mvlm_consensus_report(fresh.handle, _ptr(s), _ptr(s), _ptr(m), _ptr(d), views, nl, *o) != 0
        assert b"1..1024 views" in lib.mvlm_last_error(fresh.handle)
    assert lib.mvlm_consensus_report(fresh.handle, _ptr(s), _ptr(s), _ptr(m), _ptr(d), 8, 0, *o) != 0
    for hole in range(10):
        args = [_ptr(s), _ptr(s), _ptr(m), _ptr(d), *o]
        args[hole] = None
        assert lib.mvlm_consensus_report(fresh.handle, *args[:4], 8, nl, *args[4:]) != 0
        assert b"null pointer" in lib.mvlm_last_error(fresh.handle)
    mesh = Mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    h = upload_mesh(fresh, mesh)
    pts = torch.zeros((nl, 3), dtype=torch.float64, device=dev)
    a = [_ptr(out[:6]), _ptr(cnt), _ptr(out[8:14]), _ptr(out[16:20])]
    assert lib.mvlm_surface_attach(fresh.handle, None, _ptr(pts), nl, *a) != 0 and b"bad arguments" in lib.mvlm_last_error(fresh.handle)
    assert lib.mvlm_surface_attach(fresh.handle, h, None, nl, *a) != 0
    assert lib.mvlm_surface_attach(fresh.handle, h, _ptr(pts), 0, *a) != 0
    for hole in range(4):
        b = list(a)
        b[hole] = None
        assert lib.mvlm_surface_attach(fresh.handle, h, _ptr(pts), nl, *b) != 0
    fresh.synchronize()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (cnt == 7).all() and (fl == 7).all()
    del mesh
    fresh.close()


# ---- through every layer ------------------------------------------------------------------------------------------------
FIELDS = ("landmarks", "raw", "n_kept", "n_inliers", "n_used", "branch", "error", "rms", "max_dist", "sigma2", "cov", "sigma",
          "snap_dist", "tri", "bary", "uv", "scores", "view_dist2", "view_flags", "view_indices")


def _fields(rep):
    return {k: np.array(getattr(rep, k)) for k in FIELDS}


def _same_report(a, b, label):
    for k in FIELDS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label}: {k}")     # (NaN == NaN here)


@pytest.fixture(scope="module")
def face(tmp_path_factory):
    from mvlm_amd.utils.synthetic import write_face_like_obj

    return write_face_like_obj(tmp_path_factory.mktemp("report") / "face.obj", grid=40, tex_size=64, seed=2)


@pytest.fixture(scope="module")
def pipes():
    from mvlm_amd import pipeline

    off = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False)
    on = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False, landmark_report=True)
    return off, on


def test_the_report_changes_nothing_and_is_the_same_on_every_path(face, pipes):
    from mvlm_amd.utils.mesh_io import load_obj

    off, on = pipes
    np.random.seed(4)
    want = off.predict_one_file(face)
    assert off.last_report is None
    np.random.seed(4)
    got = on.predict_one_file(face)
    np.testing.assert_array_equal(_bits(got), _bits(want))                       # bit-equal to the run without the report
    assert on.last_error == off.last_error
    rep = on.last_report
    fused = _fields(rep)
    nl = on.get_lm_count()
    assert len(rep) == nl and rep.scores.shape == (nl, 12) and rep.view_indices.tolist() == list(range(12))
    np.testing.assert_array_equal(rep.landmarks, got)
    assert on.estimator_3d.mean_error(rep.error) == on.last_error
    # seeded random weights peak nowhere in particular: landmarks fall back, each adding 1e8 / NL to last_error (an inlier refit
    # adds less than 100 / NL) - the report names them
    failed = rep.error == 1e8
    assert failed.any() and int(failed.sum()) == int(round(on.last_error * nl / 1e8))
    np.testing.assert_array_equal(rep.branch == 2, failed)
    assert (rep.n_used[failed] == rep.n_kept[failed]).all() and (rep.n_used[rep.branch == 1] == rep.n_inliers[rep.branch == 1]).all()
    np.testing.assert_array_equal(rep.n_kept, (rep.view_flags & 1).sum(1))
    np.testing.assert_array_equal(rep.n_used, ((rep.view_flags & 8) != 0).sum(1))
    np.testing.assert_array_equal(rep.snap_dist, np.sqrt(((rep.snapped - rep.raw) ** 2).sum(1)))
    # the attachment really is where the landmark is: the weights rebuild it from the triangle's corners
    m = load_obj(face)
    recon = np.einsum("ij,ijk->ik", rep.bary, m.verts.astype(np.float64)[m.tris[rep.tri]])
    assert np.abs(recon - got).max() <= 1e-9
    assert np.isfinite(rep.uv).all() and (rep.texture_pixel(64, 64) >= 0).all() and (rep.texture_pixel(64, 64) < 64).all()
    np.random.seed(4)
    slots = on._predict_slots(face)
    np.testing.assert_array_equal(_bits(slots), _bits(want))
    _same_report(_fields(on.last_report), fused, "slot protocol")
    np.random.seed(4)
    (f, lm), = list(on.predict_files([face]))
    np.testing.assert_array_equal(_bits(lm), _bits(want))
    _same_report(_fields(on.last_report), fused, "predict_files")
    assert not on._groupable(2) and off._groupable(2)                            # with the report, scans do not share a pass


def _report_shard_worker(rank, world, port, obj, q):
    import os

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)   # every rank on the test box's one GPU
    from mvlm_amd import pipeline

    pipe = pipeline.create_pipeline("dtu3d", n_views=12, weights="synthetic:5", verbose=False, shard_views=True, landmark_report=True)
    np.random.seed(4 if rank == 0 else 99)
    out = pipe.predict_one_file(obj)
    q.put((rank, (out, _fields(pipe.last_report))))
    dist.destroy_process_group()


def test_sharded_every_rank_has_the_same_report(face, pipes):
    """Two ranks over gloo, 6 of the 12 views each (the pattern of test_gpu_parity.py::test_sharded_views_equal_single_process):
    both leave the same report, which is the single process's."""
    import socket

    import torch.multiprocessing as mp

    _, on = pipes
    np.random.seed(4)
    want = on.predict_one_file(face)
    single = _fields(on.last_report)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_report_shard_worker, args=(r, 2, port, face, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    _same_report(res[1][1], res[0][1], "rank 1 against rank 0")                  # every field, scores included
    for r in range(2):
        np.testing.assert_array_equal(res[r][0], want)
        # against the single process: a rank's pass over 6 views runs other convolution tiles than the pass over 12 (another
        # fp32 summation order), so the heatmap VALUES differ in their last bits while the maxima sit on the same pixels - the
        # scores are compared to fp32 rounding of a 1 024-term sum, everything else exactly
        np.testing.assert_allclose(res[r][1]["scores"], single["scores"], rtol=1e-4, atol=0)
        _same_report({**res[r][1], "scores": single["scores"]}, single, f"rank {r}")


def test_planted_scene_reports_the_branch():
    """The hand-made detector of tests/planted.py: every landmark is refitted on its inliers (branch 1).  The same scene with a
    white texture gives the detector nothing to find.  What that half pins is branch 0 with k = 0: a constant texture ties
    every score, no view is strictly above the median, so no landmark reaches the RANSAC at all and none has error 1e8 - the
    equality of (branch == 2) and (error == 1e8) holds there with both sides empty.  Branch 2 itself is checked on the
    random-weight scan of test_the_report_changes_nothing_and_is_the_same_on_every_path and on the recorded fuse_* cases."""
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils import Mesh
    from test_planted_cpu import planted_scene

    mesh, pts, sd, poses = planted_scene(n_views=48)
    pipe = pipeline_from_config(config.default_config("DTU3D", "RGB", n_views=48), weights=sd, verbose=False, landmark_report=True)
    np.random.seed(1)
    got, err = pipe.predict_mesh_device(mesh, poses)
    rep = pipe.last_report
    assert err < 10.0 and (rep.branch == 1).all()
    assert np.isfinite(rep.snap_dist).all() and np.isfinite(rep.sigma).all()
    assert (rep.n_used == rep.n_inliers).all() and (rep.rms < 10.0).all()      # every used line is an inlier: within 10 units
    np.testing.assert_array_equal(rep.landmarks, got)
    white = Mesh(mesh.verts, mesh.tris, mesh.uvs, np.full_like(mesh.texture, 255))
    np.random.seed(1)
    got, err = pipe.predict_mesh_device(white, poses)
    rep = pipe.last_report
    failed = rep.error == 1e8
    print(f"white views: {int(failed.sum())} of {len(rep)} landmarks fell back; branches {np.bincount(rep.branch, minlength=3).tolist()}")
    np.testing.assert_array_equal(rep.branch == 2, failed)
    assert (rep.branch == 0).all() and (rep.n_kept == 0).all() and (rep.error == 0).all() and np.isnan(rep.rms).all()
    # (measured: a constant texture ties every score, no view is strictly above the median, all 73 landmarks take branch 0
    #  with n_kept 0 and error 0; the random-weight scan of test_the_report_changes_nothing... is where branch 2 occurs)
    assert (rep.n_kept[rep.branch == 0] < 3).all() and (rep.n_kept[rep.branch != 0] >= 3).all()
    assert pipe.estimator_3d.mean_error(rep.error) == err


def test_tied_scores_report_the_repeated_solve(face):
    """Tied scores: fewer views survive than the draws were planned for, ``verify`` repeats draws and solve - and the report
    with them: its n_kept are the real counts.  Two views carry no detection: the report's views are the ten that remain."""
    from mvlm_amd import pipeline
    from mvlm_amd.prediction import PrecomputedPredictor

    rs = np.random.RandomState(3)
    nl, n = 20, 12
    lms = np.empty((nl, n, 3), np.float32)
    lms[:, :, :2] = rs.uniform(60, 200, (nl, n, 2))
    lms[:, :, 2] = 0.25
    lms[1, :7, 2] = 0.75          # 5 of the 10 valid views above the median ... (views 2 and 6 are dropped)
    lms[3, 8:, 2] = 0.75          # ... 4 above
    valid = np.ones(n, bool)
    valid[[2, 6]] = False
    kept = np.nonzero(valid)[0]
    want_k = np.array([int((lms[lm, kept, 2] > np.quantile(lms[lm, kept, 2], 0.5)).sum()) for lm in range(nl)])
    assert want_k[1] == 5 and want_k[3] == 4 and want_k[0] == 0
    dev_lms = torch.from_numpy(lms).cuda()
    reports = {}
    for name, kw in (("fused", {"device_fn": lambda images: (dev_lms, valid)}), ("slots", {"fn": lambda images: (lms, valid)})):
        pipe = pipeline.create_pipeline("dtu3d", n_views=n, weights="synthetic:1", verbose=False, landmark_report=True)
        pipe.predictor_2d = PrecomputedPredictor(nl, **kw)
        plain = pipeline.create_pipeline("dtu3d", n_views=n, weights="synthetic:1", verbose=False)
        plain.predictor_2d = PrecomputedPredictor(nl, **kw)
        np.random.seed(2)
        want = plain.predict_one_file(face)
        np.random.seed(2)
        got = pipe.predict_one_file(face)
        np.testing.assert_array_equal(_bits(got), _bits(want))
        rep = pipe.last_report
        np.testing.assert_array_equal(rep.n_kept, want_k)                         # the real counts, not the planned 5
        np.testing.assert_array_equal(rep.view_indices, kept)
        assert rep.scores.shape == (nl, 10) and rep.view_flags.shape == (nl, 10)
        np.testing.assert_array_equal(rep.scores, lms[:, kept, 2])
        assert rep.branch[0] == 0 and rep.n_used[0] == 0 and np.isnan(rep.rms[0]) and np.isnan(rep.sigma[0])
        assert pipe.estimator_3d.mean_error(rep.error) == pipe.last_error
        reports[name] = _fields(rep)
    _same_report(reports["slots"], reports["fused"], "slot protocol")


def test_pre_align_lengths_stay_in_model_space(tmp_path):
    """A BU_3DFE-depth pipeline with the config's pre-align block on an off-centre, small scan: ``landmarks`` are in the file's
    coordinates (bit-equal to the run without the report), ``raw`` and every length are in the aligned model space."""
    from mvlm_amd import config
    from mvlm_amd.pipeline import pipeline_from_config
    from mvlm_amd.utils.mesh_io import load_obj, write_obj
    from mvlm_amd.utils.prealign import landmarks_to_original_space
    from mvlm_amd.utils.synthetic import face_like_mesh, unaligned_copy

    cfg = config.default_config("BU_3DFE-depth", n_views=8)
    cfg["process_3d"]["write_renderings"] = False
    cfg["pre-align"]["write_pre_aligned"] = False
    raw = unaligned_copy(face_like_mesh(40, 64, 5), cfg["pre-align"])
    path = tmp_path / "scan.obj"
    write_obj(path, raw.verts, raw.tris, raw.uvs, raw.texture)
    plain = pipeline_from_config(cfg, weights="synthetic:9", verbose=False)
    pipe = pipeline_from_config(cfg, weights="synthetic:9", verbose=False, landmark_report=True)
    np.random.seed(4)
    want = plain.predict_one_file(path)
    np.random.seed(4)
    got = pipe.predict_one_file(path)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    rep = pipe.last_report
    np.testing.assert_array_equal(rep.landmarks, got)
    mesh = pipe.renderer_3d.load_mesh(path, load_texture=False)
    assert mesh.to_original is not None
    np.testing.assert_array_equal(landmarks_to_original_space(rep.snapped, mesh.to_original), got)
    file_lo, file_hi = load_obj(path).verts.min(0) - 1e-3, load_obj(path).verts.max(0) + 1e-3
    assert np.all(got >= file_lo) and np.all(got <= file_hi)                      # on the file's surface ...
    lo, hi = mesh.verts.min(0) - 1e-3, mesh.verts.max(0) + 1e-3
    assert np.all(rep.snapped >= lo) and np.all(rep.snapped <= hi)                # ... while the report's points are on the aligned one
    assert not (np.all(rep.snapped >= file_lo) and np.all(rep.snapped <= file_hi))
    scale = float(cfg["pre-align"]["scale"])
    # a length of the report is `scale` times the same length in the file (the block scales the scan by that factor)
    moved_file = np.linalg.norm(got - landmarks_to_original_space(rep.raw, mesh.to_original), axis=1)
    np.testing.assert_allclose(rep.snap_dist, scale * moved_file, rtol=1e-6, atol=1e-9)


def test_command_line_writes_the_report(face, tmp_path):
    from mvlm_amd.__main__ import main
    from mvlm_amd.utils.report import CSV_HEADER

    with contextlib.redirect_stdout(io.StringIO()):
        assert main(["-p", str(face), "-o", str(tmp_path), "--pipelines", "dtu3d", "--weights", "synthetic:5", "-n", "12", "--seed", "4",
                     "--report"]) == 0
    lm = np.loadtxt(tmp_path / "face_dtu3d.txt", delimiter=",")
    lines = (tmp_path / "face_dtu3d_report.csv").read_text().splitlines()
    assert lines[0] == CSV_HEADER and len(lines) == 1 + len(lm) == 1 + 73
    rows = np.genfromtxt(tmp_path / "face_dtu3d_report.csv", delimiter=",", names=True)
    np.testing.assert_allclose(np.stack([rows["x"], rows["y"], rows["z"]], 1), lm, rtol=0, atol=1e-12)
    assert (rows["tri"] >= 0).all() and set(rows["branch"].astype(int)) <= {0, 1, 2}
