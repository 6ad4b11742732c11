"""The landmark report without a GPU: the numpy model of tests/report_model.py is pinned to the reference's recorded consensus
results (the six ``fuse_*`` cases of tests/golden/estimator.npz) before tests/test_gpu_report.py lets it judge the kernels;
``LandmarkReport``'s CSV form, its texel convention and the command line's ``--report`` flag."""
import numpy as np
import pytest

import report_model as rm
from mvlm_amd.utils.report import CSV_HEADER, LandmarkReport, ReportLayout, texel


@pytest.fixture(scope="module")
def fixture_reports(golden):
    g = golden("estimator.npz")
    out = {}
    for tag in rm.FIXTURE_TAGS:
        scores, starts, ends, masks, draws, draw_k = rm.fixture_case(g, tag)
        out[tag] = (rm.consensus_report(starts, ends, masks, draws), draw_k, masks)
    return g, out


@pytest.mark.parametrize("tag", rm.FIXTURE_TAGS)
def test_the_model_reproduces_the_reference(fixture_reports, tag):
    g, reports = fixture_reports
    r, draw_k, masks = reports[tag]
    np.testing.assert_array_equal(r["point"], g[f"fuse_{tag}_out"])      # exactly: max |diff| 0
    np.testing.assert_array_equal(draw_k, g[f"fuse_{tag}_draw_k"])       # the recorded draws belong to these landmarks
    err = 0
    for e in r["error"][r["k"] >= 3]:   # the reference's left-to-right sum (estimator3d.py:180-183)
        err = err + e
    assert err / len(r["error"]) == float(g[f"fuse_{tag}_err"])


def test_what_the_fixtures_cover(fixture_reports):
    """The figures the kernel tests lean on: every branch occurs, the survivor counts, and the distance of every surviving
    line from the inlier threshold - which is why inlier flags can be compared exactly, nothing excluded."""
    _, reports = fixture_reports
    branch = np.concatenate([r["branch"] for r, _, _ in reports.values()])
    assert [int((branch == b).sum()) for b in (0, 1, 2)] == [6, 274, 244]
    ks = set(np.concatenate([r["k"] for r, _, _ in reports.values()]).tolist())
    rest = ks - {0, 2, 3, 4, 32, 64}
    assert ks >= {0, 2, 3, 4, 32, 64} and min(rest) == 45 and max(rest) == 54
    assert min(r["gap"].min() for r, _, _ in reports.values()) > 0.0083
    assert np.nanmax(np.concatenate([r["cond"][r["n_used"] >= 3] for r, _, _ in reports.values()])) <= 15
    for r, _, masks in reports.values():
        kept = (r["flags"] & rm.KEPT) != 0
        np.testing.assert_array_equal(kept, masks)
        assert not ((r["flags"] & (rm.DRAWN | rm.INLIER | rm.USED)) != 0)[~kept].any()   # only surviving views carry more bits
        np.testing.assert_array_equal(((r["flags"] & rm.USED) != 0).sum(1), r["n_used"])
        np.testing.assert_array_equal(((r["flags"] & rm.INLIER) != 0).sum(1), r["n_inliers"])


def _report(nl=5, n=4, seed=0):
    rs = np.random.RandomState(seed)
    layout = ReportLayout(nl, n)
    a = layout.host_arrays(np.zeros(layout.nbytes, np.uint8))
    for k in ("raw", "error", "stats", "snapped", "bary", "uv", "view_dist2"):
        a[k][...] = rs.uniform(-50, 50, size=a[k].shape)
    a["stats"][:, 3:6] = np.abs(a["stats"][:, 3:6]) + 200   # a diagonally dominant, i.e. positive definite, covariance
    a["counts"][...] = rs.randint(0, 9, size=a["counts"].shape)
    a["tri"][...] = rs.randint(0, 1000, size=nl)
    a["stats"][1, :] = np.nan
    a["tri"][2], a["bary"][2], a["uv"][2] = -1, np.nan, np.nan
    return LandmarkReport(a, landmarks=a["snapped"] + 7.0)


def test_the_layout_is_one_aligned_byte_range():
    layout = ReportLayout(73, 13)
    end = 0
    for name, (off, nb, dt, shape) in layout.fields.items():
        assert off == end and off % dt.itemsize == 0 and nb == int(np.prod(shape)) * dt.itemsize
        end = off + nb
    assert end <= layout.nbytes < end + 8 and layout.nbytes % 8 == 0


def test_csv_round_trip(tmp_path):
    rep = _report()
    path = rep.to_csv(tmp_path / "scan_dtu3d_report.csv")
    lines = path.read_text().splitlines()
    assert lines[0] == CSV_HEADER == "index,x,y,z,n_kept,n_inliers,n_used,branch,error,rms,sigma,snap_dist,tri,b0,b1,b2,u,v"
    assert len(lines) == 1 + len(rep)
    back = np.genfromtxt(path, delimiter=",", names=True)
    np.testing.assert_array_equal(back["index"], np.arange(len(rep)))
    np.testing.assert_array_equal(np.stack([back["x"], back["y"], back["z"]], 1), rep.landmarks)   # 17 digits: exact
    for name, want in (("n_kept", rep.n_kept), ("n_inliers", rep.n_inliers), ("n_used", rep.n_used), ("branch", rep.branch),
                       ("error", rep.error), ("rms", rep.rms), ("sigma", rep.sigma), ("snap_dist", rep.snap_dist), ("tri", rep.tri),
                       ("b0", rep.bary[:, 0]), ("b1", rep.bary[:, 1]), ("b2", rep.bary[:, 2]), ("u", rep.uv[:, 0]), ("v", rep.uv[:, 1])):
        np.testing.assert_array_equal(back[name], np.asarray(want, np.float64), err_msg=name)     # (NaN == NaN here)
    assert np.isnan(rep.sigma[1]) and np.isfinite(rep.sigma[0]) and lines[3].split(",")[12] == "-1"
    # sigma is the square root of the covariance's largest eigenvalue
    assert rep.sigma[0] == pytest.approx(np.sqrt(np.linalg.eigvalsh(rep.cov[0])[-1]), rel=1e-12)
    np.testing.assert_array_equal(rep.cov, np.transpose(rep.cov, (0, 2, 1)))


def test_texture_pixel_by_hand():
    """rm_texel of raster_math.h: u - floor(u) (GL_REPEAT), column = trunc(u' w), row counted from the TOP of an image
    whose v = 0 is the bottom: row = h - 1 - trunc(v' h).  A 4 x 2 texture, by hand:"""
    cases = [((0.3, 0.2), (1, 1)),      # 1.2 -> column 1; 0.4 -> 0 from the bottom -> row 1
             ((0.999, 0.75), (3, 0)),   # 3.996 -> 3; 1.5 -> 1 from the bottom -> row 0
             ((1.25, -0.25), (1, 0)),   # wraps to (0.25, 0.75)
             ((1.0, 1.0), (0, 1)),      # wraps to (0, 0)
             ((-0.01, 2.5), (3, 0)),    # wraps to (0.99, 0.5): 3.96 -> 3; 1.0 -> 1 -> row 0
             ((np.nan, 0.5), (-1, -1))]
    u, v = np.array([c[0] for c in cases]).T
    tx, ty = texel(u, v, 4, 2)
    assert list(zip(tx.tolist(), ty.tolist())) == [c[1] for c in cases]
    rep = _report()
    rep.uv[:len(cases)] = np.array([c[0] for c in cases])[:len(rep)]
    np.testing.assert_array_equal(rep.texture_pixel(4, 2)[:len(cases)], np.array([c[1] for c in cases])[:len(rep)])
    # float32 arithmetic like the rasteriser's: the largest double below 1 is 1.0f there and wraps to texel 0
    assert texel(np.nextafter(1.0, 0.0), 0.0, 1024, 1024)[0] == 0


def test_report_flag_of_the_command_line():
    from mvlm_amd.__main__ import build_parser

    assert build_parser().parse_args(["-p", "scans", "--report"]).report is True
    assert build_parser().parse_args(["-p", "scans"]).report is False
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-p", "scans", "--report=3"])


def test_the_pipeline_keeps_the_flag_off_by_default():
    import inspect

    from mvlm_amd.pipeline import Pipeline

    assert inspect.signature(Pipeline.__init__).parameters["landmark_report"].default is False
