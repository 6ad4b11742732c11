"""The ray view without a GPU: the CPU model of its contract (tests/native/ray_view.c) against a float64, closed-form evaluation of
the same capsules - the check that does not rest on the float formulation the contract chose -, the contract's closed forms, and
the host logic (LandmarkReport.ray_colours, the ctypes prototypes, render_ray_view's argument checks).

The float64 reference takes the float32-rounded projected ends (the projection is restated here in numpy float32) and evaluates,
per pixel centre, the 2-D distance to the projected segment (coverage: strictly inside the capsule of radius R) and the nearest
point of the 3-D capsule on the line of sight (depth, camera-facing normal component).  Pixels whose distance to the outline is
at most 1/64 pixel are left out, and so is a pixel whose float64 depth lies within the depth bound of a clip value (0 or 1),
where the clip test itself is a coverage decision - together at most 5 % of the pixels the capsule's outline covers, in every scene.

Measured (this file prints them): largest depth error of the rays 2.83e-08 z-buffer units at k = 1 and 2.98e-08 at k = 50
against 1.51e-08 and 1.49e-08 of the spheres (the bound is 4 x the spheres': 6.05e-08 and 5.94e-08); largest image byte
difference 0 at k = 1 and 1 at k = 50."""
import ctypes as C

import numpy as np
import pytest

import ray_model
import view_model

S = 384
CENTRE = (S / 2 + 0.3, S / 2 - 0.2)
DIRECTION = np.deg2rad(30.0)
LENGTHS = (0.0, 1e-4, 1e-2, 1.0, 40.0, 300.0)
INCLINATIONS = (0.0, 45.0, 89.9)
RADII = (3.0, 8.0)
BAND = 1.0 / 64.0
f32 = np.float32


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("ray_model_cpu")
    view_model.load(d)
    ray_model.load(d)
    return ray_model.render


def _frame(k_target):
    """(frame, k as the contract forms it in float32)"""
    half = f32(S / (2.0 * k_target))
    return (0.0, 0.0, float(half)), f32(S) / (f32(2.0) * half)


def _to_model(X, Y, zv, frame, k):
    """a model-space point (front pose) whose projection lies near window position (X, Y) pixels, at view depth zv"""
    half = frame[2]
    return [X / float(k) - half, Y / float(k) - half, zv]


def _project(p, frame, k):
    """the contract's projection of a model point under the front pose, in float32: (X, Y, z)"""
    half = f32(frame[2])
    xv, yv, zv = f32(p[0]), f32(p[1]), f32(p[2])
    return (xv - f32(0.0) + half) * k, (yv - f32(0.0) + half) * k, (f32(500.0) - zv) / f32(1500.0)


def _pixels():
    j, i = np.mgrid[0:S, 0:S]
    return i + 0.5, j + 0.5


def _sphere_f64(X, Y, z, R, k):
    """-> (covered, distance to the outline, depth, shade) per pixel [j, i], float64"""
    px, py = _pixels()
    d = np.hypot(px - X, py - Y)
    hgt = np.sqrt(np.maximum(R * R - d * d, 0.0))
    return d < R, np.abs(d - R), z - hgt / k / 1500.0, hgt / R


def _capsule_f64(A, B, R, k):
    """the capsule of radius R (pixels) around A -> B, ends as (X, Y, z-buffer value): -> (covered, distance to the outline, depth,
    shade) per pixel [j, i]; depth / shade NaN where nothing is covered.  All float64."""
    px, py = _pixels()
    ax, ay, aw = A[0], A[1], A[2] * 1500.0 * k          # depth in pixels: only here, in float64
    bx, by, bw = B[0], B[1], B[2] * 1500.0 * k
    ux, uy, uw = bx - ax, by - ay, bw - aw
    P2, L2 = ux * ux + uy * uy, ux * ux + uy * uy + uw * uw
    qx, qy = px - ax, py - ay
    tau = np.clip((qx * ux + qy * uy) / P2, 0.0, 1.0) if P2 > 0 else np.zeros_like(px)
    d2d = np.hypot(qx - tau * ux, qy - tau * uy)
    best_w = np.full(px.shape, np.inf)
    best_s = np.full(px.shape, np.nan)
    for ex, ey, ew in ((ax, ay, aw), (bx, by, bw)):     # the caps
        d2 = (px - ex) ** 2 + (py - ey) ** 2
        ok = d2 < R * R
        hgt = np.sqrt(np.maximum(R * R - d2, 0.0))
        w = np.where(ok, ew - hgt, np.inf)
        take = w < best_w
        best_w, best_s = np.where(take, w, best_w), np.where(take, hgt / R, best_s)
    if P2 > 0:                                          # the side: nearest root of |q + s e_w - t u|^2 = R^2, 0 <= t <= 1
        e, cr = qx * ux + qy * uy, qx * uy - qy * ux
        h2 = R * R - cr * cr / P2
        ok = h2 > 0
        hgt = np.sqrt(np.maximum(h2, 0.0))
        s = (uw * e - np.sqrt(L2) * np.sqrt(P2) * hgt) / P2
        t = (e + s * uw) / L2
        ok &= (t >= 0) & (t <= 1)
        w = np.where(ok, aw + s, np.inf)
        shade = (t * uw - s) / R                        # the camera-ward component of (surface - axis point) / R
        take = w < best_w
        best_w, best_s = np.where(take, w, best_w), np.where(take, shade, best_s)
    return d2d < R, np.abs(d2d - R), best_w / (1500.0 * k), best_s


def _compare(name, covered_model, depth_model, byte_model, base, cov64, edge64, z64, shade64, bound):
    """the band rule, then coverage / depth / byte; -> (largest depth error, largest byte difference)"""
    inside = (z64 >= 0.0) & (z64 <= 1.0)
    cov = cov64 & inside
    near_clip = cov64 & ((np.abs(z64) <= bound) | (np.abs(z64 - 1.0) <= bound))
    judged = (edge64 > BAND) & ~near_clip
    n_cov, n_band = int(cov64.sum()), int((cov64 & ~judged).sum())   # everything left out counts against the allowance
    assert n_band <= 0.05 * max(n_cov, 1), (name, n_band, n_cov)
    bad = judged & (covered_model != cov)
    assert not bad.any(), (name, "coverage differs at", np.argwhere(bad)[:5])
    both = judged & cov
    if not both.any():
        return 0.0, 0
    err = float(np.abs(depth_model[both].astype(np.float64) - z64[both]).max())
    want = np.floor(base * np.clip(shade64[both], 0.0, 1.0) + 0.5)
    dbyte = int(np.abs(byte_model[both].astype(np.int64) - want.astype(np.int64)).max())
    return err, dbyte


@pytest.mark.parametrize("k_target", [1.0, 50.0])
def test_the_model_against_a_float64_evaluation_of_the_same_capsules(model, k_target):
    verts, tris = view_model.far_triangle()
    frame, k = _frame(k_target)
    kd = float(k)
    # the yardstick: the model's own spheres against their float64 form, same band rule, same k
    sphere_err = 0.0
    for R in RADII:
        radius = f32(R / kd)
        Rp = float(radius * k)
        centres = [(CENTRE[0], CENTRE[1], 0.0), (100.37, 290.81, 31.7 / kd), (301.5, 77.5, -12.3 / kd)]
        lms = [_to_model(X, Y, zv, frame, k) for X, Y, zv in centres]
        img, _, _, winner, depth = model(verts, tris, None, None, [[0, 0, 0]], S, frame=frame, landmarks=lms, radius=float(radius),
                                         lm_rgb=[[255, 255, 255]] * 3)
        for l, p in enumerate(lms):
            X, Y, z = (float(v) for v in _project(p, frame, k))
            cov64, edge64, z64, shade64 = _sphere_f64(X, Y, z, Rp, kd)
            mine = winner[0][::-1] == -2 - l
            others = (winner[0][::-1] <= -2) & ~mine
            e, _ = _compare(f"sphere {R} {l}", mine | (others & cov64), depth[0][::-1], img[0][::-1][..., 0], 255.0, cov64, edge64, z64,
                            shade64, 1e-6)
            sphere_err = max(sphere_err, e)
    bound = 4.0 * sphere_err
    assert 0.0 < bound < 1e-6, bound
    worst_err, worst_byte = 0.0, 0
    for R in RADII:
        ray_radius = f32(R / kd)
        Rp = float(ray_radius * k)
        for length in LENGTHS:
            for incl in INCLINATIONS:
                name = f"k={k_target} R={R} length={length} inclination={incl}"
                hx, hy = 0.5 * length * np.cos(DIRECTION), 0.5 * length * np.sin(DIRECTION)
                hw = 0.5 * length * np.tan(np.deg2rad(incl)) / kd          # half the extent in view depth, model units
                a = _to_model(CENTRE[0] - hx, CENTRE[1] - hy, hw, frame, k)   # A is the nearer end
                b = _to_model(CENTRE[0] + hx, CENTRE[1] + hy, -hw, frame, k)
                img, _, rcnt, winner, depth = model(verts, tris, None, None, [[0, 0, 0]], S, frame=frame, starts=[a], ends=[b],
                                                    ray_radius=float(ray_radius), ray_rgb=[[255, 255, 255]])
                A = tuple(float(v) for v in _project(a, frame, k))
                B = tuple(float(v) for v in _project(b, frame, k))
                cov64, edge64, z64, shade64 = _capsule_f64(A, B, Rp, kd)
                covered = ray_model.ray_of(winner[0][::-1]) == 0
                err, dbyte = _compare(name, covered, depth[0][::-1], img[0][::-1][..., 0], 255.0, cov64, edge64, z64, shade64, bound)
                worst_err, worst_byte = max(worst_err, err), max(worst_byte, dbyte)
                assert err <= bound, (name, err, bound)
                assert dbyte <= 1, (name, dbyte)
                assert covered.any() or not (cov64 & (z64 >= 0) & (z64 <= 1)).any(), name
    print(f"k = {k_target}: largest ray depth error {worst_err:.3e} z-buffer units (bound {bound:.3e} = 4 x the spheres' "
          f"{sphere_err:.3e}); largest byte difference {worst_byte}")


# ---- closed forms -----------------------------------------------------------------------------------------------------------
def test_a_ray_parallel_to_the_window_has_the_closed_form_depth_and_shade(model):
    verts, tris = view_model.far_triangle()
    unit = (0.0, 0.0, 128.0)   # S = 256: k = 1
    R, y0, zv = 5.0, 20.25, 35.0
    img, _, rcnt, winner, depth = model(verts, tris, None, None, [[0, 0, 0]], 256, frame=unit, starts=[[-80.0, y0, zv]],
                                        ends=[[80.0, y0, zv]], ray_radius=R, ray_rgb=[[255, 255, 255]])
    rays = ray_model.ray_of(winner[0][::-1])
    z_axis = float((f32(500.0) - f32(zv)) / f32(1500.0))
    seen = 0
    for j in range(256):
        d = (j + 0.5) - (y0 + 128.0)
        row = rays[j, 60:200] == 0       # columns well inside the two caps
        if abs(d) >= R:
            assert not row.any()
            continue
        assert row.all()
        h = np.sqrt(R * R - d * d)
        np.testing.assert_allclose(depth[0][::-1][j, 60:200], z_axis - h / 1500.0, rtol=0, atol=6e-8)
        assert (np.abs(img[0][::-1][j, 60:200, 0].astype(int) - int(255.0 * h / R + 0.5)) <= 1).all()
        seen += 1
    assert seen == 10


def test_an_end_on_ray_is_the_sphere_at_its_nearer_end_bit_for_bit(model):
    verts, tris = view_model.quad(0.0)
    unit = (0.0, 0.0, 128.0)
    colour = [[200, 120, 30]]
    for a, b in (([10.0, 20.0, 5.0], [10.0, 20.0, 60.0]), ([-33.3, 7.7, 80.0], [-33.3, 7.7, -200.0]), ([3.0, 4.0, 5.0], [3.0, 4.0, 5.0]),
                 ([10.0, 20.0, 30.0], [10.0 + 1e-4, 20.0, 5.0])):
        near = a if a[2] >= b[2] else b
        kw = dict(colors=view_model.QUAD_COLOURS)
        s_img, s_cnt, _, s_win, s_depth = model(verts, tris, None, None, [[0, 0, 0]], 256, frame=unit, landmarks=[near], radius=4.0,
                                                lm_rgb=colour, **kw)
        r_img, _, r_cnt, r_win, r_depth = model(verts, tris, None, None, [[0, 0, 0]], 256, frame=unit, starts=[a], ends=[b],
                                                ray_radius=4.0, ray_rgb=colour, **kw)
        np.testing.assert_array_equal(r_img, s_img)
        np.testing.assert_array_equal(r_depth, s_depth)
        np.testing.assert_array_equal(r_cnt, s_cnt)
        np.testing.assert_array_equal(ray_model.ray_of(r_win) == 0, s_win == -2)
        assert s_cnt[0, 0] > 30


def test_a_sphere_wins_an_equal_depth_against_a_ray(model):
    """A ray drawn from its caps (end-on, zero-length) whose nearer end is a landmark, with the sphere's radius: every covered pixel
    has the sphere's depth bit for bit; the sphere, drawn later, owns all of them and the ray's count is 0."""
    verts, tris = view_model.quad(0.0)
    unit = (0.0, 0.0, 128.0)
    kw = dict(colors=view_model.QUAD_COLOURS)
    for a, b in (([10.3, 20.6, 5.0], [10.3, 20.6, -40.0]), ([-30.0, 7.5, 6.0], [-30.0, 7.5, 6.0])):
        rays = dict(starts=[a], ends=[b], ray_radius=4.0, ray_rgb=[[250, 10, 10]])
        sph = dict(landmarks=[a], radius=4.0)
        _, _, r_cnt, r_win, r_depth = model(verts, tris, None, None, [[0, 0, 0]], 256, frame=unit, **rays, **kw)
        s_img, s_cnt, _, s_win, s_depth = model(verts, tris, None, None, [[0, 0, 0]], 256, frame=unit, **sph, **kw)
        shared = (ray_model.ray_of(r_win) == 0) & (s_win == -2)
        assert shared.sum() > 30 and shared.sum() == r_cnt[0, 0] == s_cnt[0, 0]
        assert (r_depth[shared] == s_depth[shared]).all()                       # equal depths on every shared pixel
        img, cnt, rcnt, win, depth = model(verts, tris, None, None, [[0, 0, 0]], 256, frame=unit, **rays, **sph, **kw)
        assert (win[shared] == -2).all() and rcnt[0, 0] == 0 and cnt[0, 0] == shared.sum()
        np.testing.assert_array_equal(img, s_img)
        np.testing.assert_array_equal(depth, s_depth)


def test_the_landmark_views_model_is_the_ray_model_without_rays(model):
    sc_v, sc_t = view_model.quad(0.0)
    lm = [[10.0, 10.0, 0.0], [-30.3, 5.2, -2.0], [40.0, -41.0, 2.5]]
    want = view_model.render(sc_v, sc_t, None, None, [[0, 0, 0], [10, -40, 5]], 256, frame=(0.0, 0.0, 128.0), landmarks=lm, radius=5.0,
                             colors=view_model.QUAD_COLOURS)
    got = model(sc_v, sc_t, None, None, [[0, 0, 0], [10, -40, 5]], 256, frame=(0.0, 0.0, 128.0), landmarks=lm, radius=5.0,
                colors=view_model.QUAD_COLOURS)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[3], want[2])


# ---- host logic -------------------------------------------------------------------------------------------------------------
def _report(flags, view_indices):
    from mvlm_amd.utils.report import LandmarkReport

    nl, n = flags.shape
    z = np.zeros
    arrays = dict(raw=z((nl, 3)), error=z(nl), snapped=z((nl, 3)), counts=z((nl, 4), np.int32), stats=z((nl, 9)), tri=z(nl, np.int32),
                  bary=z((nl, 3)), uv=z((nl, 2)), scores=z((nl, n), np.float32), view_dist2=z((nl, n)), view_flags=flags)
    return LandmarkReport(arrays, view_indices=view_indices)


def test_ray_colours_follow_the_view_flags_through_view_indices():
    from mvlm_amd.utils import report as rp

    K, D, I, U = rp.VIEW_KEPT, rp.VIEW_DRAWN, rp.VIEW_INLIER, rp.VIEW_USED
    flags = np.array([[0, K, K | D | I | U, K | U], [K | D, 0, D, K | I | U]], np.uint8)
    r = _report(flags, [0, 2, 5, 7])
    green, orange, grey = (26, 230, 26), (255, 165, 0), (160, 160, 160)
    c = r.ray_colours()
    assert c.shape == (2, 4, 3) and c.dtype == np.uint8
    assert [tuple(x) for x in c[0]] == [grey, orange, green, green]
    assert [tuple(x) for x in c[1]] == [orange, grey, grey, green]
    sub = r.ray_colours([7, 2])                                  # view numbers, not columns
    assert [tuple(x) for x in sub[0]] == [green, orange] and [tuple(x) for x in sub[1]] == [green, grey]
    with pytest.raises(ValueError):
        r.ray_colours([1])                                       # a view the detector dropped
    assert (26, 230, 26) == tuple(int(v * 255.0 + 0.5) for v in (0.1, 0.9, 0.1))


def test_the_prototypes_of_the_ray_view():
    from mvlm_amd import _lib

    res, args = _lib.SIGNATURES["mvlm_render_ray_view"]
    lm_res, lm_args = _lib.SIGNATURES["mvlm_render_landmark_view"]
    assert res is C.c_int and len(args) == 18
    assert args[:10] == lm_args[:10] and args[15:17] == lm_args[10:12]   # what it shares with the landmark view, in place
    assert args[10:15] == [C.c_void_p, C.c_void_p, C.c_int, C.c_float, _lib.c_uint8_p] and args[17] is C.c_void_p
    assert _lib.SIGNATURES["mvlm_ray_view_stage_ms"] == (C.c_int, [C.c_void_p, _lib.c_float_p])
    header = (_lib.REPO / "include" / "mvlm_hip.h").read_text() if hasattr(_lib, "REPO") else None
    if header is not None:
        assert "int mvlm_render_ray_view(" in header and "int mvlm_ray_view_stage_ms(" in header


def test_render_ray_view_checks_its_rays_before_it_needs_a_device():
    from mvlm_amd.utils import HipRenderer3D

    check = HipRenderer3D.ray_view_arguments
    a, b, rr, rgb = check(np.zeros((84, 8, 3)), np.ones((84, 8, 3)), 0.5, np.zeros((672, 3), np.uint8))
    assert a.shape == (672, 3) and b.shape == (672, 3) and a.dtype == np.float64 and rr == 0.5 and rgb.shape == (672, 3)
    assert check(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0, 3)
    for bad in (dict(starts=np.zeros((4, 2)), ends=np.zeros((4, 2))), dict(starts=np.zeros((4, 3)), ends=np.zeros((5, 3))),
                dict(starts=np.zeros((65537, 3)), ends=np.zeros((65537, 3))),
                dict(starts=np.zeros((4, 3)), ends=np.zeros((4, 3)), ray_radius=-1.0),
                dict(starts=np.zeros((4, 3)), ends=np.zeros((4, 3)), ray_radius=float("nan")),
                dict(starts=np.zeros((4, 3)), ends=np.zeros((4, 3)), ray_colors=np.zeros((3, 3), np.uint8))):
        with pytest.raises(ValueError):
            check(**bad)


def test_the_pipeline_takes_the_flag_and_refuses_to_group_under_it():
    import inspect

    from mvlm_amd.pipeline.general_pipeline import Pipeline

    sig = inspect.signature(Pipeline.__init__).parameters
    assert sig["visualize_rays_img"].default is False
    assert tuple(map(tuple, sig["visualize_rays_poses"].default)) == ((0, 0, 0), (0, 60, 0), (0, -60, 0))
    from mvlm_amd.__main__ import build_parser

    args = build_parser().parse_args(["-p", "x", "--visualize-rays", "--visualize-size", "512"])
    assert args.visualize_rays and args.visualize_size == 512
    assert not build_parser().parse_args(["-p", "x"]).visualize_rays
