"""Numpy model of the per-landmark quality report (mvlm_consensus_report, mvlm_surface_attach), built from the oracle's own
functions: ``oracle.estimator.compute_intersection_between_lines``, ``_sq_dist_to_lines`` and ``line_mask`` (the reference's
estimator3d.py:92-137, :140-155, :174-176 and utils3d.py:99-124 restated) and ``oracle.surface.closest_point_on_triangles``.
It imports nothing from mvlm_amd.  tests/test_report_cpu.py pins it to the reference's recorded results
(tests/golden/estimator.npz) before tests/test_gpu_report.py lets it judge the kernels.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from oracle import estimator as oest
from oracle.surface import closest_point_on_triangles

KEPT, DRAWN, INLIER, USED = 1, 2, 4, 8
FIXTURE_TAGS = ("q64", "q8", "qfail", "abs", "absfew", "q128x478")


def consensus_report(starts, ends, masks, draws):
    """starts / ends f64[NL,N,3], masks bool[NL,N], draws int[NL,8] (rows of landmarks with fewer than 3 surviving lines are
    ignored) -> dict of arrays.  The consensus is ``oracle.estimator.ransac_with_draw`` / the k < 3 branch of
    ``estimate_landmarks_from_lines`` step by step, with what they decide kept."""
    nl, n = masks.shape
    r = {"point": np.zeros((nl, 3)), "error": np.zeros(nl), "k": np.zeros(nl, int), "n_inliers": np.zeros(nl, int),
         "n_used": np.zeros(nl, int), "branch": np.zeros(nl, int), "rms": np.full(nl, np.nan), "max_dist": np.full(nl, np.nan),
         "sigma2": np.full(nl, np.nan), "cov": np.full((nl, 3, 3), np.nan), "dist2": np.zeros((nl, n)),
         "flags": np.zeros((nl, n), np.uint8), "gap": np.full(nl, np.inf), "cond": np.full(nl, np.nan)}
    with np.errstate(all="ignore"):
        for lm in range(nl):
            idx = np.nonzero(masks[lm])[0]
            pa, pb = starts[lm][idx], ends[lm][idx]
            k = len(idx)
            flags = np.zeros(n, np.uint8)
            flags[idx] |= KEPT
            used = np.ones(k, bool)
            if k < 3:
                p, err, branch, n_in = oest.compute_intersection_between_lines(pa, pb), 0.0, 0, 0
            else:
                ran = np.asarray(draws[lm])
                flags[idx[ran]] |= DRAWN
                p = oest.compute_intersection_between_lines(pa[ran, :], pb[ran, :])
                distances = oest._sq_dist_to_lines(p, pa, pb)
                r["gap"][lm] = np.abs(distances - 100).min()
                inl = distances < 10 * 10
                n_in = int(np.sum(inl))
                flags[idx[inl]] |= INLIER
                err, branch = 100000000, 2
                if n_in > k / 3:
                    p_est = oest.compute_intersection_between_lines(pa[inl, :], pb[inl, :])
                    sum_squared = np.sum(oest._sq_dist_to_lines(p_est, pa[inl, :], pb[inl, :])) / n_in
                    if sum_squared < err:
                        err, p, branch, used = sum_squared, p_est, 1, inl
                if branch == 2:
                    p = oest.compute_intersection_between_lines(pa, pb)
            flags[idx[used]] |= USED
            n_used = int(used.sum())
            d2 = oest._sq_dist_to_lines(p, starts[lm], ends[lm])
            du = d2[idx[used]]
            si = pb[used] - pa[used]
            ni = si / np.sqrt(np.sum(si ** 2, 1))[:, None]
            a = n_used * np.eye(3) - ni.T @ ni  # sum over the used lines of (I - n n^T)
            r["point"][lm], r["error"][lm], r["k"][lm], r["n_inliers"][lm] = p, err, k, n_in
            r["n_used"][lm], r["branch"][lm], r["dist2"][lm], r["flags"][lm] = n_used, branch, d2, flags
            if n_used > 0:
                r["rms"][lm], r["max_dist"][lm] = np.sqrt(np.mean(du)), np.sqrt(np.max(du))
                r["cond"][lm] = np.linalg.cond(a)
            if 2 * n_used > 3:
                r["sigma2"][lm] = np.sum(du) / (2 * n_used - 3)
            r["cov"][lm] = r["sigma2"][lm] * np.linalg.pinv(a)
    return r


def fixture_case(g, tag):
    """One ``fuse_*`` case of tests/golden/estimator.npz -> (scores [NL,N], starts, ends, masks, draws int[NL,8]): the rays by
    the oracle, the masks by ``line_mask``, the draws as the reference's own run recorded them (landmark order, one per
    landmark with at least 3 surviving lines)."""
    lms, poses = g[f"fuse_{tag}_lms"], g[f"fuse_{tag}_poses"]
    mode = ["quantile", "absolute"][int(g[f"fuse_{tag}_cfg"][0])]
    q, thr = float(g[f"fuse_{tag}_cfg"][1]), float(g[f"fuse_{tag}_cfg"][2])
    starts, ends = oest.estimate_landmark_lines(256, lms, poses)
    masks = np.stack([oest.line_mask(lms[lm, :, 2], mode, q, thr) for lm in range(len(lms))])
    draws, draw_k, j = np.zeros((len(lms), 8), int), [], 0
    for lm in range(len(lms)):
        if masks[lm].sum() >= 3:
            draws[lm] = g[f"fuse_{tag}_draws"][j]
            draw_k.append(int(masks[lm].sum()))
            j += 1
    assert j == len(g[f"fuse_{tag}_draws"])
    return lms[:, :, 2], starts, ends, masks, draws, np.array(draw_k, int)


def synthetic_rays(nl: int, n: int, seed: int):
    """Rays through seeded planted points: every view's line passes its landmark's point at a seeded distance - about one
    unit for most, 25..90 units for a seeded share of outliers that differs from landmark to landmark (0 .. 0.9, so that all
    three branches occur) - in a seeded direction.  masks: a seeded 60 % of the views; with nl > 2, landmark 1 keeps no view
    and landmark 2 exactly one.  -> (starts, ends, masks, draws)."""
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-90, 90, size=(nl, 1, 3))
    d = rs.normal(size=(nl, n, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    off = np.cross(d, rs.normal(size=(nl, n, 3)))
    off /= np.linalg.norm(off, axis=2, keepdims=True)
    share = rs.uniform(0, 0.9, size=(nl, 1))
    outlier = rs.uniform(size=(nl, n)) < share
    dist = np.where(outlier, rs.uniform(25, 90, size=(nl, n)), np.abs(rs.normal(size=(nl, n))))
    mid = pts + off * dist[:, :, None]
    starts, ends = mid + 500.0 * d, mid - 500.0 * d
    masks = rs.uniform(size=(nl, n)) < 0.6
    if nl > 2:
        masks[1] = False
        masks[2] = False
        masks[2, rs.randint(n)] = True
    draws = np.zeros((nl, 8), int)
    for lm in range(nl):
        k = int(masks[lm].sum())
        if k >= 3:
            draws[lm] = rs.randint(0, k, size=8)
    return starts, ends, masks, draws


# ---- surface attachment ---------------------------------------------------------------------------------------------
def barycentric(p, a, b, c):
    """The walk of ``closest_point_on_triangles`` for one triangle, answering with the weights of (a, b, c): vertex regions
    (1,0,0) ..., edge regions (1 - t, t) on the edge's two corners, face (1 - v - w, v, w) with the first weight kept from rounding below 0."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    bp = p - b
    d3, d4 = ab @ bp, ac @ bp
    cp = p - c
    d5, d6 = ab @ cp, ac @ cp
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        if d1 <= 0 and d2 <= 0:
            return np.array([1.0, 0.0, 0.0])
        if d3 >= 0 and d4 <= d3:
            return np.array([0.0, 1.0, 0.0])
        if vc <= 0 and d1 >= 0 and d3 <= 0 and d1 - d3 > 0:
            t = d1 / (d1 - d3)
            return np.array([1.0 - t, t, 0.0])
        if d6 >= 0 and d5 <= d6:
            return np.array([0.0, 0.0, 1.0])
        if vb <= 0 and d2 >= 0 and d6 <= 0:
            t = d2 / (d2 - d6)
            return np.array([1.0 - t, 0.0, t])
        if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
            t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
            return np.array([0.0, 1.0 - t, t])
        denom = 1.0 / (va + vb + vc)
        v, w = vb * denom, vc * denom
        return np.array([max(0.0, 1.0 - v - w), v, w])


def attach(verts, tris, uvs, pts):
    """verts f32[V,3], tris int[T,3], uvs f32[V,2] | None, pts f64[n,3] -> (snapped, tri, bary, uv) as
    ``oracle.surface.project_landmarks_to_surface`` chooses: the first minimum of the finite squared distances."""
    v = verts.astype(np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    n = len(pts)
    snapped, tri = np.copy(pts), np.full(n, -1, int)
    bary, uv = np.full((n, 3), np.nan), np.full((n, 2), np.nan)
    for i in range(n):
        with np.errstate(all="ignore"):
            q, d2 = closest_point_on_triangles(pts[i], a, b, c)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        if np.isfinite(d2).any():
            t = int(np.argmin(d2))
            snapped[i], tri[i] = q[t], t
            bary[i] = barycentric(pts[i], a[t], b[t], c[t])
            if uvs is not None:
                uv[i] = bary[i] @ uvs[tris[t]].astype(np.float64)
    return snapped, tri, bary, uv
