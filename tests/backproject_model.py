"""The checker of the surface heat (mvlm_surface_heat; DESIGN.md 5.1, "Surface heat"): an independent numpy / float64 restatement of
the contract, which does not share csrc/surface_backproject_math.h.  tests/test_backproject_cpu.py holds it against hand-computed
cases, tests/test_gpu_backproject.py holds the kernels against it, exactly."""
from __future__ import annotations

import numpy as np

F = np.float32
GREY = (200, 200, 200)


def transform(rot, verts, sub_bits: int = 8):
    """Where the render puts vertices [V,3] in the view of rotation ``rot`` [3,3]: (X, Y) int64 in 1/256 pixel, y up, and the
    z-buffer value float32 - the double-precision rotation rounded to float32, the window of 300 units on 256 pixels, the snap to
    2^-sub_bits pixel.  Rows of non-finite vertices hold zeros (``finite`` says which)."""
    verts = np.asarray(verts, F).reshape(-1, 3)
    finite = np.isfinite(verts).all(axis=1)
    p = np.where(finite[:, None], verts, F(0)).astype(np.float64)
    m = np.asarray(rot, np.float64).reshape(3, 3)
    xv, yv, zv = (((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]).astype(F) for r in range(3))
    k, sub = F(256.0) / F(300.0), F(1 << sub_bits)
    lim = F((1 << 22) >> (8 - sub_bits))
    fx = np.clip(np.floor(((xv + F(150.0)) * k) * sub + F(0.5)), -lim, lim)
    fy = np.clip(np.floor(((yv + F(150.0)) * k) * sub + F(0.5)), -lim, lim)
    step = 256 >> sub_bits
    z = (F(500.0) - zv) / F(1500.0)
    assert z.dtype == F and fx.dtype == F
    return fx.astype(np.int64) * step, fy.astype(np.int64) * step, z, finite


def visibility(rot, verts, depth_plane, depth_tol: int = 2, sub_bits: int = 8):
    """(visible bool [V], row int [V], col int [V]) of vertices in one view whose depth plane is ``depth_plane`` float32 [256,256]
    (``images[n, :, :, 3]``); row / col are 0 where the vertex is outside."""
    X, Y, z, finite = transform(rot, verts, sub_bits)
    i, j = X // 256, Y // 256  # (floor division)
    inside = finite & (i >= 0) & (i < 256) & (j >= 0) & (j < 256) & (z >= F(0)) & (z <= F(1))
    row, col = np.where(inside, 255 - j, 0), np.where(inside, i, 0)
    t_v = np.trunc(255.0 * z.astype(np.float64)).astype(np.int64)
    byte = np.trunc(np.asarray(depth_plane, F)[row, col] * F(255.0) + F(0.5)).astype(np.int64)
    t_pix = (256 - byte) & 255
    return inside & (t_v <= t_pix + int(depth_tol)), row, col


def plane_peaks(heat) -> np.ndarray:
    """float32 [N,NL]: each plane's largest finite value, -inf without one."""
    h = np.asarray(heat, F)
    return np.where(np.isfinite(h), h, F(-np.inf)).max(axis=(2, 3))


def scores(verts, rot, images, heat, depth_tol: int = 2, sub_bits: int = 8):
    """(score float32 [V,NL], n_visible int32 [V]): per view in ascending order the share max(h / m, 0) of the heat value at the
    vertex's pixel in its plane's peak - 0 where the peak is not finite and above 0 or the value is not finite -, summed in
    float64 over the views that see the vertex and divided by their number."""
    verts = np.asarray(verts, F).reshape(-1, 3)
    heat = np.asarray(heat, F)
    n_views, n_lm = heat.shape[:2]
    peaks = plane_peaks(heat)
    total = np.zeros((len(verts), n_lm), np.float64)
    n_vis = np.zeros(len(verts), np.int32)
    for n in range(n_views):
        vis, row, col = visibility(np.asarray(rot, np.float64).reshape(-1, 3, 3)[n], verts, np.asarray(images, F)[n, :, :, 3], depth_tol,
                                   sub_bits)
        n_vis += vis
        for l in range(n_lm):
            m = peaks[n, l]
            if not (np.isfinite(m) and m > 0):
                continue
            h = heat[n, l][row, col]
            with np.errstate(invalid="ignore", divide="ignore"):
                t = np.maximum(h.astype(np.float64) / np.float64(m), 0.0)
            total[:, l] = total[:, l] + np.where(vis & np.isfinite(h), t, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = np.where(n_vis[:, None] > 0, total / n_vis[:, None].astype(np.float64), 0.0).astype(F)
    return score, n_vis


def base_colours(mesh) -> np.ndarray:
    """uint8 [V,3]: the vertex's own colour where the mesh is drawn with colours (it has them and no usable texture); else the
    nearest texel of its texture coordinates (GL_REPEAT, rows top first while v = 0 is the bottom); else (200, 200, 200)."""
    textured = mesh.uvs is not None and mesh.texture is not None
    if mesh.colors is not None and not textured:
        return np.asarray(mesh.colors, np.uint8).reshape(-1, 3).copy()
    if textured:
        tex = np.asarray(mesh.texture, np.uint8)
        th, tw = tex.shape[:2]
        uv = np.asarray(mesh.uvs, F)
        frac = uv - np.floor(uv)
        tx = np.clip((frac[:, 0] * F(tw)).astype(np.int64), 0, tw - 1)
        ty = np.clip((frac[:, 1] * F(th)).astype(np.int64), 0, th - 1)
        return tex[th - 1 - ty, tx].copy()
    return np.tile(np.asarray(GREY, np.uint8), (mesh.n_verts, 1))


def paint(score, base, selected=None, colors=None, floor: float = 0.25, opacity: float = 0.75) -> np.ndarray:
    """uint8 [V,4]: per vertex the selected landmark of the largest score (the lowest index on a tie) laid over ``base`` in its
    colour with opacity * (score - floor) / (1 - floor); a score <= floor leaves the base.  Alpha 255."""
    score = np.asarray(score, F)
    n_verts, n_lm = score.shape
    sel = np.ones(n_lm, bool) if selected is None else np.isin(np.arange(n_lm), list(selected))
    lm_rgb = np.tile(np.array([255, 0, 0], np.uint8), (n_lm, 1)) if colors is None else np.asarray(colors, np.uint8)
    out = np.full((n_verts, 4), 255, np.uint8)
    out[:, :3] = base
    if not sel.any():
        return out
    masked = np.where(sel[None, :], score, F(-1))
    winner = masked.argmax(axis=1)  # (the first of equal maxima)
    s = masked[np.arange(n_verts), winner].astype(np.float64)
    a = float(opacity) * (s - float(floor)) / (1.0 - float(floor))
    b = np.asarray(base, np.uint8).astype(np.float64)
    laid = np.trunc(b + a[:, None] * (lm_rgb[winner].astype(np.float64) - b) + 0.5)
    draw = s > float(floor)
    out[draw, :3] = laid[draw].astype(np.uint8)
    return out


def surface_peaks(score):
    """(peak_vertex int32 [NL], peak_score float32 [NL]): per landmark the vertex of the largest score above 0, the lowest id on a
    tie; -1 and 0 where no score is above 0."""
    score = np.asarray(score, F)
    v = score.argmax(axis=0).astype(np.int32)
    s = score[v, np.arange(score.shape[1])]
    none = ~(s > 0)
    return np.where(none, np.int32(-1), v).astype(np.int32), np.where(none, F(0), s).astype(F)


def surface_heat(mesh, rot, images, heat, selected=None, colors=None, floor=0.25, opacity=0.75, depth_tol=2, sub_bits=8) -> dict:
    """What ``HipRenderer3D.surface_heat(..., return_scores=True)`` returns, as numpy arrays."""
    score, n_vis = scores(mesh.verts, rot, images, heat, depth_tol, sub_bits)
    peak_vertex, peak_score = surface_peaks(score)
    return {"scores": score, "n_visible": n_vis, "colors": paint(score, base_colours(mesh), selected, colors, floor, opacity),
            "peak_vertex": peak_vertex, "peak_score": peak_score}
