"""The view-sheet contract ("View sheet") restated in numpy: the checker of mvlm_view_sheet_layout and of
mvlm_render_view_sheet.  It shares nothing with mvlm_amd/csrc/view_sheet_math.h.

Layout: cols = ceil(sqrt(N)) unless given, rows = ceil(N / cols), view v in cell (v // cols, v % cols), a cell 256 * scale pixels a
side, gap pixels between cells and around the sheet, grey (128, 128, 128) like the cells beyond N.  A cell's sheet pixel (y, x) shows
view pixel (y // scale, x // scale): planes 0..2 ("rgb") or plane 3 three times ("depth"), a byte = int(p * 255 + 0.5) in float32,
cut to 0..255.  A prediction (a, b, score) stands at X = b, Y = a + 1 view pixels from the cell's left / top edge; the sheet pixel
(j, i) with centre (i + 0.5, j + 0.5) is covered iff dx^2 + dy^2 <= (R scale)^2, dx = (i + 0.5) - scale X; with used == 0 only where
also d^2 > (R scale - max(1, scale))^2 (everywhere when that inner radius is negative).  The residual runs from (X, Y) to X' = (q.x +
150) * 256 / 300, Y' = 256 - (q.y + 150) * 256 / 300 with q = M p; it covers the pixels whose centre is within max(0.5, scale / 2)
of the segment (t = clamp(w.v / v.v, 0, 1), c = w - t v, |c|^2 <= hw^2; t = 0 when v.v == 0).  Order: background, residuals (red),
markers; landmark order within each.  All float64, one rounding per operation."""
import math

import numpy as np

VIEW = 256
GREY = (128, 128, 128)
RED = (255, 0, 0)
BLUE = (0, 0, 255)
LIMIT = 4096


def layout(n_views: int, cols=None, scale: int = 1, gap: int = 2):
    """-> (cols, rows, width, height); ValueError for what the contract refuses (the message names the largest scale that fits)."""
    if n_views < 1:
        raise ValueError("n_views")
    if cols is not None and cols < 1:
        raise ValueError("cols")
    if not 1 <= scale <= 4:
        raise ValueError("scale")
    if not 0 <= gap <= 16:
        raise ValueError("gap")
    c = cols if cols is not None else math.isqrt(n_views - 1) + 1 if n_views > 1 else 1
    r = -(-n_views // c)

    def extent(s):
        return c * VIEW * s + (c + 1) * gap, r * VIEW * s + (r + 1) * gap

    w, h = extent(scale)
    if max(w, h) > LIMIT:
        fits = [s for s in (4, 3, 2, 1) if max(extent(s)) <= LIMIT]
        raise ValueError(f"too large: largest scale {fits[0] if fits else None}")
    return c, r, w, h


def auto_background(chan_sel) -> str:
    return "rgb" if any(int(c) < 3 for c in chan_sel) else "depth"


def plane_bytes(images) -> np.ndarray:
    """float32 [...] -> uint8: int(p * 255 + 0.5) in float32, cut to 0..255 (NaN: 0)."""
    p = np.asarray(images, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = p * np.float32(255.0) + np.float32(0.5)
        v = np.where(v >= np.float32(0.0), v, np.float32(0.0))
        v = np.where(v > np.float32(255.0), np.float32(255.0), v)
    return v.astype(np.int32).astype(np.uint8)


def marker_position(a, b):
    """(X, Y): continuous view pixels from the cell's left and top edge."""
    return float(np.float32(b)), float(np.float32(a)) + 1.0


def project(m, p):
    """Rotation f64[9] (row-major Ry Rx Rz), landmark f64[3] -> (X', Y')."""
    m = [float(x) for x in np.asarray(m, np.float64).ravel()]
    p = [float(x) for x in np.asarray(p, np.float64).ravel()]
    qx = (m[0] * p[0] + m[1] * p[1]) + m[2] * p[2]
    qy = (m[3] * p[0] + m[4] * p[1]) + m[5] * p[2]
    return ((qx + 150.0) * 256.0) / 300.0, 256.0 - ((qy + 150.0) * 256.0) / 300.0


def _window(lo: float, hi: float, side: int):
    a, b = max(0, math.floor(lo) - 2), min(side - 1, math.ceil(hi) + 2)
    return (a, b) if a <= b else None


def _centres(win_x, win_y):
    i = np.arange(win_x[0], win_x[1] + 1, dtype=np.float64)[None, :] + 0.5
    j = np.arange(win_y[0], win_y[1] + 1, dtype=np.float64)[:, None] + 0.5
    return i, j


def marker_mask(X: float, Y: float, radius: float, scale: int, used: bool = True):
    """-> (rows slice, cols slice, bool mask) of the covered pixels of the cell, or None."""
    side, s = VIEW * scale, float(scale)
    sx, sy, rr = s * X, s * Y, float(radius) * s
    wx, wy = _window(sx - rr, sx + rr, side), _window(sy - rr, sy + rr, side)
    if wx is None or wy is None:
        return None
    ci, cj = _centres(wx, wy)
    dx, dy = ci - sx, cj - sy
    d2 = dx * dx + dy * dy
    mask = d2 <= rr * rr
    if not used:
        inner = rr - float(max(1, scale))
        if inner >= 0.0:
            mask &= d2 > inner * inner
    return slice(wy[0], wy[1] + 1), slice(wx[0], wx[1] + 1), mask


def segment_mask(X: float, Y: float, Xp: float, Yp: float, scale: int):
    side, s = VIEW * scale, float(scale)
    ax, ay, bx, by = s * X, s * Y, s * Xp, s * Yp
    hw = max(0.5, 0.5 * s)
    wx, wy = _window(min(ax, bx) - hw, max(ax, bx) + hw, side), _window(min(ay, by) - hw, max(ay, by) + hw, side)
    if wx is None or wy is None:
        return None
    ci, cj = _centres(wx, wy)
    vx, vy = bx - ax, by - ay
    px, py = ci - ax, cj - ay
    l2 = vx * vx + vy * vy
    with np.errstate(invalid="ignore", over="ignore"):
        if l2 > 0.0:
            t = (px * vx + py * vy) / l2
            t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        else:
            t = np.zeros(np.broadcast(px, py).shape)
        cx, cy = px - t * vx, py - t * vy
        mask = (cx * cx + cy * cy) <= hw * hw
    return slice(wy[0], wy[1] + 1), slice(wx[0], wx[1] + 1), mask


def pixels(hit) -> set:
    """A mask triple -> {(x, y)} cell pixels."""
    if hit is None:
        return set()
    rows, cols, mask = hit
    jj, ii = np.nonzero(mask)
    return {(int(i) + cols.start, int(j) + rows.start) for i, j in zip(ii, jj)}


def render(images, maxima=None, rot=None, landmarks=None, colors=None, used=None, background="rgb", cols=None, scale=1, gap=2,
           marker_radius=2.0) -> np.ndarray:
    """-> uint8 [H,W,3], what render_view_sheet gives."""
    images = np.asarray(images, np.float32)
    n = images.shape[0]
    c, r, w, h = layout(n, cols, scale, gap)
    side = VIEW * scale
    sheet = np.empty((h, w, 3), np.uint8)
    sheet[...] = GREY
    planes = plane_bytes(images)
    nl = 0 if maxima is None else int(np.asarray(maxima).shape[0])
    mx = None if maxima is None else np.asarray(maxima, np.float32)
    residuals = nl > 0 and rot is not None and landmarks is not None
    if residuals:
        rot = np.asarray(rot, np.float64).reshape(n, 9)
        landmarks = np.asarray(landmarks, np.float64).reshape(nl, 3)
    colors = None if colors is None else np.asarray(colors, np.uint8).reshape(nl, 3)
    used = None if used is None else np.asarray(used, np.uint8).reshape(nl, n)
    for v in range(n):
        bg = planes[v, :, :, :3] if background == "rgb" else np.repeat(planes[v, :, :, 3:4], 3, axis=2)
        cell = np.repeat(np.repeat(bg, scale, axis=0), scale, axis=1).copy()
        ok = [bool(np.isfinite(mx[l, v]).all()) for l in range(nl)]
        pos = [marker_position(mx[l, v, 0], mx[l, v, 1]) if ok[l] else None for l in range(nl)]
        if residuals:
            for l in range(nl):
                if not ok[l] or not np.isfinite(landmarks[l]).all():
                    continue
                xp, yp = project(rot[v], landmarks[l])
                if not (math.isfinite(scale * xp) and math.isfinite(scale * yp)):
                    continue
                hit = segment_mask(pos[l][0], pos[l][1], xp, yp, scale)
                if hit is not None:
                    cell[hit[0], hit[1]][hit[2]] = RED
        for l in range(nl):
            if not ok[l]:
                continue
            hit = marker_mask(pos[l][0], pos[l][1], marker_radius, scale, True if used is None else bool(used[l, v]))
            if hit is not None:
                cell[hit[0], hit[1]][hit[2]] = BLUE if colors is None else colors[l]
        y0, x0 = gap + (v // c) * (side + gap), gap + (v % c) * (side + gap)
        sheet[y0:y0 + side, x0:x0 + side] = cell
    return sheet
